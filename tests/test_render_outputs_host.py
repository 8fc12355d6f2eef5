"""CPU checks of the differentiable render outputs: the extended autograd oracle (tests/render_outputs_ref.py), the binding
of the three new entry points, and the torch bridge against a fake Context that records its calls."""
import os
import re

import numpy as np
import pytest
import torch

import render_outputs_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nerf_train_render_forward_outputs", "nerf_train_render_backward_outputs", "nerf_render_output_grads")


def _setup(oracle, golden_ckpt, n=12, sc=8, sf=10):
    rng = np.random.default_rng(0)
    c2w = oracle.get_sphere_matrix(1.0, -20, 30, 0).astype(np.float32)
    d = oracle.get_rays_directions(6, 6, 0.46, c2w).reshape(-1, 4)[:n]
    o = np.tile(c2w[:, 3], (n, 1)).astype(np.float32)
    return dict(o=o, d=d, u_c=rng.random((n, sc), dtype=np.float32), u_f=rng.random((n, sf), dtype=np.float32),
                near=float(golden_ckpt["near"]), far=float(golden_ckpt["far"]), bc=golden_ckpt["blob_coarse"],
                bf=golden_ckpt["blob_fine"], n=n, s=sc + sf)


def _cotangents(p, seed=4):
    rng = np.random.default_rng(seed)
    n, s = p["n"], p["s"]
    return dict(d_rgb=rng.standard_normal((n, 3)), d_depth=rng.standard_normal(n), d_weights=rng.standard_normal((n, s)),
                d_z=rng.standard_normal((n, s)))


def test_fold_restatement_is_float32_with_separate_roundings():
    rng = np.random.default_rng(0)
    w, z = rng.random((3, 5), dtype=np.float32), rng.random((3, 5), dtype=np.float32) + 1
    dd, dw, dz = (rng.standard_normal(s).astype(np.float32) for s in ((3,), (3, 5), (3, 5)))
    gw, gz = R.fold(w, z, dd, dw, dz)
    assert gw.dtype == np.float32 and gz.dtype == np.float32
    # element by element with explicit float32 scalars: product rounded, then the sum rounded
    for r in range(3):
        for s in range(5):
            assert gw[r, s] == np.float32(dw[r, s] + np.float32(dd[r] * z[r, s]))
            assert gz[r, s] == np.float32(dz[r, s] + np.float32(dd[r] * w[r, s]))
    g0w, g0z = R.fold(w, z)
    assert not g0w.any() and not g0z.any()
    np.testing.assert_array_equal(R.fold(w, z, d_weights=dw)[0], dw)
    np.testing.assert_array_equal(R.fold(w, z, d_z=dz)[1], dz)


def test_extended_oracle_with_d_rgb_alone_is_render_gradients(oracle, golden_ckpt):
    from oracle import train_oracle as T
    p = _setup(oracle, golden_ckpt)
    d_rgb = _cotangents(p)["d_rgb"]
    for sampler_grad in (True, False):
        a = R.render_outputs_gradients(p["bc"], p["bf"], p["o"], p["d"], p["near"], p["far"], p["u_c"], p["u_f"], d_rgb=d_rgb,
                                       sampler_grad=sampler_grad)
        b = T.render_gradients(p["bc"], p["bf"], p["o"], p["d"], d_rgb, p["near"], p["far"], p["u_c"], p["u_f"],
                               sampler_grad=sampler_grad)
        for k in ("rgb", "grad_coarse", "grad_fine"):
            np.testing.assert_array_equal(a[k], b[k])
    # the outputs are what they say: depth = sum w z, z sorted, weights sum to 1 (the 1e9 last interval)
    np.testing.assert_allclose(a["depth"], (a["weights"] * a["z"]).sum(-1), rtol=0, atol=1e-14)
    assert (np.diff(a["z"], axis=-1) >= 0).all() and a["z"].shape == (p["n"], p["s"])
    assert np.abs(a["weights"].sum(-1) - 1).max() <= 1e-12


def test_extended_oracle_gradients_by_central_differences(oracle, golden_ckpt):
    from oracle import train_oracle as T
    p = _setup(oracle, golden_ckpt)
    cot = _cotangents(p)
    args = (p["o"], p["d"], p["near"], p["far"], p["u_c"], p["u_f"])
    r = R.render_outputs_gradients(p["bc"], p["bf"], *args, **cot)
    tc = [torch.tensor(np.asarray(cot[k])) for k in ("d_rgb", "d_depth", "d_weights", "d_z")]

    def loss_at(bc64, bf64):
        pc = [t.detach() for t in T.blob_to_params(p["bc"])]
        pf = [t.detach() for t in T.blob_to_params(p["bf"])]
        for params, blob in ((pc, bc64), (pf, bf64)):
            off = 0
            for t in params:
                t.copy_(torch.tensor(blob[off:off + t.numel()].reshape(t.shape)))
                off += t.numel()
        with torch.no_grad():
            outs = R.render_outputs_forward(pc, pf, *args)
            return float(sum((o * c).sum() for o, c in zip(outs, tc)))

    bc64, bf64 = p["bc"].astype(np.float64), p["bf"].astype(np.float64)
    assert abs(loss_at(bc64, bf64) - r["loss"]) <= 1e-12 * max(1.0, abs(r["loss"]))
    rng = np.random.default_rng(1)
    for which, g in ((0, r["grad_coarse"]), (1, r["grad_fine"])):
        picks = list(np.argsort(-np.abs(g))[:3]) + [g.size - 1] + list(rng.choice(g.size, 2))
        for i in picks:
            h = 1e-5
            blobs = [bc64.copy(), bf64.copy()]
            blobs[which][i] += h
            up = loss_at(*blobs)
            blobs[which][i] -= 2 * h
            fd = (up - loss_at(*blobs)) / (2 * h)
            # central differences straddle LeakyReLU / relu / bin-selection kinks: a structural check, 1 % bar
            assert abs(fd - g[i]) <= 1e-5 * np.abs(g).max() + 1e-2 * abs(g[i]), (which, i, fd, g[i])
    # where the new cotangents act: d_z alone moves only the coarse network, and only through the sampler
    rz = R.render_outputs_gradients(p["bc"], p["bf"], *args, d_z=cot["d_z"])
    assert not rz["grad_fine"].any() and rz["grad_coarse"].any()
    rz0 = R.render_outputs_gradients(p["bc"], p["bf"], *args, d_z=cot["d_z"], sampler_grad=False)
    assert not rz0["grad_fine"].any() and not rz0["grad_coarse"].any()
    # ... and a coarse-only render does not see d_z at all
    a = R.render_outputs_gradients(p["bc"], None, *args, d_depth=cot["d_depth"], d_weights=cot["d_weights"][:, :8])
    b = R.render_outputs_gradients(p["bc"], None, *args, d_depth=cot["d_depth"], d_weights=cot["d_weights"][:, :8],
                                   d_z=cot["d_z"][:, :8])
    np.testing.assert_array_equal(a["grad_coarse"], b["grad_coarse"])
    assert a["grad_coarse"].any()


def test_gradient_sets_share_one_forward_and_equal_the_single_calls(oracle, golden_ckpt):
    p = _setup(oracle, golden_ckpt)
    cot = _cotangents(p)
    args = (p["bc"], p["bf"], p["o"], p["d"], p["near"], p["far"], p["u_c"], p["u_f"])
    sets = {"d_depth": {"d_depth": cot["d_depth"]}, "d_z": {"d_z": cot["d_z"]}, "all": cot}
    many = R.render_outputs_gradient_sets(*args, sets)
    for name, kw in sets.items():
        one = R.render_outputs_gradients(*args, **kw)
        np.testing.assert_array_equal(many["grads"][name][0], one["grad_coarse"])
        np.testing.assert_array_equal(many["grads"][name][1], one["grad_fine"])
        np.testing.assert_array_equal(many["depth"], one["depth"])


def test_new_entry_points_are_declared_bound_wrapped_and_exported():
    import nerf_and_dietnerf_amd as N
    text = open(os.path.join(ROOT, "include", "nerf_mi355.h")).read()
    declared = set(re.findall(r"\b(nerf_[a-z_]+)\s*\(", text))
    bound = {name: args for name, _, args in N._lib.SYMBOLS}
    lib = N._lib.load()
    for name in NEW:
        assert name in declared, name
        assert name in bound, name
        assert getattr(lib, name) is not None
    assert re.search(r"#define\s+NERF_ABI_VERSION\s+6\b", text) and N._lib.NERF_ABI_VERSION == 6 and lib.nerf_abi_version() == 6
    # the structs as the header lays them out: four pointers each, in this order
    for struct, fields in (("nerf_train_outputs", ("rgb", "depth", "weights", "z")),
                           ("nerf_render_grads", ("d_rgb", "d_depth", "d_weights", "d_z"))):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
        assert tuple(re.findall(r"float\*\s+(\w+);", body)) == fields
    assert [f for f, _ in N._lib.NerfTrainOutputs._fields_] == ["rgb", "depth", "weights", "z"]
    assert [f for f, _ in N._lib.NerfRenderGrads._fields_] == ["d_rgb", "d_depth", "d_weights", "d_z"]
    assert len(bound["nerf_train_render_forward_outputs"]) == 13
    assert len(bound["nerf_train_render_backward_outputs"]) == 7
    assert len(bound["nerf_render_output_grads"]) == 11
    for method in ("train_render_forward_outputs", "train_render_backward_outputs", "render_output_grads"):
        assert callable(getattr(N.Context, method))
    assert callable(N.NeRF.train_step_custom)
    assert N.render_with_grad is N.autograd.render_with_grad


class _FakeContext:
    """Stands in for Context behind the bridge: records every call, hands out fixed outputs, keeps the slot rule."""
    MESSAGE = "slot 3 holds no forward pass (nerf_train_render_forward first; a backward pass consumes it, and so does an optimizer step)"

    def __init__(self, n=5, s=7):
        self.n, self.s, self.calls, self.valid = n, s, [], set()

    def train_render_forward_outputs(self, slot, rays_orig, rays_dirs, n_c, n_f, u_coarse=None, u_fine=None, seed=0, ray_base=0,
                                     outputs=("rgb", "depth", "weights", "z")):
        self.calls.append(("forward", dict(slot=slot, n_c=n_c, n_f=n_f, seed=seed, ray_base=ray_base, outputs=tuple(outputs),
                                           u_coarse=u_coarse, u_fine=u_fine)))
        self.valid.add(slot)
        g = torch.Generator().manual_seed(0)
        shapes = {"rgb": (self.n, 3), "depth": (self.n,), "weights": (self.n, self.s), "z": (self.n, self.s)}
        return {k: torch.rand(shapes[k], generator=g) for k in outputs}

    def train_render_backward_outputs(self, slot, d_rgb=None, d_depth=None, d_weights=None, d_z=None, accumulate=False,
                                      want_blobs=True):
        if slot not in self.valid:
            raise RuntimeError(self.MESSAGE)
        self.valid.discard(slot)
        self.calls.append(("backward", dict(slot=slot, d_rgb=d_rgb, d_depth=d_depth, d_weights=d_weights, d_z=d_z,
                                            accumulate=accumulate, want_blobs=want_blobs)))
        return None, None


def test_bridge_against_a_recording_context():
    import nerf_and_dietnerf_amd as N
    fake = _FakeContext()
    o, d = torch.zeros(5, 4), torch.ones(5, 4)
    out = N.render_with_grad(fake, o, d, 3, 4, slot=3, seed=11, ray_base=20, accumulate=True)
    assert set(out) == {"rgb", "depth", "weights", "z"} and all(v.requires_grad for v in out.values())
    kind, fw = fake.calls[0]
    assert kind == "forward" and fw == dict(slot=3, n_c=3, n_f=4, seed=11, ray_base=20, outputs=("rgb", "depth", "weights", "z"),
                                            u_coarse=None, u_fine=None)
    # a loss on depth and (a transposed, hence non-contiguous, view of) the weights: rgb and z are not used
    coef = torch.arange(35, dtype=torch.float32).reshape(7, 5)
    loss = (out["depth"] ** 2).sum() + (out["weights"].t() * coef).sum()
    loss.backward(retain_graph=True)
    kind, bw = fake.calls[1]
    assert kind == "backward" and bw["slot"] == 3 and bw["accumulate"] is True and bw["want_blobs"] is False
    assert bw["d_rgb"] is None and bw["d_z"] is None                       # unused outputs arrive as None
    assert bw["d_depth"].is_contiguous() and bw["d_weights"].is_contiguous()
    torch.testing.assert_close(bw["d_depth"], 2 * out["depth"].detach(), rtol=0, atol=0)
    torch.testing.assert_close(bw["d_weights"], coef.t().contiguous(), rtol=0, atol=0)
    # a second backward through the same graph: the slot is consumed, the library's message surfaces
    with pytest.raises(RuntimeError, match="holds no forward pass"):
        loss.backward()
    assert len(fake.calls) == 2

    # the anchor gets a zero; accumulate defaults to False and is forwarded as such
    fake = _FakeContext()
    fn = N.autograd._render_function()
    anchor = torch.zeros((), requires_grad=True)
    rgb = fn.apply(anchor, fake, 0, False, o, d, 3, 4, None, None, 0, 0)[0]
    rgb.sum().backward()
    assert anchor.grad is not None and anchor.grad.shape == () and float(anchor.grad) == 0.0
    bw = fake.calls[1][1]
    assert bw["accumulate"] is False and bw["d_depth"] is None and bw["d_weights"] is None and bw["d_z"] is None
    torch.testing.assert_close(bw["d_rgb"], torch.ones(5, 3), rtol=0, atol=0)
