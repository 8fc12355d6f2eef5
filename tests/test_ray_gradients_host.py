"""CPU checks of the ray gradients: header / binding / package agree on the three new entry points, rays_from_pose against
the oracle's ray generator and against central differences, and the reference-only facts the GPU bars of
tests/test_gpu_ray_gradients.py rest on (float32 autograd against float64, the share of the view-direction term and of the
sampler term), on the problems and the d_rgb of tests/test_gpu_render_outputs.py.

The figures of the float32 restatement are the measured ones, stated to two digits (3.9e-5; 1.9e-4 and 8.8e-5): they are
compared at that precision, i.e. after rounding the measurement to two significant digits."""
import os
import re

import numpy as np
import pytest
import torch

import ray_grad_ref as G
import render_outputs_ref as R
import support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"nerf_train_set_ray_gradients": 2, "nerf_train_render_backward_rays": 9, "nerf_ray_position_grads": 8}


def _two_digits(x):
    return float(f"{x:.1e}")


def _problem(oracle, ck, n, sc, sf, seed):
    """The rays and draws of support.golden_problem, as the argument tuple of the references."""
    o, d, rng = S.oracle_rays(oracle, n, seed)
    u_c, u_f = rng.random((n, sc), dtype=np.float32), rng.random((n, sf), dtype=np.float32)
    return (ck["blob_coarse"], ck["blob_fine"], o, d, float(ck["near"]), float(ck["far"]), u_c, u_f)


def _d_rgb(n, seed=3):
    """The first draw of tests/render_outputs_ref.py::cotangents."""
    return (np.random.default_rng(seed).standard_normal((n, 3)) * 0.1).astype(np.float32)


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_new_entry_points_are_declared_bound_wrapped_and_exported():
    import nerf_and_dietnerf_amd as N
    text = open(os.path.join(ROOT, "include", "nerf_mi355.h")).read()
    declared = set(re.findall(r"\b(nerf_[a-z_]+)\s*\(", text))
    bound = {name: args for name, _, args in N._lib.SYMBOLS}
    lib = N._lib.load()
    for name, nargs in NEW.items():
        assert name in declared, name
        assert name in bound and len(bound[name]) == nargs, name
        assert getattr(lib, name) is not None
    assert re.search(r"#define\s+NERF_ABI_VERSION\s+6\b", text) and N._lib.NERF_ABI_VERSION == 6 and lib.nerf_abi_version() == 6
    for method in ("train_set_ray_gradients", "ray_position_grads", "train_render_backward_outputs"):
        assert callable(getattr(N.Context, method))
    assert isinstance(N.Context.train_ray_gradients, property)
    assert N.rays_from_pose is N.pose.rays_from_pose
    # the semantics the header owes its reader
    doc = text[text.index("ray gradients: dL/d(rays_orig)"):text.index("int nerf_ray_position_grads")]
    doc = re.sub(r"\s*\n \*\s*", " ", doc)
    for phrase in ("the coarse depths are data", "nerf_train_begin leaves", "names the fused trainer", "component 3"):
        assert phrase in doc, phrase


def test_reduce_restatement():
    rng = np.random.default_rng(0)
    dp, z = rng.standard_normal((2, 3, 3)), rng.random((2, 3)) + 1
    d_o, d_d, a_o, a_d = G.position_reduce(dp, z)
    assert d_o.shape == (2, 4) and not d_o[:, 3].any() and not d_d[:, 3].any()
    for r in range(2):
        for c in range(3):
            assert abs(d_o[r, c] - sum(dp[r, s, c] for s in range(3))) <= 1e-15
            assert abs(d_d[r, c] - sum(z[r, s] * dp[r, s, c] for s in range(3))) <= 1e-15
            assert abs(a_d[r, c] - sum(abs(z[r, s] * dp[r, s, c]) for s in range(3))) <= 1e-15
    assert (a_o >= np.abs(d_o)).all()


def test_split_render_rays_is_the_oracles(oracle, golden_ckpt):
    """ray_grad_ref._render_rays with both directions the same tensor is train_oracle._render_rays, bit for bit, in the plain
    and in the fp16-emulating arithmetic."""
    from oracle import train_oracle as T
    bc, _, o, d, near, far, u_c, _ = _problem(oracle, golden_ckpt, 6, 9, 4, 1)
    pc = [t.detach() for t in T.blob_to_params(bc)]
    ot, dt = torch.tensor(o, dtype=torch.float64), torch.tensor(d, dtype=torch.float64)
    z = torch.tensor(oracle.get_z_values(near, far, u_c), dtype=torch.float64)
    for ls in (None, 2048.0):
        a = G._render_rays(pc, ot, dt, dt, z, 5, 4, 2, 0.05, ls)
        b = T._render_rays(pc, ot, dt, z, 5, 4, 2, 0.05, ls)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x.numpy(), y.numpy())
    # ... and the forward on ray tensors is the forward of render_outputs_ref
    bc, bf, o, d, near, far, u_c, u_f = _problem(oracle, golden_ckpt, 6, 9, 4, 1)
    pf = [t.detach() for t in T.blob_to_params(bf)]
    a = G.forward(pc, pf, ot, dt, near, far, u_c, u_f)
    b = R.render_outputs_forward(pc, pf, o, d, near, far, u_c, u_f)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x.numpy(), y.numpy())


def test_rays_from_pose_is_the_ray_generator(oracle, golden_ckpt):
    import nerf_and_dietnerf_amd as N
    c2w, fov = golden_ckpt["c2w_test"].astype(np.float32), float(golden_ckpt["fov"])
    want = oracle.get_rays_directions(8, 8, fov, c2w).reshape(-1, 4)
    o, d = N.rays_from_pose(torch.tensor(c2w), fov, 8, 8)
    assert o.shape == (64, 4) and d.shape == (64, 4) and o.dtype == torch.float32
    # float32 rounding: a few ulps of the largest term of each three-term sum
    scale = np.abs(c2w[:, :3]).sum(1)[None, :] * max(1.0, np.tan(fov / 2))
    assert (np.abs(d.numpy() - want) <= 4 * np.finfo(np.float32).eps * scale + 1e-30).all()
    np.testing.assert_array_equal(o.numpy(), np.tile(c2w[:, 3], (64, 1)))
    idx = [5, 63, 0, 17]
    o2, d2 = N.rays_from_pose(torch.tensor(c2w), fov, 8, 8, pixel_index=idx)
    np.testing.assert_array_equal(d2.numpy(), d.numpy()[idx])
    assert o2.shape == (4, 4)
    with pytest.raises(ValueError):
        N.rays_from_pose(torch.zeros(3, 4), fov, 8, 8)


def test_rays_from_pose_jacobian_by_central_differences(golden_ckpt):
    import nerf_and_dietnerf_amd as N
    c2w, fov = torch.tensor(golden_ckpt["c2w_test"], dtype=torch.float64), float(golden_ckpt["fov"])
    rng = np.random.default_rng(2)
    co, cd = torch.tensor(rng.standard_normal((12, 4))), torch.tensor(rng.standard_normal((12, 4)))
    idx = rng.choice(64, 12, replace=False)

    def f(m):
        o, d = N.rays_from_pose(m, fov, 8, 8, pixel_index=idx)
        return (o * co).sum() + (d * cd).sum()

    leaf = c2w.clone().requires_grad_(True)
    f(leaf).backward()
    g = leaf.grad.numpy()
    h = 1e-6
    for i in range(4):
        for j in range(4):
            e = torch.zeros_like(c2w)
            e[i, j] = h
            fd = float(f(c2w + e) - f(c2w - e)) / (2 * h)
            assert abs(fd - g[i, j]) <= 1e-8 * max(1.0, np.abs(g).max()), (i, j, fd, g[i, j])
    assert g[:, :3].any() and g[:, 3].any()


@pytest.fixture(scope="module")
def big(oracle, golden_ckpt):
    """40 x (55 + 55), seed 9, with the d_rgb of tests/test_gpu_render_outputs.py: float64 and float32 autograd, the graph
    without the view-direction input and without the sampler term, at alpha = 1 and at the trained slope."""
    args = _problem(oracle, golden_ckpt, 40, 55, 55, 9)
    sets = {"d_rgb": {"d_rgb": _d_rgb(40)}}
    run = lambda **kw: G.ray_gradient_sets(*args, sets, **kw)["grads"]["d_rgb"]                     # noqa: E731
    out = {}
    for alpha in (1.0, 0.05):
        out[alpha] = dict(f64=run(alpha=alpha), no_view=run(alpha=alpha, view_term=False), no_sampler=run(alpha=alpha, sampler_grad=False))
    out[1.0]["f32"] = run(alpha=1.0, dtype=torch.float32)
    return out


def test_float32_autograd_sits_at_the_stated_figures(big, oracle, golden_ckpt, capsys):
    e_o, e_d = _rel(big[1.0]["f32"][0], big[1.0]["f64"][0]), _rel(big[1.0]["f32"][1], big[1.0]["f64"][1])
    args = _problem(oracle, golden_ckpt, 7, 33, 32, 21)
    sets = {"d_rgb": {"d_rgb": _d_rgb(7, seed=5)}}
    g64 = G.ray_gradient_sets(*args, sets, alpha=0.05)["grads"]["d_rgb"]
    g32 = G.ray_gradient_sets(*args, sets, alpha=0.05, dtype=torch.float32)["grads"]["d_rgb"]
    r_o, r_d = _rel(g32[0], g64[0]), _rel(g32[1], g64[1])
    with capsys.disabled():
        print(f"\n[ray gradients, float32 vs float64 autograd] 40 x (55 + 55), alpha 1: d_o {e_o:.3e} d_d {e_d:.3e}; "
              f"7 x (33 + 32), alpha 0.05: d_o {r_o:.3e} d_d {r_d:.3e}", end="")
    assert _two_digits(e_o) <= 3.9e-5 and _two_digits(e_d) <= 3.9e-5
    assert _two_digits(r_o) <= 1.9e-4 and _two_digits(r_d) <= 8.8e-5
    for g in (*big[1.0]["f64"], *g64):
        assert g.shape[1] == 4 and not g[:, 3].any() and g[:, :3].any()


def test_neither_term_can_be_dropped(big, capsys):
    """What the GPU bars (2e-4 at alpha = 1, 1e-2 at alpha = 0.05) can tell apart: the view-direction input carries at least
    5e-4 of max|d_d| at alpha = 1 and at least 0.1 at alpha = 0.05, the sampler term at least 1e-2 of either tensor at
    alpha = 1; the origin does not see the view-direction input at all."""
    v1, v005 = _rel(big[1.0]["no_view"][1], big[1.0]["f64"][1]), _rel(big[0.05]["no_view"][1], big[0.05]["f64"][1])
    s_o, s_d = _rel(big[1.0]["no_sampler"][0], big[1.0]["f64"][0]), _rel(big[1.0]["no_sampler"][1], big[1.0]["f64"][1])
    with capsys.disabled():
        print(f"\n[ray gradients, shares of max|g|] view-direction term: {v1:.2e} (alpha 1), {v005:.2e} (alpha 0.05); sampler "
              f"term at alpha 1: d_o {s_o:.2e} d_d {s_d:.2e}", end="")
    assert v1 >= 5e-4 and v005 >= 0.1
    assert s_o >= 1e-2 and s_d >= 1e-2
    np.testing.assert_array_equal(big[1.0]["no_view"][0], big[1.0]["f64"][0])
