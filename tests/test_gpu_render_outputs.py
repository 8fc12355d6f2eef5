"""Differentiable render outputs on the device (include/nerf_mi355.h: nerf_train_render_forward_outputs,
nerf_train_render_backward_outputs, nerf_render_output_grads) and the torch bridge over them.

The reference of every gradient here is float64 autograd of NeRF.render()'s graph with all four outputs of the last pass
(tests/render_outputs_ref.py), differentiating L = sum(d_rgb rgb) + sum(d_depth depth) + sum(d_weights w) + sum(d_z z).
The bars are the ones tests/test_gpu_train.py::test_backward_through_render holds the d_rgb path to on the same problem
(40 rays x (55 + 55), alpha = 1: 2e-4 of max|g|, cosine > 0.9999999): on the CPU float32 autograd itself sits at 3.4e-5 /
1.8e-5 (fine / coarse) of max|g| for the combined cotangent drawn here and at 3.0e-5 .. 3.9e-5 for each new cotangent alone,
the class of the d_rgb path, so the bar carries over unchanged.
"""
import numpy as np
import pytest

import grad_blocks as GB
import occupancy_ref as O
import render_outputs_ref as R
import support as S

pytestmark = pytest.mark.gpu

BLOCKS = GB.blocks(5, 4, 2)


def _sets(cot):
    return {"d_depth": {"d_depth": cot["d_depth"]}, "d_weights": {"d_weights": cot["d_weights"]}, "d_z": {"d_z": cot["d_z"]},
            "all": dict(cot)}


@pytest.fixture(scope="module")
def big(oracle, golden_ckpt):
    """The 40 x (55 + 55) problem of test_backward_through_render, its cotangents, and -- computed once per (sampler term,
    dtype, loss scale) and shared -- the oracle's outputs and gradients for the four cotangent sets."""
    p = S.golden_problem(oracle, golden_ckpt, n=40, sc=55, sf=55, seed=9)
    p["cot"] = R.cotangents(40, 110)
    cache = {}

    def ref(sampler_grad, dtype="float64", fp16_loss_scale=None, alpha=1.0):
        import torch
        key = (sampler_grad, dtype, fp16_loss_scale, alpha)
        if key not in cache:
            cache[key] = R.render_outputs_gradient_sets(
                p["bc"], p["bf"], p["o"], p["d"], p["near"], p["far"], p["u_c"], p["u_f"], _sets(p["cot"]),
                dtype=getattr(torch, dtype), sampler_grad=sampler_grad, alpha=alpha, fp16_loss_scale=fp16_loss_scale)
        return cache[key]

    p["ref"] = ref
    return p


def test_bare_operator_is_bit_equal_to_the_numpy_restatement(golden_ckpt):
    """nerf_render_output_grads on caller data: every subset of the three cotangents absent, at sizes below, at and across
    the 256-thread block and the 64-sample chunk; host arrays and device tensors."""
    import itertools
    import torch
    import nerf_and_dietnerf_amd as N
    ctx = N.Context(near=float(golden_ckpt["near"]), far=float(golden_ckpt["far"]))
    rng = np.random.default_rng(0)
    for n, s in ((1, 1), (5, 63), (4, 64), (7, 65), (3, 257)):
        w = rng.random((n, s), dtype=np.float32)
        z = np.sort(rng.random((n, s), dtype=np.float32) + 0.5, axis=-1)
        full = dict(d_depth=rng.standard_normal(n).astype(np.float32), d_weights=rng.standard_normal((n, s)).astype(np.float32),
                    d_z=rng.standard_normal((n, s)).astype(np.float32))
        for mask in itertools.product((False, True), repeat=3):
            kw = {k: (v if on else None) for (k, v), on in zip(full.items(), mask)}
            want_w, want_z = R.fold(w, z, **kw)
            got_w, got_z = ctx.render_output_grads(w, z, **kw)
            np.testing.assert_array_equal(got_w, want_w, err_msg=f"g_w {n}x{s} {mask}")
            np.testing.assert_array_equal(got_z, want_z, err_msg=f"g_z {n}x{s} {mask}")
        dev = lambda a: torch.as_tensor(a, device="cuda")                                          # noqa: E731
        got_w, got_z = ctx.render_output_grads(dev(w), dev(z), **{k: dev(v) for k, v in full.items()})
        want_w, want_z = R.fold(w, z, **full)
        np.testing.assert_array_equal(got_w.cpu().numpy(), want_w)
        np.testing.assert_array_equal(got_z.cpu().numpy(), want_z)
    with pytest.raises(RuntimeError, match="weights is NULL"):
        N._lib.check(ctx.lib.nerf_render_output_grads(ctx.h, None, None, 1, 1, None, None, None, None, None, 0))
    ctx.close()


def test_forward_outputs_and_interchangeable_slots(big, capsys):
    """The four outputs at 40 x (55 + 55) under the float32 policy: rgb the same bits as nerf_train_render_forward; rgb and
    weights within the forward bar of test_backward_through_render (5e-5) of the float64 oracle, depth within that bar x far,
    z within 1e-6 x far.  Either forward fills a slot that either backward consumes, bit for bit."""
    p, far = big, big["far"]
    r = p["ref"](True)
    ctx = S.golden_context(p, leaky_relu_alpha=1.0)
    ctx.train_begin(5e-4)
    out = R.forward(ctx, p, slot=2)
    rgb_old = ctx.train_render_forward(5, p["o"], p["d"], *R.draws(p))
    np.testing.assert_array_equal(out["rgb"], rgb_old)
    assert out["depth"].shape == (40,) and out["weights"].shape == (40, 110) and out["z"].shape == (40, 110)
    figs = {k: float(np.abs(out[k] - r[k]).max()) for k in ("rgb", "weights", "depth", "z")}
    with capsys.disabled():
        print("\n[render outputs, 40 x (55 + 55), float32] max-abs vs float64: " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()),
              end="")
    assert figs["rgb"] <= 5e-5 and figs["weights"] <= 5e-5
    assert figs["depth"] <= 5e-5 * far
    assert figs["z"] <= 1e-6 * far
    assert (np.diff(out["z"], axis=-1) >= 0).all()
    # a subset of the outputs: the same bits, nothing else returned
    part = R.forward(ctx, p, slot=3, outputs=("depth", "z"))
    assert set(part) == {"depth", "z"}
    np.testing.assert_array_equal(part["depth"], out["depth"])
    np.testing.assert_array_equal(part["z"], out["z"])
    # slots: new forward (2) -> old backward, old forward (5) -> new backward, against old -> old (6)
    d_rgb = p["cot"]["d_rgb"]
    ctx.train_render_forward(6, p["o"], p["d"], *R.draws(p))
    gc0, gf0 = ctx.train_render_backward(6, d_rgb)
    gc1, gf1 = ctx.train_render_backward(2, d_rgb)
    gc2, gf2 = ctx.train_render_backward_outputs(5, d_rgb=d_rgb)
    for g, g0 in ((gc1, gc0), (gf1, gf0), (gc2, gc0), (gf2, gf0)):
        np.testing.assert_array_equal(g, g0)
    # errors: a consumed slot, an empty one, no cotangent at all, NULL structs
    for slot in (5, 77):
        with pytest.raises(RuntimeError, match="holds no forward pass"):
            ctx.train_render_backward_outputs(slot, d_depth=p["cot"]["d_depth"])
    with pytest.raises(RuntimeError, match="all four cotangents"):
        ctx.train_render_backward_outputs(3)
    import nerf_and_dietnerf_amd as N
    with pytest.raises(RuntimeError, match="nerf_render_grads is NULL"):
        N._lib.check(ctx.lib.nerf_train_render_backward_outputs(ctx.h, 3, None, 0, None, None, 0))
    with pytest.raises(RuntimeError, match="nerf_train_outputs is NULL"):
        N._lib.check(ctx.lib.nerf_train_render_forward_outputs(ctx.h, 3, p["o"].ctypes.data, p["d"].ctypes.data, 40, 55, 55,
                                                               None, None, 0, 0, None, 0))
    ctx.close()


@pytest.mark.parametrize("policy", ["float32", "mixed_float16"])
def test_d_rgb_alone_is_the_existing_backward_bit_for_bit(big, policy):
    p, d_rgb = big, big["cot"]["d_rgb"]
    ctx = S.golden_context(p, leaky_relu_alpha=1.0)
    ctx.train_begin(5e-4, mixed_float16=policy == "mixed_float16")
    rgb_old = ctx.train_render_forward(0, p["o"], p["d"], *R.draws(p))
    gc0, gf0 = ctx.train_render_backward(0, d_rgb)
    out = R.forward(ctx, p, slot=0)
    gc1, gf1 = ctx.train_render_backward_outputs(0, d_rgb=d_rgb)
    np.testing.assert_array_equal(out["rgb"], rgb_old)
    GB.check_equal(gc1, gc0, BLOCKS, 0, f"[{policy}] coarse")
    GB.check_equal(gf1, gf0, BLOCKS, 0, f"[{policy}] fine")
    assert gf0.any() and gc0.any()
    ctx.close()


def _report(capsys, label, g, ref64, ref32_fn):
    """The blob-wide figures; where they miss the bar, the block-wise ones as well (GB.check_fp32_smooth prints them; what it
    asserts of its own is printed too, the caller fails the case on the blob-wide bar)."""
    e, c = S.relerr(g, ref64), S.cos(g, ref64)
    with capsys.disabled():
        print(f"\n    {label}: {e:.2e} of max|g|, cosine {c:.8f}", end="")
        if not (e <= 2e-4 and c > 0.9999999):
            try:
                GB.check_fp32_smooth(g, ref64, ref32_fn(), BLOCKS, 2e-4, label)
            except AssertionError as ex:
                print(f"\n    {label}: {ex}", end="")
    return e, c


@pytest.mark.parametrize("sampler_gradient", [True, False])
def test_gradients_against_float64_autograd(big, sampler_gradient, capsys):
    """Each of d_depth, d_weights, d_z alone and all four together at 40 x (55 + 55), alpha = 1, against float64 autograd at
    the bars of test_backward_through_render: 2e-4 of max|g| and cosine > 0.9999999, fine and (through the sampler) coarse.
    d_z alone leaves the fine network exactly zero; without the sampler term the coarse gradient is exactly zero and d_z
    changes no bit."""
    p, cot = big, big["cot"]
    r = p["ref"](sampler_gradient)
    ctx = S.golden_context(p, leaky_relu_alpha=1.0)
    ctx.train_begin(5e-4, sampler_gradient=sampler_gradient)
    with capsys.disabled():
        print(f"\n[render-output gradients, 40 x (55 + 55), sampler term {'on' if sampler_gradient else 'off'}]", end="")
    failed = []
    for name, kw in _sets(cot).items():
        R.forward(ctx, p, outputs=("rgb",))
        gc, gf = ctx.train_render_backward_outputs(0, **kw)
        rc, rf = r["grads"][name]
        r32 = lambda which: (lambda: p["ref"](sampler_gradient, "float32")["grads"][name][which])      # noqa: E731
        if name == "d_z":
            assert not gf.any() and not rf.any()
        else:
            e, c = _report(capsys, f"{name}: fine", gf, rf, r32(1))
            if not (e <= 2e-4 and c > 0.9999999):
                failed.append((name, "fine", e, c))
        if sampler_gradient:
            e, c = _report(capsys, f"{name}: coarse", gc, rc, r32(0))
            if not (e <= 2e-4 and c > 0.9999999):
                failed.append((name, "coarse", e, c))
        else:
            assert not gc.any() and not rc.any()
    assert not failed, failed
    if not sampler_gradient:
        three = {k: cot[k] for k in ("d_rgb", "d_depth", "d_weights")}
        R.forward(ctx, p, outputs=("rgb",))
        gc_a, gf_a = ctx.train_render_backward_outputs(0, **three)
        R.forward(ctx, p, outputs=("rgb",))
        gc_b, gf_b = ctx.train_render_backward_outputs(0, **three, d_z=cot["d_z"])
        np.testing.assert_array_equal(gf_a, gf_b)
        np.testing.assert_array_equal(gc_a, gc_b)
    ctx.close()


def test_ragged_merged_pass_at_the_trained_slope(oracle, golden_ckpt, capsys):
    """7 rays x (33 + 32): the merged S = 65 crosses the 64-sample chunk and N is no multiple of the 4 rays per block; the
    trained slope alpha = 0.05 and the combined cotangent, at the project's alpha = 0.05 blob bars (relative error <= 1e-2 of
    max|g|, cosine > 0.9999; float32 autograd itself is at 3.5e-5 / 6.9e-5 (fine / coarse) of max|g| on these inputs, with
    gradients of order 0.1 .. 1)."""
    p = S.golden_problem(oracle, golden_ckpt, n=7, sc=33, sf=32, seed=21)
    cot = R.cotangents(7, 65, seed=5)
    r = R.render_outputs_gradients(p["bc"], p["bf"], p["o"], p["d"], p["near"], p["far"], p["u_c"], p["u_f"], **cot)
    ctx = S.golden_context(p)
    ctx.train_begin(5e-4)
    out = R.forward(ctx, p)
    gc, gf = ctx.train_render_backward_outputs(0, **cot)
    assert np.abs(out["depth"] - r["depth"]).max() <= 5e-5 * p["far"]
    ef, cf, ec, cc = S.relerr(gf, r["grad_fine"]), S.cos(gf, r["grad_fine"]), S.relerr(gc, r["grad_coarse"]), S.cos(gc, r["grad_coarse"])
    with capsys.disabled():
        print(f"\n[render-output gradients, 7 x (33 + 32), alpha 0.05, all four] fine {ef:.2e} cosine {cf:.7f}; "
              f"coarse {ec:.2e} cosine {cc:.7f}; max|g| fine {np.abs(r['grad_fine']).max():.2e} coarse "
              f"{np.abs(r['grad_coarse']).max():.2e}", end="")
    assert ef <= 1e-2 and cf > 0.9999
    assert ec <= 1e-2 and cc > 0.9999
    ctx.close()


def test_coarse_only_context_ignores_d_z(oracle, golden_ckpt, capsys):
    """A context without a fine network, 5 rays x 3 samples: d_depth + d_weights against the oracle at the same alpha = 0.05
    bars (the same network and policy as the ragged case); the depths of a coarse pass are data, so d_z changes no bit."""
    p = S.golden_problem(oracle, golden_ckpt, n=5, sc=3, sf=0, seed=2)
    cot = R.cotangents(5, 3, seed=8)
    two = {k: cot[k] for k in ("d_depth", "d_weights")}
    r = R.render_outputs_gradients(p["bc"], None, p["o"], p["d"], p["near"], p["far"], p["u_c"], None, **two)
    ctx = S.golden_context(p, fine=False)
    ctx.train_begin(5e-4)
    out = ctx.train_render_forward_outputs(0, p["o"], p["d"], 3, 0, p["u_c"])
    assert out["weights"].shape == (5, 3) and out["z"].shape == (5, 3)
    assert np.abs(out["weights"] - r["weights"]).max() <= 5e-5 and np.abs(out["depth"] - r["depth"]).max() <= 5e-5 * p["far"]
    gc, gf = ctx.train_render_backward_outputs(0, **two)
    assert gf is None
    e, c = S.relerr(gc, r["grad_coarse"]), S.cos(gc, r["grad_coarse"])
    with capsys.disabled():
        print(f"\n[render-output gradients, coarse only, 5 x 3, d_depth + d_weights] {e:.2e} of max|g|, cosine {c:.7f}", end="")
    assert e <= 1e-2 and c > 0.9999
    ctx.train_render_forward_outputs(0, p["o"], p["d"], 3, 0, p["u_c"])
    gc_z, _ = ctx.train_render_backward_outputs(0, **two, d_z=cot["d_z"])
    np.testing.assert_array_equal(gc_z, gc)
    ctx.close()


def test_mixed_float16_policy(big, capsys):
    """The combined cotangent at 40 x (55 + 55) under mixed_float16 against the oracle that rounds where the kernels round,
    as test_backward_through_render_mixed_policy checks d_rgb (forward 2e-3; fine 5e-3 of max|g|, cosine > 0.9999; coarse 3e-2,
    cosine > 0.999; GB.check_mixed block by block).  The cotangents go in unscaled.  Of that test's two loss scales this one
    runs 2048: 0.1 N(0, 1) on every weight makes pre-activation gradients of order 1..10, which times 32768 leave the fp16
    range -- the emulating oracle itself returns non-finite fine gradients there (306 entries for d_weights alone), a step
    the dynamic loss scale exists to skip.  Then an inf in d_depth: the step is skipped and the loss scale halves."""
    p, cot, scale = big, big["cot"], 2048.0
    ctx = S.golden_context(p, leaky_relu_alpha=1.0)
    ctx.train_begin(5e-4, mixed_float16=True, initial_loss_scale=scale)
    out = R.forward(ctx, p)
    gc, gf = ctx.train_render_backward_outputs(0, **cot)
    r16 = p["ref"](True, "float64", scale)
    e32 = p["ref"](True, "float32", scale)
    rc, rf = r16["grads"]["all"]
    assert np.abs(out["rgb"] - r16["rgb"]).max() <= 2e-3
    assert np.isfinite(gc).all() and np.isfinite(gf).all()
    qf, cf, qc, cc = S.relerr(gf, rf), S.cos(gf, rf), S.relerr(gc, rc), S.cos(gc, rc)
    with capsys.disabled():
        print(f"\n[render-output gradients, mixed_float16, loss scale {scale:g}, all four] fine vs the fp16-emulating oracle "
              f"{qf:.2e} of max|g|, cosine {cf:.6f}; coarse {qc:.2e}, cosine {cc:.6f}", end="")
        assert qf <= 5e-3 and cf > 0.9999
        GB.check_mixed(gf, rf, e32["grads"]["all"][1], BLOCKS, "[render outputs, mixed] fine")
        assert qc <= 3e-2 and cc > 0.999
        GB.check_mixed(gc, rc, e32["grads"]["all"][0], BLOCKS, "[render outputs, mixed] coarse")
    ctx.train_apply()
    assert ctx.train_loss_scale() == (scale, 1, 0)
    w0, w1 = ctx.get_weights(0), ctx.get_weights(1)
    bad = cot["d_depth"].copy()
    bad[3] = np.inf
    R.forward(ctx, p, outputs=("rgb",))
    ctx.train_render_backward_outputs(0, d_rgb=cot["d_rgb"], d_depth=bad, want_blobs=False)
    ctx.train_apply()
    assert ctx.train_loss_scale() == (scale / 2, 1, 1)
    np.testing.assert_array_equal(ctx.get_weights(0), w0)
    np.testing.assert_array_equal(ctx.get_weights(1), w1)
    ctx.close()


def test_accumulate_adds_to_the_ray_loss_gradients(big):
    """accumulate = 1 after nerf_train_gradients: the sum of the two gradients, to 1e-6 of max|g| (the existing test's bar)."""
    p, cot = big, big["cot"]
    ctx = S.golden_context(p, leaky_relu_alpha=1.0)
    ctx.train_begin(5e-4)
    R.forward(ctx, p, outputs=("rgb",))
    gc, gf = ctx.train_render_backward_outputs(0, **cot)
    _, gc1, gf1 = ctx.train_gradients(p["o"], p["d"], p["tgt"], *R.draws(p))
    R.forward(ctx, p, outputs=("rgb",))
    gc2, gf2 = ctx.train_render_backward_outputs(0, **cot, accumulate=True)
    assert np.abs(gf2 - (gf1 + gf)).max() <= 1e-6 * np.abs(gf2).max()
    assert np.abs(gc2 - (gc1 + gc)).max() <= 1e-6 * max(np.abs(gc2).max(), 1e-30)
    ctx.train_apply()
    ctx.close()


def test_train_sample_culling_under_a_full_grid_changes_no_bit(oracle, golden_ckpt):
    """nerf_ctx_set_train_sample_culling with a grid that keeps every cell: outputs and gradients of the new calls are the
    bits of the flag being off (compositing, its backward and the fold run on all samples either way)."""
    import nerf_and_dietnerf_amd as N
    p = S.golden_problem(oracle, golden_ckpt, n=13, sc=20, sf=17, seed=4)
    cot = R.cotangents(13, 37, seed=6)
    got = []
    for flag in (False, True):
        ctx = N.Context(near=p["near"], far=p["far"], precision="fp32")
        ctx.load_weights(0, p["bc"])
        ctx.load_weights(1, p["bf"])
        ctx.set_scene_box(*O.GOLDEN_BOX)
        ctx.set_occupancy_grid(np.ones((16, 16, 16), bool))
        ctx.set_train_sample_culling(flag)
        ctx.train_begin(5e-4)
        out = R.forward(ctx, p)
        gc, gf = ctx.train_render_backward_outputs(0, **cot)
        got.append((out, gc, gf))
        ctx.close()
    (o0, gc0, gf0), (o1, gc1, gf1) = got
    for k in ("rgb", "depth", "weights", "z"):
        np.testing.assert_array_equal(o1[k], o0[k])
    np.testing.assert_array_equal(gc1, gc0)
    np.testing.assert_array_equal(gf1, gf0)
    assert gf0.any() and gc0.any()


def test_bridge_mse_equals_the_d_rgb_backward(big):
    """loss = ((rgb - t)^2).mean() through render_with_grad leaves the gradients of nerf_train_render_backward with
    d_rgb = 2 (rgb - t) / (3 N), bit for bit (d_rgb as torch forms it from the same rgb: (rgb - t) * 2 * fl(1 / 3N))."""
    import torch
    import nerf_and_dietnerf_amd as N
    p = big
    ctx = S.golden_context(p, leaky_relu_alpha=1.0)
    ctx.train_begin(5e-4)
    dev = lambda a: torch.as_tensor(a, device="cuda")                                              # noqa: E731
    o, d, t, uc, uf = (dev(p[k]) for k in ("o", "d", "tgt", "u_c", "u_f"))
    out = N.render_with_grad(ctx, o, d, p["sc"], p["sf"], slot=4, u_coarse=uc, u_fine=uf)
    assert all(v.is_cuda and v.requires_grad for v in out.values())
    loss = ((out["rgb"] - t) ** 2).mean()
    loss.backward()
    gc, gf = ctx.train_get_gradients(0), ctx.train_get_gradients(1)
    leaf = out["rgb"].detach().clone().requires_grad_(True)
    ((leaf - t) ** 2).mean().backward()
    d_rgb = leaf.grad.cpu().numpy()
    formula = 2.0 * (out["rgb"].detach().cpu().numpy().astype(np.float64) - p["tgt"]) / (3 * p["n"])
    np.testing.assert_allclose(d_rgb, formula, rtol=1e-6, atol=1e-12)
    rgb = ctx.train_render_forward(0, p["o"], p["d"], *R.draws(p))
    np.testing.assert_array_equal(rgb, out["rgb"].detach().cpu().numpy())
    gc0, gf0 = ctx.train_render_backward(0, d_rgb)
    np.testing.assert_array_equal(gc, gc0)
    np.testing.assert_array_equal(gf, gf0)
    # the backward consumes the slot: a second one through the same graph surfaces the library's message
    again = N.render_with_grad(ctx, o, d, p["sc"], p["sf"], slot=4, u_coarse=uc, u_fine=uf)["depth"].sum()
    again.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="holds no forward pass"):
        again.backward()
    ctx.close()


def test_train_step_custom_reduces_a_depth_loss(oracle, golden_ckpt, capsys):
    """Twenty NeRF.train_step_custom steps on one 48-ray x (16 + 24) batch with loss = ((depth - depth_target)^2).mean(),
    depth_target = the initial depth + 0.1: the loss ends below its start.  Learning rate 2e-5: Adam's first steps move every
    weight by about the learning rate whatever the gradient's size, and the trained network's half a million weights moving
    together by 5e-4 (the rate of the other tests here) shift the depth by far more than the 0.1 asked for -- float64
    autograd + Adam on the CPU goes 1.0e-2 -> 5.7e-1 at the second step there, and 1.0e-2 -> 8e-4 in twenty steps at 2e-5."""
    import torch
    import nerf_and_dietnerf_amd as N
    net_cfg = {"hidden_layer_dim": 256, "last_hidden_layer_dim": 128, "leaky_relu_alpha": 0.05,
               "n_pos_enc_dim_xyz": 5, "n_pos_enc_view_dir": 4, "n_angles_for_model": 2,
               "n_rays_in_batch_train": 4096, "n_rays_in_batch_render": 4096}
    m = N.NeRF(net_cfg, {"n_render_samples_coarse": 16, "n_render_samples_fine": 24}, float(golden_ckpt["near"]),
               float(golden_ckpt["far"]))
    m.set_weights(golden_ckpt["blob_coarse"], golden_ckpt["blob_fine"])
    m.compile(2e-5)
    o, d, rng = S.oracle_rays(oracle, 48, 0)
    dev = lambda a: torch.as_tensor(a, device="cuda")                                              # noqa: E731
    o, d, tgt = dev(o), dev(d), dev(rng.random((48, 3), dtype=np.float32))
    u_c, u_f = dev(rng.random((48, 16), dtype=np.float32)), dev(rng.random((48, 24), dtype=np.float32))
    first = N.render_with_grad(m.ctx, o, d, 16, 24, u_coarse=u_c, u_fine=u_f)["depth"].detach()
    target = first + 0.1
    loss_fn = lambda out, real_rgb: ((out["depth"] - target) ** 2).mean()                         # noqa: E731
    losses = [m.train_step_custom((o, d, tgt), loss_fn, u_coarse=u_c, u_fine=u_f, want_loss=True) for _ in range(20)]
    assert m.train_step_custom((o, d, tgt), loss_fn, u_coarse=u_c, u_fine=u_f) is None
    with capsys.disabled():
        print(f"\n[train_step_custom, depth loss, 48 x (16 + 24)] loss {losses[0]:.6e} -> {losses[-1]:.6e} after 20 steps", end="")
    assert abs(losses[0] - 0.01) <= 1e-4 and np.isfinite(losses).all()
    assert losses[-1] < losses[0]
    m.ctx.close()
