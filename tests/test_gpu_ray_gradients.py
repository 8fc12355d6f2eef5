"""Ray gradients on the device (include/nerf_mi355.h: nerf_train_set_ray_gradients, nerf_train_render_backward_rays,
nerf_ray_position_grads), the torch bridge over them and pose recovery through rays_from_pose.

The reference of every gradient is float64 autograd of NeRF.render()'s graph with the rays as leaves (tests/ray_grad_ref.py),
on the problems, draws and cotangents of tests/test_gpu_render_outputs.py.  Bars: at 40 x (55 + 55), alpha = 1, 2e-4 of each
tensor's max|g| and cosine > 0.9999999 (float32 autograd itself sits at 3.9e-5 there); at the trained slope alpha = 0.05, 1e-2
and cosine > 0.9999; under mixed_float16 against the fp16-emulating oracle, 3e-2 and cosine > 0.999.
tests/test_ray_gradients_host.py shows on the CPU that none of these can pass with the view-direction term or the sampler
term missing.
"""
import numpy as np
import pytest

import culling_ref as K
import grad_blocks as GB
import occupancy_ref as O
import ray_grad_ref as G
import render_outputs_ref as R
import support as S

pytestmark = pytest.mark.gpu

BLOCKS = GB.blocks(5, 4, 2)


def _sets(cot):
    return {**{k: {k: cot[k]} for k in R.NAMES}, "all": dict(cot)}


def _args(p, fine=True):
    return (p["bc"], p["bf"] if fine else None, p["o"], p["d"], p["near"], p["far"], p["u_c"], p["u_f"] if fine else None)


def _begin(p, ray_gradients=True, fine=True, ctx_kw=None, **train_kw):
    ctx = S.golden_context(p, fine=fine, **(ctx_kw or {}))
    ctx.train_begin(5e-4, **train_kw)
    if ray_gradients:
        ctx.train_set_ray_gradients(True)
    return ctx


def _rays_backward(ctx, p, slot=0, **cot):
    R.forward(ctx, p, slot=slot, outputs=("rgb",))
    return ctx.train_render_backward_outputs(slot, **cot, want_rays=True)


def _figures(capsys, label, got, ref):
    """(relative error, cosine) of d_rays_orig and of d_rays_dirs, printed; component 3 is exactly zero."""
    out = []
    for name, g, r in zip(("d_rays_orig", "d_rays_dirs"), got, ref):
        assert g.shape == r.shape and g.dtype == np.float32
        assert not g[:, 3].any(), f"{label}: {name}[:, 3] is not zero"
        out.append((S.relerr(g, r), S.cos(g.ravel(), r.ravel().astype(np.float64))))
    with capsys.disabled():
        print(f"\n    {label}: d_rays_orig {out[0][0]:.2e} of max|g|, cosine {out[0][1]:.8f}; d_rays_dirs {out[1][0]:.2e}, "
              f"cosine {out[1][1]:.8f}", end="")
    return out


@pytest.fixture(scope="module")
def big(oracle, golden_ckpt):
    """The 40 x (55 + 55) problem of tests/test_gpu_render_outputs.py with its cotangents and, computed once per (sampler
    term, dtype, loss scale) and shared, the oracle's ray and weight gradients for the five cotangent sets."""
    p = S.golden_problem(oracle, golden_ckpt, n=40, sc=55, sf=55, seed=9)
    p["cot"] = R.cotangents(40, 110)
    cache = {}

    def ref(sampler_grad, fp16_loss_scale=None, weights=False):
        key = (sampler_grad, fp16_loss_scale, weights)
        if key not in cache:
            fn = R.render_outputs_gradient_sets if weights else G.ray_gradient_sets
            cache[key] = fn(*_args(p), _sets(p["cot"]), sampler_grad=sampler_grad, alpha=1.0, fp16_loss_scale=fp16_loss_scale)["grads"]
        return cache[key]

    p["ref"] = ref
    return p


def test_bare_operator(golden_ckpt):
    """nerf_ray_position_grads on (13, 65, 3): ragged across the 64 lanes of the wave that owns a ray and across the four
    rays of a workgroup.  Within 1e-6 of sum|terms| per component of the float64 restatement; the same bits on a second run
    and from device tensors; component 3 exactly zero."""
    import torch
    import nerf_and_dietnerf_amd as N
    ctx = N.Context(near=float(golden_ckpt["near"]), far=float(golden_ckpt["far"]))
    rng = np.random.default_rng(0)
    dp = rng.standard_normal((13, 65, 3)).astype(np.float32)
    z = np.sort(rng.random((13, 65), dtype=np.float32) * 4 + 2, axis=-1)
    w_o, w_d, a_o, a_d = G.position_reduce(dp, z)
    g_o, g_d = ctx.ray_position_grads(dp, z)
    assert g_o.shape == (13, 4) and g_d.shape == (13, 4) and g_o.dtype == np.float32
    assert not g_o[:, 3].any() and not g_d[:, 3].any()
    assert (np.abs(g_o - w_o) <= 1e-6 * a_o).all(), float((np.abs(g_o - w_o)[:, :3] / a_o[:, :3]).max())
    assert (np.abs(g_d - w_d) <= 1e-6 * a_d).all(), float((np.abs(g_d - w_d)[:, :3] / a_d[:, :3]).max())
    h_o, h_d = ctx.ray_position_grads(dp, z)
    np.testing.assert_array_equal(h_o, g_o)
    np.testing.assert_array_equal(h_d, g_d)
    t_o, t_d = ctx.ray_position_grads(torch.as_tensor(dp, device="cuda"), torch.as_tensor(z, device="cuda"))
    np.testing.assert_array_equal(t_o.cpu().numpy(), g_o)
    np.testing.assert_array_equal(t_d.cpu().numpy(), g_d)
    with pytest.raises(RuntimeError, match="d_points is NULL"):
        N._lib.check(ctx.lib.nerf_ray_position_grads(ctx.h, None, None, 1, 1, None, None, 0))
    ctx.close()


@pytest.mark.parametrize("name", R.NAMES + ("all",))
@pytest.mark.parametrize("sampler_gradient", [True, False])
def test_against_float64_autograd(big, sampler_gradient, name, capsys):
    """40 x (55 + 55), alpha = 1, the shipped checkpoint: both ray gradients within 2e-4 of the tensor's max|g| of float64
    autograd with cosine > 0.9999999, component 3 exactly zero; d_z without the sampler term gives exact zeros; the weight
    gradients of the same call keep their bars (tests/test_gpu_render_outputs.py)."""
    p, kw = big, _sets(big["cot"])[name]
    ref = p["ref"](sampler_gradient)[name]
    rc, rf = p["ref"](sampler_gradient, weights=True)[name]
    ctx = _begin(p, ctx_kw=dict(leaky_relu_alpha=1.0), sampler_gradient=sampler_gradient)
    assert ctx.train_ray_gradients
    gc, gf, g_o, g_d = _rays_backward(ctx, p, **kw)
    ctx.close()
    if name == "d_z" and not sampler_gradient:
        assert not g_o.any() and not g_d.any() and not ref[0].any() and not ref[1].any()
        assert not gc.any() and not gf.any()
        return
    figs = _figures(capsys, f"[ray gradients, 40 x (55 + 55), sampler term {'on' if sampler_gradient else 'off'}] {name}",
                    (g_o, g_d), ref)
    for e, c in figs:
        assert e <= 2e-4 and c > 0.9999999
    blobs = [(gf, rf, "fine")] if name != "d_z" else []
    if name == "d_z":
        assert not gf.any() and not rf.any()
    if sampler_gradient:
        blobs.append((gc, rc, "coarse"))
    else:
        assert not gc.any() and not rc.any()
    for g, r, which in blobs:
        e, c = S.relerr(g, r), S.cos(g, r)
        assert e <= 2e-4 and c > 0.9999999, (which, e, c)


def test_ragged_pass_at_the_trained_slope(oracle, golden_ckpt, capsys):
    """7 rays x (33 + 32): the merged S = 65 crosses the 64 lanes and the 32-sample rounds, N is no multiple of the four rays
    per workgroup; alpha = 0.05 and all four cotangents at the alpha = 0.05 bars (1e-2 of max|g|, cosine > 0.9999)."""
    p = S.golden_problem(oracle, golden_ckpt, n=7, sc=33, sf=32, seed=21)
    cot = R.cotangents(7, 65, seed=5)
    ref = G.ray_gradients(*_args(p), **cot)
    ctx = _begin(p)
    _, _, g_o, g_d = _rays_backward(ctx, p, **cot)
    ctx.close()
    for e, c in _figures(capsys, "[ray gradients, 7 x (33 + 32), alpha 0.05, all four]", (g_o, g_d), ref):
        assert e <= 1e-2 and c > 0.9999


def test_coarse_only_context(oracle, golden_ckpt, capsys):
    """A context without a fine network, 5 rays x 3 samples: the coarse pass is the last pass; d_z changes no bit."""
    p = S.golden_problem(oracle, golden_ckpt, n=5, sc=3, sf=0, seed=2)
    cot = R.cotangents(5, 3, seed=8)
    three = {k: cot[k] for k in ("d_rgb", "d_depth", "d_weights")}
    ref = G.ray_gradients(*_args(p, fine=False), **three)
    ctx = _begin(p, fine=False)
    fwd = lambda: ctx.train_render_forward_outputs(0, p["o"], p["d"], 3, 0, p["u_c"], outputs=("rgb",))      # noqa: E731
    fwd()
    gc, gf, g_o, g_d = ctx.train_render_backward_outputs(0, **three, want_rays=True)
    assert gf is None and gc.any()
    for e, c in _figures(capsys, "[ray gradients, coarse only, 5 x 3, alpha 0.05]", (g_o, g_d), ref):
        assert e <= 1e-2 and c > 0.9999
    fwd()
    _, _, z_o, z_d = ctx.train_render_backward_outputs(0, **three, d_z=cot["d_z"], want_rays=True)
    np.testing.assert_array_equal(z_o, g_o)
    np.testing.assert_array_equal(z_d, g_d)
    ctx.close()


@pytest.mark.parametrize("lx,ld,na", [(5, 4, 1), (5, 4, 0), (10, 2, 2)])
def test_network_variants(oracle, golden_ckpt, lx, ld, na, capsys):
    """6 x (8 + 8) on Glorot weights: n_angles = 1 reads direction components 0 and 2 (component 1 carries the position term
    alone), n_angles = 0 has no view-direction input, (10, 2) runs the wide-PE layout.  The alpha = 0.05 bars.  (At (10, 2)
    float32 autograd itself sits at 9.2e-3 / 9.4e-3 of max|g| on the CPU -- the top octave multiplies a position's float32
    rounding by 2^9 pi, and the sampler's 1e5 gain acts on it -- and the device at 8.9e-3 / 9.4e-3; the view-direction term is
    2e-2 of max|d_rays_dirs| there and the sampler term about 100 %, so the 1e-2 bar still tells either from missing.)"""
    import nerf_and_dietnerf_amd as N
    kw = dict(n_pos_enc_xyz=lx, n_pos_enc_dir=ld, n_angles=na)
    p = S.golden_problem(oracle, golden_ckpt, n=6, sc=8, sf=8, seed=13)
    p["bc"], p["bf"] = N.glorot_blob(3, **kw), N.glorot_blob(4, **kw)
    p["bc"][-1] = p["bf"][-1] = 1.5              # lift sigma: Glorot networks are almost transparent
    cot = R.cotangents(6, 16, seed=7)
    ref = G.ray_gradients(*_args(p), **cot, **kw)
    ctx = _begin(p, ctx_kw=dict(precision="fp32" if lx <= 5 else "f16x3", **kw))
    _, _, g_o, g_d = _rays_backward(ctx, p, **cot)
    ctx.close()
    for e, c in _figures(capsys, f"[ray gradients, 6 x (8 + 8), Lx {lx} Ld {ld} n_angles {na}]", (g_o, g_d), ref):
        assert e <= 1e-2 and c > 0.9999
    if na != 2:
        # without the view-direction term in component 1 (n_angles 1) / anywhere (n_angles 0) the oracle says the same
        no_view = G.ray_gradients(*_args(p), **cot, view_term=False, **kw)
        cols = [1] if na == 1 else [0, 1, 2]
        np.testing.assert_array_equal(no_view[1][:, cols], ref[1][:, cols])
        assert np.abs(g_d[:, cols] - ref[1][:, cols]).max() <= 1e-2 * np.abs(ref[1]).max()


def test_mixed_float16_policy(big, capsys):
    """All four cotangents at 40 x (55 + 55), alpha = 1, loss scale 2048, against the oracle that rounds where the kernels
    round: finite, within 3e-2 of max|g|, cosine > 0.999 -- the bars of gradients that cross the sampler under this policy.
    (The emulating oracle itself differs from float64 by 4.2e-2 with cosine 0.99997 here.)  The ray gradients come back
    unscaled; the loss scale and the step verdict are untouched by them."""
    p, scale = big, 2048.0
    ref = p["ref"](True, scale)["all"]
    ctx = _begin(p, ctx_kw=dict(leaky_relu_alpha=1.0), mixed_float16=True, initial_loss_scale=scale)
    gc, gf, g_o, g_d = _rays_backward(ctx, p, **p["cot"])
    assert np.isfinite(g_o).all() and np.isfinite(g_d).all() and np.isfinite(gc).all() and np.isfinite(gf).all()
    for e, c in _figures(capsys, f"[ray gradients, mixed_float16, loss scale {scale:g}, all four] vs the fp16-emulating oracle",
                         (g_o, g_d), ref):
        assert e <= 3e-2 and c > 0.999
    ctx.train_apply()
    assert ctx.train_loss_scale() == (scale, 1, 0)
    ctx.close()


def test_switch_semantics(big):
    p, cot = big, big["cot"]
    d_rgb = cot["d_rgb"]
    ctx = _begin(p, ray_gradients=False, ctx_kw=dict(leaky_relu_alpha=1.0))
    assert ctx.train_ray_gradients is False

    def both():
        R.forward(ctx, p, outputs=("rgb",))
        a = ctx.train_render_backward_outputs(0, **cot)
        ctx.train_render_forward(0, p["o"], p["d"], *R.draws(p))
        return a + ctx.train_render_backward(0, d_rgb)

    off = both()
    # off: asking for the rays raises, and the slot survives the refusal
    R.forward(ctx, p, outputs=("rgb",))
    with pytest.raises(RuntimeError, match="nerf_train_set_ray_gradients"):
        ctx.train_render_backward_outputs(0, **cot, want_rays=True)
    ctx.train_render_backward_outputs(0, **cot, want_blobs=False)
    # on: the fine network runs the variant it already ran (bit-equal), the coarse one its encoding-gradient variant
    ctx.train_set_ray_gradients(True)
    assert ctx.train_ray_gradients is True
    on = both()
    np.testing.assert_array_equal(on[1], off[1])
    np.testing.assert_array_equal(on[3], off[3])
    rc, _ = R.render_outputs_gradient_sets(*_args(p), {"all": dict(cot)}, alpha=1.0)["grads"]["all"]
    assert S.relerr(on[0], rc) <= 2e-4 and S.cos(on[0], rc) > 0.9999999
    # both ray outputs NULL: nerf_train_render_backward_outputs, bit for bit
    import ctypes as C
    import nerf_and_dietnerf_amd as N
    R.forward(ctx, p, outputs=("rgb",))
    keep = [np.ascontiguousarray(cot[k]) for k in R.NAMES]
    g = N._lib.NerfRenderGrads(*[a.ctypes.data for a in keep])
    gc, gf = np.empty(ctx.blob_size(), np.float32), np.empty(ctx.blob_size(), np.float32)
    N._lib.check(ctx.lib.nerf_train_render_backward_rays(ctx.h, 0, C.byref(g), 0, gc.ctypes.data, gf.ctypes.data, None, None, 0))
    np.testing.assert_array_equal(gc, on[0])
    np.testing.assert_array_equal(gf, on[1])
    # back off: every bit of the first off run
    ctx.train_set_ray_gradients(False)
    again = both()
    for a, b in zip(again, off):
        np.testing.assert_array_equal(a, b)
    # train_begin resets the switch
    ctx.train_set_ray_gradients(True)
    ctx.train_begin(5e-4)
    assert ctx.train_ray_gradients is False
    R.forward(ctx, p, outputs=("rgb",))
    with pytest.raises(RuntimeError, match="nerf_train_set_ray_gradients"):
        ctx.train_render_backward_outputs(0, **cot, want_rays=True)
    fresh = both()
    for a, b in zip(fresh, off):
        np.testing.assert_array_equal(a, b)
    ctx.close()


def test_train_sample_culling(oracle, golden_ckpt):
    """Sixteen rays of the golden training camera, the last ten turned round so that they miss the box.  Under
    nerf_ctx_set_train_sample_culling with a full grid the ray gradients are the bits of the flag being off; with one half of
    the grid emptied the rays that miss the box keep their bits, the others change, and every ray's result is finite."""
    p = K.train_scene(oracle, golden_ckpt, 16, 20, 17, 4)
    cot = R.cotangents(16, 37, seed=6)
    full, half = np.ones((16, 16, 16), bool), np.ones((16, 16, 16), bool)
    half[:8] = False
    got = {}
    for key, flag, grid in (("off", False, full), ("full", True, full), ("half", True, half)):
        ctx = K.culled_context(p, grid, flag)
        ctx.train_begin(5e-4)
        ctx.train_set_ray_gradients(True)
        z = R.forward(ctx, p)["z"]
        got[key] = ctx.train_render_backward_outputs(0, **cot, want_rays=True)[2:]
        if key == "off":
            inside, _ = K.sample_cells(p["o"], p["d"], z, *O.GOLDEN_BOX, 16, K.F32)
            outside = ~inside.any(-1)
        ctx.close()
    assert outside[6:].all() and not outside[:6].any()
    for a, b in zip(got["full"], got["off"]):
        np.testing.assert_array_equal(a, b)
    assert got["off"][0].any() and got["off"][1].any()
    for a, b in zip(got["half"], got["off"]):
        assert np.isfinite(a).all() and not a[:, 3].any()
        np.testing.assert_array_equal(a[outside], b[outside])
    assert any((a[~outside] != b[~outside]).any() for a, b in zip(got["half"], got["off"]))


def test_bridge(big):
    """render_with_grad with rays_dirs.requires_grad_() and an MSE loss: rays_dirs.grad is the direct call's d_rays_dirs, bit
    for bit; rays without requires_grad get None; with the switch off the library's error surfaces."""
    import torch
    import nerf_and_dietnerf_amd as N
    p = big
    ctx = _begin(p, ctx_kw=dict(leaky_relu_alpha=1.0))
    dev = lambda a: torch.as_tensor(a, device="cuda")                                              # noqa: E731
    o, d, t, uc, uf = (dev(p[k]) for k in ("o", "d", "tgt", "u_c", "u_f"))
    d.requires_grad_()
    out = N.render_with_grad(ctx, o, d, p["sc"], p["sf"], slot=4, u_coarse=uc, u_fine=uf)
    ((out["rgb"] - t) ** 2).mean().backward()
    assert o.grad is None and d.grad is not None and d.grad.shape == (40, 4)
    leaf = out["rgb"].detach().clone().requires_grad_(True)
    ((leaf - t) ** 2).mean().backward()
    _, _, g_o, g_d = _rays_backward(ctx, p, d_rgb=leaf.grad.cpu().numpy())
    np.testing.assert_array_equal(d.grad.cpu().numpy(), g_d)
    # both leaves
    o2, d2 = dev(p["o"]).requires_grad_(), dev(p["d"]).requires_grad_()
    out = N.render_with_grad(ctx, o2, d2, p["sc"], p["sf"], slot=4, u_coarse=uc, u_fine=uf)
    ((out["rgb"] - t) ** 2).mean().backward()
    np.testing.assert_array_equal(o2.grad.cpu().numpy(), g_o)
    np.testing.assert_array_equal(d2.grad.cpu().numpy(), g_d)
    ctx.train_set_ray_gradients(False)
    d3 = dev(p["d"]).requires_grad_()
    loss = N.render_with_grad(ctx, o, d3, p["sc"], p["sf"], slot=4, u_coarse=uc, u_fine=uf)["rgb"].sum()
    with pytest.raises(RuntimeError, match="nerf_train_set_ray_gradients"):
        loss.backward()
    ctx.close()


def test_pose_recovery(oracle, golden_ckpt, capsys):
    """48 rays x (16 + 24), fixed explicit draws, weights frozen (no train_apply): targets rendered from the golden test pose,
    the translation offset by 0.02 along each axis, twenty torch-Adam steps on the translation alone through rays_from_pose +
    render_with_grad.  The photometric loss and the translation error both end below their starting values.  Learning rate
    1e-3, chosen once from the first gradient's magnitude (about 3 per coordinate on the float64 oracle): at that size plain
    gradient descent would need a rate near 1e-2 / 3 and would be at the mercy of the gradient's scale, while Adam moves each
    coordinate by about the rate per step whatever the gradient's size -- twenty steps of 1e-3 cover the 0.02 offset once and
    cannot overshoot it.  (float64 autograd + Adam on the CPU: loss 3.06e-2 -> 1.68e-2, error 3.46e-2 -> 1.83e-2.)"""
    import torch
    import nerf_and_dietnerf_amd as N
    rng = np.random.default_rng(0)
    hw, n, sc, sf = 16, 48, 16, 24
    p = dict(near=float(golden_ckpt["near"]), far=float(golden_ckpt["far"]), bc=golden_ckpt["blob_coarse"],
             bf=golden_ckpt["blob_fine"])
    ctx = _begin(p)
    fov = float(golden_ckpt["fov"])
    c2w = torch.as_tensor(golden_ckpt["c2w_test"].astype(np.float32), device="cuda")
    idx = torch.as_tensor(rng.choice(hw * hw, n, replace=False), device="cuda")
    u_c = torch.as_tensor(rng.random((n, sc), dtype=np.float32), device="cuda")
    u_f = torch.as_tensor(rng.random((n, sf), dtype=np.float32), device="cuda")
    render = lambda o, d: N.render_with_grad(ctx, o, d, sc, sf, u_coarse=u_c, u_fine=u_f)["rgb"]     # noqa: E731
    with torch.no_grad():
        target = render(*N.rays_from_pose(c2w, fov, hw, hw, idx)).clone()
    offset = torch.full((3,), 0.02, device="cuda")
    trans = torch.nn.Parameter(c2w[:3, 3] + offset)
    opt = torch.optim.Adam([trans], lr=1e-3)
    losses, errors = [], []
    for _ in range(21):
        pose = torch.cat([c2w[:, :3], torch.cat([trans, c2w[3:, 3]])[:, None]], 1)
        loss = ((render(*N.rays_from_pose(pose, fov, hw, hw, idx)) - target) ** 2).mean()
        losses.append(float(loss.detach()))
        errors.append(float((trans.detach() - c2w[:3, 3]).norm()))
        if len(losses) == 21:
            break
        opt.zero_grad()
        loss.backward()
        if len(losses) == 1:
            first = trans.grad.detach().cpu().numpy().copy()
        opt.step()
    w0 = ctx.get_weights(1)
    with capsys.disabled():
        print(f"\n[pose recovery, 48 x (16 + 24), 20 Adam steps, lr 1e-3] first gradient {first}; loss {losses[0]:.4e} -> "
              f"{losses[-1]:.4e}; translation error {errors[0]:.4e} -> {errors[-1]:.4e}", end="")
    assert np.isfinite(losses).all() and np.isfinite(first).all() and first.any()
    assert losses[-1] < losses[0]
    assert errors[-1] < errors[0]
    np.testing.assert_array_equal(w0, golden_ckpt["blob_fine"])
    ctx.close()
