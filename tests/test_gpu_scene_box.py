"""The scene box on the device: the ray / box interval (nerf_ray_box_bounds), the coarse depths of narrowed rays
(nerf_get_z_values_rays) and every layer that draws depths for rays -- render, render_image (world and NDC) and its sharded
form, the trainer under both policies and the kept-activation slots.  The rule and its float32 restatement live in
tests/scene_box_ref.py; the CPU oracle is used unchanged, through the entries it has for given rays and depths.  Every test
here needs the three entry points this adds to the ABI."""
import numpy as np
import pytest

from occupancy_ref import NDC_BOX, NDC_NEAR
import sampling_space_ref as R
import scene_box_ref as B
import support as S

pytestmark = pytest.mark.gpu

LINDISP_MESSAGE = "lindisp needs near_boundary > 0"
BOX_MESSAGE = "scene box needs finite lo < hi on every axis"
NEAR, FAR = B.NEAR, B.FAR
SAMPLES = (1, 2, 5, 64)
FAR_AWAY = ((50.0, 50.0, 50.0), (51.0, 51.0, 51.0))        # a box no ray of these tests hits
HUGE = ((-100.0,) * 3, (100.0,) * 3)                       # a box that contains every [near, far]
# the golden scene's content lies about here (cameras near the unit sphere, near 0.56, far 2.56); tighter than, and not to be
# replaced by, occupancy_ref.GOLDEN_BOX: the training tests need rays that miss it
TRAIN_BOX = ((-0.3, 0.0, -1.0), (0.1, 0.5, -0.7))


@pytest.fixture(scope="module")
def blobs():
    import nerf_and_dietnerf_amd as N
    return N.glorot_blob(0), N.glorot_blob(1)


@pytest.fixture(scope="module")
def rays():
    """The 130 recipe rays and the seven edge rays, with the reference's verdict on them -- and the recipe's own check: it
    shows narrowed rays, missed rays and every edge category."""
    o, d = B.recipe_rays()
    a, b, hit, narrowed = B.ray_box_interval(o, d, B.LO, B.HI, NEAR, FAR)
    assert o.shape == (137, 4)
    assert narrowed.mean() >= 0.25 and (~hit).mean() >= 0.25
    for i, (_, _, name, want) in enumerate(B.EDGE_RAYS):
        k = 130 + i
        assert (bool(narrowed[k]), bool(hit[k])) == ((True, True) if want else (False, False)), name
        if want:
            assert (float(a[k]), float(b[k])) == want, name
    return o, d, a, b, hit, narrowed


def _ctx(blobs=None, near=NEAR, far=FAR, precision="fp32", box=None, **kw):
    import nerf_and_dietnerf_amd as N
    ctx = N.Context(near=near, far=far, precision=precision, **kw)
    if blobs is not None:
        ctx.load_weights(0, blobs[0])
        ctx.load_weights(1, blobs[1])
    if box is not None:
        ctx.set_scene_box(*box)
    return ctx


def _draws(rng, n, s):
    u = rng.random((n, s), dtype=np.float32)
    u[0], u[-1] = 0.0, R.U_BELOW_ONE                                  # (the last ray is an edge ray the box narrows)
    return u


# ---- 1. the interval --------------------------------------------------------------------------------------------------------
def test_ray_box_bounds_equal_the_reference(rays):
    import torch
    o, d, a, b, hit, narrowed = rays
    ctx = _ctx(box=(B.LO, B.HI))
    want_bounds, want_flag = B.ray_box_bounds(o, d, B.LO, B.HI, NEAR, FAR)
    bounds, flag = ctx.ray_box_bounds(o, d)
    assert flag.dtype == np.int32 and bounds.dtype == np.float32
    np.testing.assert_array_equal(flag, want_flag)
    np.testing.assert_array_equal(bounds.view(np.uint32), want_bounds.view(np.uint32))
    bt, ft = ctx.ray_box_bounds(torch.as_tensor(o).cuda(), torch.as_tensor(d).cuda())     # device memory == host memory
    assert bt.is_cuda and ft.is_cuda and ft.dtype == torch.int32
    np.testing.assert_array_equal(bt.cpu().numpy(), bounds)
    np.testing.assert_array_equal(ft.cpu().numpy(), flag)
    ctx.set_scene_box(*HUGE)
    bounds, flag = ctx.ray_box_bounds(o, d)
    assert not flag.any() and np.all(bounds == np.array([NEAR, FAR], np.float32))
    ctx.set_scene_box(None)
    with pytest.raises(RuntimeError, match="no scene box"):
        ctx.ray_box_bounds(o, d)
    ctx.close()


# ---- 2. the depths ----------------------------------------------------------------------------------------------------------
def test_linear_depths_equal_the_reference(rays, oracle):
    """Explicit draws (u = 0 and u = nextafter(1, 0) among them) and on-device draws, S in {1, 2, 5, 64}: bit-equal to the
    float32 restatement on all 137 rays; narrowed rays stay in [a, b + (b - a) / S], non-decreasing."""
    o, d, a, b, hit, narrowed = rays
    ctx = _ctx(box=(B.LO, B.HI))
    rng = np.random.default_rng(7)
    an, bn = a[narrowed, None], b[narrowed, None]
    for s in SAMPLES:
        u = _draws(rng, 137, s)
        z = ctx.get_z_values_for_rays(o, d, s, uniform_values=u)
        np.testing.assert_array_equal(z.view(np.uint32), B.z_values(o, d, B.LO, B.HI, NEAR, FAR, u).view(np.uint32))
        assert np.all(z[narrowed] >= an) and np.all(z[narrowed] <= bn + (bn - an) / np.float32(s)), s
        assert np.all(np.diff(z, axis=1) >= 0), s
        # on the device: the draws of the global ray index, the same on every call
        z0 = ctx.get_z_values_for_rays(o, d, s, seed=9)
        np.testing.assert_array_equal(z0, ctx.get_z_values_for_rays(o, d, s, seed=9))
        zb = ctx.get_z_values_for_rays(o[31:51], d[31:51], s, seed=9, ray_base=31)
        np.testing.assert_array_equal(zb, z0[31:51])
        assert not np.array_equal(z0, ctx.get_z_values_for_rays(o, d, s, seed=10))
        up = oracle.philox_uniform(9, np.arange(137, dtype=np.uint64), s, 0)
        np.testing.assert_array_equal(z0, B.z_values(o, d, B.LO, B.HI, NEAR, FAR, up))
        assert np.all(z0[narrowed] >= an) and np.all(z0[narrowed] <= bn + (bn - an) / np.float32(s)), s
    ctx.close()


def test_lindisp_depths_against_the_reference(rays, capsys):
    """Disparity-linear depths on all 137 rays: the float32 restatement reproduces the kernel, so they are held to its bits
    (measured on an MI355X: 0 values differ); narrowed rays are also within the derived bar (scene_box_ref.lindisp_bar; measured
    0.224 of it) of the float64 formula on the float32 (a, b), in [a, b) and non-decreasing; rays the box leaves alone are the
    existing kernel's, bit for bit.  Prints the measured error."""
    o, d, a, b, hit, narrowed = rays
    ctx = _ctx(box=(B.LO, B.HI))
    ctx.set_sampling("lindisp")
    plain = _ctx()
    plain.set_sampling("lindisp")
    rng = np.random.default_rng(8)
    an, bn = a[narrowed], b[narrowed]
    bar = B.lindisp_bar(an, bn)[:, None]
    worst, differing = 0.0, 0
    for s in SAMPLES:
        u = _draws(rng, 137, s)
        for uu, kw in ((u, dict(uniform_values=u)), (None, dict(seed=9))):
            z = ctx.get_z_values_for_rays(o, d, s, **kw)
            if uu is None:
                np.testing.assert_array_equal(z, ctx.get_z_values_for_rays(o, d, s, seed=9))
                np.testing.assert_array_equal(ctx.get_z_values_for_rays(o[31:51], d[31:51], s, seed=9, ray_base=31), z[31:51])
                np.testing.assert_array_equal(z[~narrowed], plain.get_z_values(NEAR, FAR, 1, 137, s, seed=9).reshape(137, s)[~narrowed])
            else:
                ref32 = B.z_values(o, d, B.LO, B.HI, NEAR, FAR, uu, lindisp=True)
                differing += int((z.view(np.uint32) != ref32.view(np.uint32)).sum())
                np.testing.assert_array_equal(z[~narrowed], ref32[~narrowed])
                ref = B.lindisp_f64(an, bn, uu[narrowed])
                worst = max(worst, float((np.abs(z[narrowed] - ref) / (bar * ref)).max()))
                assert np.all(np.abs(z[narrowed] - ref) <= bar * ref), s
            assert np.all(z[narrowed] >= an[:, None]) and np.all(z[narrowed] < bn[:, None]), s
            assert np.all(np.diff(z, axis=1) >= 0), s
    with capsys.disabled():
        print(f"\n[scene box, lindisp] max |dz| / z = {worst:.3f} of the bar 9 * 2^-24 * b / a; {differing} values differ in bits "
              f"from the float32 restatement", end="")
    assert differing == 0
    ctx.close()
    plain.close()


# ---- 3. a box that narrows nothing is no box -----------------------------------------------------------------------------------
def test_a_box_that_narrows_nothing_changes_no_bit(rays, blobs):
    """A box no ray hits, a box that contains every [near, far], and set_scene_box(None) after a box: depths, the seven outputs
    of render (64 + 128 samples, fp32) and one train_gradients call equal those of a context that never had a box."""
    o, d = rays[0], rays[1]
    rng = np.random.default_rng(12)
    u5 = rng.random((137, 5), dtype=np.float32)
    u_c, u_f = rng.random((137, 64), dtype=np.float32), rng.random((137, 128), dtype=np.float32)
    ut_c, ut_f = u_c[:, :16].copy(), u_f[:, :24].copy()
    tgt = rng.random((137, 3), dtype=np.float32)

    def everything(ctx):
        got = [ctx.get_z_values_for_rays(o, d, 5, uniform_values=u5), ctx.get_z_values_for_rays(o, d, 64, seed=3)]
        got += list(ctx.render(o, d, 64, 128, u_c, u_f, want_depth=True))
        got += list(ctx.render(o, d, 64, 128, seed=3, want_depth=True))
        ctx.train_begin(5e-4)
        m, gc, gf = ctx.train_gradients(o, d, tgt, 16, 24, ut_c, ut_f)
        ctx.train_end()
        return got + [gc, gf, np.array([m[k] for k in sorted(m)])]

    fresh = _ctx(blobs)
    want = everything(fresh)
    np.testing.assert_array_equal(want[0], fresh.get_z_values(NEAR, FAR, 1, 137, 5, uniform_values=u5).reshape(137, 5))
    fresh.close()
    assert len(want) == 2 + 7 + 7 + 3
    for name, box, off_again in (("missed", FAR_AWAY, False), ("contains", HUGE, False), ("off again", (B.LO, B.HI), True)):
        ctx = _ctx(blobs, box=box)
        if off_again:
            assert not np.array_equal(ctx.get_z_values_for_rays(o, d, 5, uniform_values=u5), want[0])   # the box did act
            ctx.set_scene_box(None)
        for i, (g, w) in enumerate(zip(everything(ctx), want)):
            np.testing.assert_array_equal(g, w, err_msg=f"{name}: item {i}")
        ctx.close()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(rays, blobs):
    import nerf_and_dietnerf_amd as N
    o, d = rays[0], rays[1]
    ctx = _ctx(blobs, near=1.0, far=8.0)
    for lo, hi in (((-1, 0.75, -0.5), (1, 0.75, 0.5)), ((-1, -0.75, 0.6), (1, 0.75, 0.5)),
                   ((-1, float("nan"), -0.5), (1, 0.75, 0.5)), ((-1, -0.75, -0.5), (1, float("inf"), 0.5))):
        with pytest.raises(RuntimeError, match=BOX_MESSAGE):
            ctx.set_scene_box(lo, hi)
        lo_a, hi_a = np.array(lo, np.float32), np.array(hi, np.float32)           # the library's own check
        assert ctx.lib.nerf_ctx_set_scene_box(ctx.h, lo_a.ctypes.data, hi_a.ctypes.data) != 0
        assert BOX_MESSAGE in N._lib.last_error()
    assert ctx.lib.nerf_ctx_set_scene_box(ctx.h, np.zeros(3, np.float32).ctypes.data, None) != 0
    with pytest.raises(RuntimeError, match="no scene box"):                      # none of these left a box behind
        ctx.ray_box_bounds(o, d)
    # a box does not make disparity sampling legal at near <= 0
    ctx.set_sampling("lindisp")
    ctx.set_scene_box(B.LO, B.HI)
    ctx.set_bounds(0.0, 1.0)
    for call in (lambda: ctx.get_z_values_for_rays(o, d, 8), lambda: ctx.render(o, d, 8, 8)):
        with pytest.raises(RuntimeError, match=LINDISP_MESSAGE):
            call()
    ctx.train_begin(5e-4)
    with pytest.raises(RuntimeError, match=LINDISP_MESSAGE):
        ctx.train_gradients(o, d, np.zeros((137, 3), np.float32), 8, 8)
    ctx.close()


# ---- 5. render parity ----------------------------------------------------------------------------------------------------------
IMAGE = (16, 24)                                 # (h, w): 24 x 16 pixels
IMAGE_FOV = 0.6
_PARITY = {}


def _camera(oracle):
    return oracle.get_sphere_matrix(4.0, -30.0, 45.0, 0.0).astype(np.float32)     # 4 units from the box's centre, looking at it


def _parity_reference(oracle, blobs, lindisp):
    """Coarse depths from scene_box_ref; render_rays, the inverse CDF, the sort and the fine render_rays from the unmodified CPU
    oracle (computed once per mode)."""
    if lindisp not in _PARITY:
        h, w = IMAGE
        rng = np.random.default_rng(21)
        u_c, u_f = rng.random((h * w, 64), dtype=np.float32), rng.random((h * w, 128), dtype=np.float32)
        o, d = R.world_rays(oracle, _camera(oracle), IMAGE_FOV, h, w)
        _, _, hit, narrowed = B.ray_box_interval(o, d, B.LO, B.HI, NEAR, FAR)
        z_c = B.z_values(o, d, B.LO, B.HI, NEAR, FAR, u_c, lindisp=lindisp)
        coarse, fine = oracle.unpack_blob(blobs[0]), oracle.unpack_blob(blobs[1])
        res = oracle.render_rays(coarse, o, d, z_c)
        z_f = oracle.get_z_vals_from_prob_dist_func(res[1], z_c, u_f)
        z = np.sort(np.concatenate([z_f, z_c], axis=-1), axis=-1)
        _PARITY[lindisp] = (u_c, u_f, oracle.render_rays(fine, o, d, z)[0], z, hit, narrowed)
    return _PARITY[lindisp]


@pytest.mark.parametrize("precision,lindisp", [("fp32", False), ("f16x3", False), ("bf16x3", False), ("fp32", True)])
def test_parity_end_to_end(oracle, blobs, precision, lindisp, capsys):
    """NeRF(render_config with scene_box).render_image on a 24 x 16 image at 64 + 128 samples, Glorot weights, explicit draws:
    final RGB within the project's 1e-4 bar (tests/test_gpu_parity.py) of the unmodified CPU oracle on the reference's coarse
    depths.  The image holds narrowed rays and rays that miss the box."""
    import nerf_and_dietnerf_amd as N
    h, w = IMAGE
    u_c, u_f, ref, ref_z, hit, narrowed = _parity_reference(oracle, blobs, lindisp)
    assert narrowed.sum() >= h * w // 8 and (~hit).sum() >= h * w // 8
    rc = {"n_render_samples_coarse": 64, "n_render_samples_fine": 128, "scene_box": [B.LO.tolist(), B.HI.tolist()], "lindisp": lindisp}
    model = N.NeRF(S.NET, rc, NEAR, FAR, precision=precision)
    assert model.ctx.scene_box == (tuple(B.LO.tolist()), tuple(B.HI.tolist()))
    model.set_weights(*blobs)
    out = model.render_image(_camera(oracle), IMAGE_FOV, h, w, u_coarse=u_c, u_fine=u_f)
    err = float(np.abs(out[0].reshape(-1, 3) - ref).max())
    with capsys.disabled():
        print(f"\n[{precision}, scene box{' + lindisp' if lindisp else ''}] max-abs RGB error vs the oracle {err:.3e}; "
              f"max |dz| {np.abs(out[5].reshape(ref_z.shape) - ref_z).max():.3e}; {int(narrowed.sum())} rays narrowed, "
              f"{int((~hit).sum())} miss", end="")
    assert np.isfinite(out[0]).all() and err <= 1e-4
    assert model.ctx.read_nonfinite() == 0
    model.ctx.close()


# ---- 6. render_image under NDC ---------------------------------------------------------------------------------------------------
def test_render_image_in_ndc_mode_clips_the_ndc_rays(blobs):
    """use_ndc + scene_box: render_image == get_rays_directions -> rays_to_ndc -> render with the same box, bit for bit -- the box
    acts on the rays the depth kernel sees.  The whole image and a slab, two batch sizes."""
    import nerf_and_dietnerf_amd as N
    poses, fov = R.forward_facing_poses()
    (h, w), sc, sf, seed = (16, 24), 16, 24, 5
    rc = {"n_render_samples_coarse": sc, "n_render_samples_fine": sf, "use_ndc": True, "ndc_near_plane": NDC_NEAR,
          "scene_box": [list(NDC_BOX[0]), list(NDC_BOX[1])]}
    model = N.NeRF(S.NET, rc, 0.0, 1.0, precision="fp32")
    model.set_weights(*blobs)
    ndc = model.ctx
    plain = _ctx(blobs, near=0.0, far=1.0, box=NDC_BOX)
    nobox = _ctx(blobs, near=0.0, far=1.0)
    c2w = poses[1]
    dirs = plain.get_rays_directions(h, w, fov, c2w).reshape(-1, 4)
    orig = np.tile(c2w[:, 3], (h * w, 1)).astype(np.float32)
    o, d = plain.rays_to_ndc(orig, dirs, fov, NDC_NEAR)
    _, flag = plain.ray_box_bounds(o, d)
    assert 0 < flag.sum() < h * w                                   # some NDC rays are narrowed, some are not
    _, flag_world = plain.ray_box_bounds(orig, dirs)
    assert not np.array_equal(flag, flag_world)                     # and the world rays would be clipped differently
    want = plain.render(o, d, sc, sf, seed=seed, want_depth=True)
    assert not np.array_equal(want[0], nobox.render(o, d, sc, sf, seed=seed)[0])
    for batch in (0, 100):
        got = ndc.render_image(c2w, fov, h, w, batch, sc, sf, seed=seed, want_depth=True)
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a.reshape(b.shape), b)
    begin, count = 37, 101
    got = ndc.render_image(c2w, fov, h, w, 64, sc, sf, seed=seed, ray_begin=begin, ray_count=count, want_depth=True)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b[begin:begin + count])
    for c in (ndc, plain, nobox):
        c.close()


# ---- 7. training follows the box ---------------------------------------------------------------------------------------------------
def _golden_rays(oracle, golden_ckpt, n, seed):
    """n rays of the golden checkpoint's training camera (8 x 8 pixels), its bounds, and the reference's verdict under TRAIN_BOX."""
    near, far = float(golden_ckpt["near"]), float(golden_ckpt["far"])
    o, d = R.world_rays(oracle, golden_ckpt["c2w_train"], float(golden_ckpt["fov"]), 8, 8)
    idx = np.random.default_rng(seed).choice(64, n, replace=False)
    o, d = o[idx], np.ascontiguousarray(d[idx])
    _, _, hit, narrowed = B.ray_box_interval(o, d, *TRAIN_BOX, near, far)
    assert narrowed.sum() >= n // 4 and (~hit).sum() >= n // 4
    return o, d, near, far


@pytest.mark.parametrize("policy", ["float32", "mixed_float16"])
def test_train_gradients_follow_the_box(oracle, golden_ckpt, policy, capsys):
    """One train_gradients call with the box and draws u against one without a box and with the per-ray draws
    u' = (z_box - linspace(near, far, S)[s]) S / (far - near), which put the plain context's depths on the same values up to
    rounding (draws outside [0, 1) are fine when they are explicit).  Bars of test_train_gradients_follow_the_sampling_mode:
    loss within 2e-6 relative (2e-3 under mixed_float16), both blobs within 5e-2 of max|g|, cosine > 0.999.  48 rays x (16 + 24)."""
    n, sc, sf = 48, 16, 24
    o, d, near, far = _golden_rays(oracle, golden_ckpt, n, 3)
    rng = np.random.default_rng(4)
    u_c, u_f = rng.random((n, sc), dtype=np.float32), rng.random((n, sf), dtype=np.float32)
    tgt = rng.random((n, 3), dtype=np.float32)
    mixed = policy == "mixed_float16"
    w = (golden_ckpt["blob_coarse"], golden_ckpt["blob_fine"])
    res = {}
    for mode in ("box", "substituted", "plain"):
        ctx = _ctx(w, near=near, far=far, box=TRAIN_BOX if mode == "box" else None)
        if mode == "box":
            z_box = ctx.get_z_values_for_rays(o, d, sc, uniform_values=u_c)
            u = u_c
        elif mode == "substituted":
            u = ((z_box.astype(np.float64) - oracle.linspace_f32(near, far, sc)[None, :]) * sc / (far - near)).astype(np.float32)
            z_sub = ctx.get_z_values_for_rays(o, d, sc, uniform_values=u)
            np.testing.assert_array_equal(z_sub, ctx.get_z_values(near, far, 1, n, sc, uniform_values=u).reshape(n, sc))
            assert np.abs(z_sub - z_box).max() <= 4 * B.U * far                  # the same depths, to rounding
        else:
            u = u_c                                                              # the box's draws without the box
        ctx.train_begin(5e-4, mixed_float16=mixed)
        res[mode] = ctx.train_gradients(o, d, tgt, sc, sf, u, u_f)
        ctx.train_end()
        ctx.close()
    (m0, gc0, gf0), (m1, gc1, gf1), (m2, _, _) = res["box"], res["substituted"], res["plain"]
    with capsys.disabled():
        print(f"\n[{policy}] box vs no box on the same depths: loss {m0['loss']:.7f} / {m1['loss']:.7f} (no box, same draws: "
              f"{m2['loss']:.7f}), gradients {S.relerr(gc0, gc1):.2e} (coarse), {S.relerr(gf0, gf1):.2e} (fine) of max|g|", end="")
    assert np.isfinite(gc0).all() and np.isfinite(gf0).all()
    assert abs(m0["loss"] - m1["loss"]) <= (2e-3 if mixed else 2e-6) * m1["loss"]
    assert S.relerr(gc0, gc1) <= 5e-2 and S.cos(gc0, gc1) > 0.999
    assert S.relerr(gf0, gf1) <= 5e-2 and S.cos(gf0, gf1) > 0.999
    assert abs(m2["loss"] - m0["loss"]) > 1e-4 * m0["loss"]                      # and the box matters


# ---- 8. slots ------------------------------------------------------------------------------------------------------------------------
def test_a_slot_keeps_the_depths_it_drew(oracle, golden_ckpt):
    """train_render_forward with a box, set_scene_box(None), train_render_backward: the gradients are those of
    train_render_gradients with the box on, bit for bit.  50 rays x (8 + 16)."""
    n, sc, sf = 50, 8, 16
    o, d, near, far = _golden_rays(oracle, golden_ckpt, n, 6)
    rng = np.random.default_rng(9)
    d_rgb = (rng.random((n, 3), dtype=np.float32) - 0.5) / n
    w = (golden_ckpt["blob_coarse"], golden_ckpt["blob_fine"])
    ctx = _ctx(w, near=near, far=far, box=TRAIN_BOX)
    ctx.train_begin(5e-4)
    rgb, gc, gf = ctx.train_render_gradients(o, d, d_rgb, sc, sf, seed=7, ray_base=11)
    rgb_slot = ctx.train_render_forward(0, o, d, sc, sf, seed=7, ray_base=11)
    ctx.set_scene_box(None)
    gc_slot, gf_slot = ctx.train_render_backward(0, d_rgb)
    np.testing.assert_array_equal(rgb_slot, rgb)
    np.testing.assert_array_equal(gc_slot, gc)
    np.testing.assert_array_equal(gf_slot, gf)
    assert np.abs(gf).max() > 0
    rgb_off, _, gf_off = ctx.train_render_gradients(o, d, d_rgb, sc, sf, seed=7, ray_base=11)   # the box is off now: another render
    assert not np.array_equal(rgb_off, rgb) and not np.array_equal(gf_off, gf)
    ctx.train_end()
    ctx.close()


# ---- 9. sharded render -------------------------------------------------------------------------------------------------------------
def _rank_main(rank, world, p, id_path, q):
    try:
        import nerf_and_dietnerf_amd as N
        ctx = N.Context(near=NEAR, far=FAR, precision="fp32")
        ctx.load_weights(0, p["blobs"][0])
        ctx.load_weights(1, p["blobs"][1])
        ctx.set_scene_box(*p["box"])
        ctx.comm_init(S.exchange_comm_id(N, rank, id_path), rank, world)
        h, w = p["hw"]
        img = ctx.render_image_sharded(p["c2w"], p["fov"], h, w, 0, 16, 24, seed=5)
        six = ctx.render_image_sharded(p["c2w"], p["fov"], h, w, 0, 16, 24, seed=5, outputs="all")
        S.assert_stand_in_loaded()
        ctx.comm_destroy()
        q.put((rank, (img, six[5])))
    except BaseException as e:
        import traceback
        q.put((rank, RuntimeError(f"rank {rank}: {e}\n{traceback.format_exc()}")))
        raise


def test_sharded_render_with_a_box(oracle, blobs, tmp_path):
    """nerf_render_image_sharded over two ranks (the test-only RCCL stand-in, tests/stub_rccl.c) on contexts with a box == the
    one-context image, bit for bit."""
    h, w = 7, 13                                                  # 91 rays: the second slab is one ray short
    c2w = _camera(oracle)
    one = _ctx(blobs, box=(B.LO, B.HI))
    want = one.render_image(c2w, IMAGE_FOV, h, w, 0, 16, 24, seed=5)
    one.set_scene_box(None)
    assert not np.array_equal(want[5], one.render_image(c2w, IMAGE_FOV, h, w, 0, 16, 24, seed=5)[5])    # the box is not a no-op
    one.close()
    p = dict(blobs=blobs, c2w=c2w, fov=IMAGE_FOV, hw=(h, w), box=(B.LO.tolist(), B.HI.tolist()))
    res = S.run_ranks(_rank_main, 2, (p, str(tmp_path / "comm_id")), S.build_stub_rccl(tmp_path), timeout=300)
    for img, z in res:
        np.testing.assert_array_equal(img, want[0])
        np.testing.assert_array_equal(z, want[5])
