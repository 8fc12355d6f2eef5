"""Sample culling on the device: the verdict (nerf_sample_occupancy) bit for bit against the float32 restatement of
tests/culling_ref.py; the culled render path against the same network on the compacted rows the restatement names, bit for
bit; and the layers above it -- render, render_image, the trainer (which ignores the flag), NeRF.  Every test here needs the
entry points culling adds to the ABI."""
import ctypes as C

import numpy as np
import pytest

import culling_ref as K
import occupancy_ref as G
import support as S

pytestmark = pytest.mark.gpu

NEAR, FAR = G.NEAR, G.FAR
WIDE_BOX = ((-1.5, -1.5, -2.2), (1.5, 1.5, 0.5))
NO_GRID = "no occupancy grid"
PRECISIONS = ["fp32", "f16x3", "f16", "bf16x3"]


# ---- 1. the verdict ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    import nerf_and_dietnerf_amd as N
    c = N.Context(near=NEAR, far=FAR, precision="fp32")
    yield c
    c.close()


@pytest.fixture(scope="module")
def world(ctx):
    """The six hand rays of the grid's tests, then 4090 rays of its recipe: 4096 in all."""
    return G.world_scene(4096)


@pytest.fixture(scope="module")
def ndc(ctx):
    """A 65 x 65 image of a forward-facing camera through rays_to_ndc (its first 4096 rays), bounds 0 and 1."""
    return G.ndc_scene(ctx, 4096)


@pytest.mark.parametrize("n", [1, 63, 65, 4096])
@pytest.mark.parametrize("s", [1, 55])
@pytest.mark.parametrize("r", [4, 16])
@pytest.mark.parametrize("space", ["world", "ndc"])
def test_verdicts_equal_the_restatement(ctx, world, ndc, space, r, s, n):
    """Depths drawn on the grid's own bounds, as a render draws them; one wave, a wave and a lane, many blocks."""
    o, d, lo, hi, near, far = world if space == "world" else ndc
    grid = G.grid_for(r, lo, hi)
    u = np.random.default_rng(s).random((4096, s), dtype=np.float32)
    z = np.ascontiguousarray(G.z_values(o, d, lo, hi, near, far, grid, u)[:n])
    o, d = o[:n], d[:n]
    want = K.sample_keep(o, d, z, lo, hi, grid, K.F32)
    G.arm(ctx, lo, hi, near, far, grid)
    keep = ctx.sample_occupancy(o, d, z)
    assert keep.dtype == np.int32 and keep.shape == (n, s)
    np.testing.assert_array_equal(keep, want.astype(np.int32))
    if n == 4096 and s == 55:
        assert 0.05 < want.mean() < 0.95, want.mean()                    # the input shows kept and culled samples
    if n == 65:                                                         # device memory == host memory
        import torch
        kt = ctx.sample_occupancy(torch.as_tensor(o).cuda(), torch.as_tensor(d).cuda(), torch.as_tensor(z).cuda())
        assert kt.is_cuda and kt.dtype == torch.int32
        np.testing.assert_array_equal(kt.cpu().numpy(), keep)


def test_hand_cases_on_the_device(ctx):
    """A point on the hi face, on an interior cell face, outside the box, and a NaN depth (tests/culling_ref.py)."""
    for grid, want in K.hand_grids():
        G.arm(ctx, K.HAND_LO, K.HAND_HI, NEAR, FAR, grid)
        assert ctx.sample_occupancy(K.HAND_O, K.HAND_D, K.HAND_Z).tolist() == [[int(w) for w in want]]


# ---- the golden checkpoint -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold(golden_ckpt):
    import nerf_and_dietnerf_amd as N
    c = N.Context(near=float(golden_ckpt["near"]), far=float(golden_ckpt["far"]), precision="fp32")
    c.load_weights(0, golden_ckpt["blob_coarse"])
    c.load_weights(1, golden_ckpt["blob_fine"])
    yield c
    c.close()


def _gold_arm(c, precision, grid, cull, box=G.GOLDEN_BOX):
    c.set_precision(precision)
    c.set_scene_box(*box)
    if grid is not None:
        c.set_occupancy_grid(grid)
    c.set_sample_culling(cull)
    c.read_culling()


def _outputs7(n, s):
    from nerf_and_dietnerf_amd._lib import NerfOutputs
    arrays = [np.empty(shape, np.float32) for shape in ((n, 3), (n, s), (n, s), (n, s), (n, s, 3), (n, s), (n,))]
    return NerfOutputs(*[a.ctypes.data for a in arrays]), arrays


def _ray_marching7(c, raw, z):
    from nerf_and_dietnerf_amd import _lib
    n, s = z.shape
    outs, arrays = _outputs7(n, s)
    raw, z = np.ascontiguousarray(raw, np.float32), np.ascontiguousarray(z, np.float32)
    _lib.check(c.lib.nerf_ray_marching(c.h, raw.ctypes.data, z.ctypes.data, n, s, C.byref(outs), _lib.NERF_MEM_HOST))
    return arrays


# ---- 2. off is off -------------------------------------------------------------------------------------------------------------
def test_culling_without_a_grid_is_off(oracle, golden_ckpt, gold):
    o, d = K.camera_rays(oracle, golden_ckpt, 130)
    rng = np.random.default_rng(2)
    u_c, u_f = rng.random((130, 8), dtype=np.float32), rng.random((130, 16), dtype=np.float32)
    _gold_arm(gold, "f16x3", None, False)
    want = gold.render(o, d, 8, 16, u_c, u_f, want_depth=True)
    z = gold.get_z_values_for_rays(o, d, 8, uniform_values=u_c)
    want_rays = S.render_rays(gold, 0, o, d, z, S.RENDER_OUTPUTS)
    gold.set_sample_culling(True)
    S.assert_same_bits_each(gold.render(o, d, 8, 16, u_c, u_f, want_depth=True), want)
    S.assert_same_bits_each(S.render_rays(gold, 0, o, d, z, S.RENDER_OUTPUTS), want_rays)
    assert gold.read_culling() == (0, 0)
    with pytest.raises(RuntimeError, match=NO_GRID):
        gold.sample_occupancy(o, d, z)
    # the flag outlives a grid that comes and goes
    gold.set_occupancy_grid(K.HALF_GRID)
    gold.set_occupancy_grid(None)
    assert gold.sample_culling
    S.assert_same_bits_each(S.render_rays(gold, 0, o, d, z, S.RENDER_OUTPUTS), want_rays)
    assert gold.read_culling() == (0, 0)
    gold.set_sample_culling(False)


# ---- 3. render_rays against compacted rows ---------------------------------------------------------------------------------------
RAY_SIZES = [(1, 2), (130, 24), (521, 40)]


@pytest.fixture(scope="module")
def compact_scene(oracle, golden_ckpt, gold):
    """Per size: rays, the depths the context draws for them under the random grid, and the restatement's verdict."""
    _gold_arm(gold, "fp32", K.HALF_GRID, False)
    out = {}
    for n, s in RAY_SIZES:
        o, d = K.camera_rays(oracle, golden_ckpt, n)
        z = gold.get_z_values_for_rays(o, d, s, seed=n)
        keep = K.sample_keep(o, d, z, *G.GOLDEN_BOX, K.HALF_GRID, K.F32)
        out[(n, s)] = (o, d, z, keep)
    assert any(v[3].sum() % 128 != 0 for v in out.values())              # a last tile of the network kernels that is not full
    assert any(v[3].any() and not v[3].all() for v in out.values())      # kept and culled samples exist
    big = out[RAY_SIZES[-1]][3]
    assert 0.2 < big.mean() < 0.9 and big[-10:].all()                     # the rays that miss the box keep every sample
    return out


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("n,s", RAY_SIZES)
def test_render_rays_equals_the_network_on_the_compacted_rows(gold, compact_scene, n, s, which, precision):
    o, d, z, keep = compact_scene[(n, s)]
    pts = K.sample_points(o, d, z, K.F32)
    dirs = np.broadcast_to(d[:, None, :3], (n, s, 3))
    _gold_arm(gold, precision, K.HALF_GRID, False)
    m = int(keep.sum())
    raw_c = gold.model_predict(which, np.ascontiguousarray(pts[keep]), np.ascontiguousarray(dirs[keep])) if m else np.zeros((0, 4), np.float32)
    # row independence, which the bake already relies on: the network on all rows, restricted to the kept ones
    raw_all = gold.model_predict(which, np.ascontiguousarray(pts.reshape(-1, 3)), np.ascontiguousarray(dirs.reshape(-1, 3)))
    np.testing.assert_array_equal(S.bits(raw_all.reshape(n, s, 4)[keep]), S.bits(raw_c))
    want = _ray_marching7(gold, K.scatter_rows(raw_c, keep), z)
    gold.set_sample_culling(True)
    gold.read_culling()
    got = S.render_rays(gold, which, o, d, z, S.RENDER_OUTPUTS)
    assert gold.read_culling() == (n * s, m)
    assert gold.read_culling() == (0, 0)                                  # read clears
    gold.set_sample_culling(False)
    S.assert_same_bits_each(got, want)
    culled = ~keep
    if culled.any():                                                      # what the rule promises of a culled sample
        assert not got[1][culled].any() and not got[3][culled].any() and (got[4][culled] == 0.5).all()


# ---- 4. the hierarchical render is the chain done by hand ------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_render_equals_the_chain_done_by_hand(oracle, golden_ckpt, gold, precision):
    """render's coarse pass is the sigma-only network where the precision has one (f16x3): this pins the culled sigma-only pass
    to the culled full one."""
    n, sc, sf = 130, 8, 16
    o, d = K.camera_rays(oracle, golden_ckpt, n)
    rng = np.random.default_rng(4)
    u_c, u_f = rng.random((n, sc), dtype=np.float32), rng.random((n, sf), dtype=np.float32)
    _gold_arm(gold, precision, K.HALF_GRID, True)
    got = gold.render(o, d, sc, sf, u_c, u_f, want_depth=True)
    samples, kept = gold.read_culling()
    assert samples == n * (sc + sc + sf) and 0 < kept < samples
    zc = gold.get_z_values_for_rays(o, d, sc, uniform_values=u_c)
    weights = S.render_rays(gold, 0, o, d, zc, S.RENDER_OUTPUTS)[1]
    _, zf = gold.get_z_vals_from_prob_dist_func(weights, zc, sf, uniform_values=u_f, return_merged=True)
    want = S.render_rays(gold, 1, o, d, zf, S.RENDER_OUTPUTS)
    gold.set_sample_culling(False)
    S.assert_same_bits_each(got, want)
    S.assert_same_bits_each([got[5]], [zf])


# ---- 5. nothing kept ---------------------------------------------------------------------------------------------------------
def test_nothing_kept(oracle, golden_ckpt, gold):
    """An all-zero grid and rays whose depths all lie inside the box: no row reaches the network and every output is an exact
    zero.  With ten rays that miss the box appended, those equal the culling-off render bit for bit."""
    n, s = 130, 24
    o, d = K.camera_rays(oracle, golden_ckpt, n)
    empty = np.zeros((16, 16, 16), bool)
    _gold_arm(gold, "f16x3", empty, False)
    bounds, narrowed = gold.ray_box_bounds(o, d)
    hit = narrowed == 1
    assert hit[:-10].sum() >= 30 and not hit[-10:].any()
    oi, di, bi = o[hit], d[hit], bounds[hit]
    t = (np.arange(s, dtype=np.float32) + np.float32(0.5)) / np.float32(s)
    zi = (bi[:, :1] + (bi[:, 1:] - bi[:, :1]) * t[None, :]).astype(np.float32)
    inside, _ = K.sample_cells(oi, di, zi, *G.GOLDEN_BOX, 16, K.F32)
    assert inside.all() and not K.sample_keep(oi, di, zi, *G.GOLDEN_BOX, empty, K.F32).any()
    gold.set_sample_culling(True)
    gold.read_culling()
    got = S.render_rays(gold, 1, oi, di, zi, S.RENDER_OUTPUTS)
    assert gold.read_culling() == (zi.size, 0)
    for k in (0, 1, 3, 6):                                                # rgb, weights, alpha, depth
        assert np.isfinite(got[k]).all() and not got[k].any()
    assert (got[2] == 1.0).all() and (got[4] == 0.5).all()                # the transmittance is untouched; sigmoid(0)
    # the same with the ten rays that miss the box
    om, dm = np.concatenate([oi, o[-10:]]), np.concatenate([di, d[-10:]])
    zm = np.concatenate([zi, np.tile(zi[:1], (10, 1))])
    assert K.sample_keep(om, dm, zm, *G.GOLDEN_BOX, empty, K.F32)[-10:].all()
    got = S.render_rays(gold, 1, om, dm, zm, S.RENDER_OUTPUTS)
    assert gold.read_culling() == (zm.size, 10 * s)
    gold.set_sample_culling(False)
    off = S.render_rays(gold, 1, om, dm, zm, S.RENDER_OUTPUTS)
    S.assert_same_bits_each([g[-10:] for g in got], [w[-10:] for w in off])
    assert not got[0][:-10].any() and not got[1][:-10].any() and not got[6][:-10].any()
    assert off[1][:-10].any()                                            # and without culling those rays do see the network


# ---- 6. a full grid ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_full_grid_is_culling_off(oracle, golden_ckpt, gold, precision):
    """Every sample kept: the network in point mode on the gathered points against ray mode, which forms the same points with the
    same two rounded operations."""
    n, sc, sf = 130, 8, 16
    o, d = K.camera_rays(oracle, golden_ckpt, n)
    rng = np.random.default_rng(6)
    u_c, u_f = rng.random((n, sc), dtype=np.float32), rng.random((n, sf), dtype=np.float32)
    _gold_arm(gold, precision, np.ones((16, 16, 16), bool), False)
    want = gold.render(o, d, sc, sf, u_c, u_f, want_depth=True)
    gold.set_sample_culling(True)
    got = gold.render(o, d, sc, sf, u_c, u_f, want_depth=True)
    assert gold.read_culling() == (n * (2 * sc + sf), n * (2 * sc + sf))
    gold.set_sample_culling(False)
    S.assert_same_bits_each(got, want)


# ---- 7. render_image ---------------------------------------------------------------------------------------------------------
def test_render_image_is_slab_and_batch_invariant_with_culling(golden_ckpt, gold):
    (h, w), sc, sf, seed = (23, 23), 8, 16, 5
    c2w, fov = golden_ckpt["c2w_train"], float(golden_ckpt["fov"])
    _gold_arm(gold, "f16x3", K.HALF_GRID, True)
    whole = gold.render_image(c2w, fov, h, w, 0, sc, sf, seed=seed, want_depth=True)
    samples, kept = gold.read_culling()
    assert samples == h * w * (2 * sc + sf) and 0 < kept < samples
    S.assert_same_bits_each(gold.render_image(c2w, fov, h, w, 100, sc, sf, seed=seed, want_depth=True), whole)
    first = gold.render_image(c2w, fov, h, w, 0, sc, sf, seed=seed, ray_begin=0, ray_count=200, want_depth=True)
    rest = gold.render_image(c2w, fov, h, w, 64, sc, sf, seed=seed, ray_begin=200, ray_count=329, want_depth=True)
    flat = [a.reshape((h * w,) + a.shape[2:]) for a in whole]
    S.assert_same_bits_each([np.concatenate([a, b]) for a, b in zip(first, rest)], flat)
    gold.set_sample_culling(False)
    off = gold.render_image(c2w, fov, h, w, 0, sc, sf, seed=seed, want_depth=True)
    assert not np.array_equal(off[1], whole[1])                           # and culling did act


# ---- 8. the trainer ----------------------------------------------------------------------------------------------------------
def test_the_trainer_ignores_the_flag(oracle, golden_ckpt):
    import nerf_and_dietnerf_amd as N
    n, sc, sf = 130, 8, 16
    o, d = K.camera_rays(oracle, golden_ckpt, n)
    rng = np.random.default_rng(8)
    u_c, u_f = rng.random((n, sc), dtype=np.float32), rng.random((n, sf), dtype=np.float32)
    tgt = rng.random((n, 3), dtype=np.float32)
    res = []
    for cull in (False, True):
        c = N.Context(near=float(golden_ckpt["near"]), far=float(golden_ckpt["far"]), precision="fp32")
        c.load_weights(0, golden_ckpt["blob_coarse"])
        c.load_weights(1, golden_ckpt["blob_fine"])
        c.set_scene_box(*G.GOLDEN_BOX)
        c.set_occupancy_grid(K.HALF_GRID)
        c.set_sample_culling(cull)
        c.train_begin(5e-4, mixed_float16=False)
        res.append(c.train_gradients(o, d, tgt, sc, sf, u_c, u_f))
        c.train_end()
        assert c.read_culling() == (0, 0)
        c.close()
    (m0, gc0, gf0), (m1, gc1, gf1) = res
    assert m0 == m1 and np.isfinite(gc0).all() and gc0.any()
    S.assert_same_bits_each([gc1, gf1], [gc0, gf0])


# ---- 9. the model class --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cull", [True, False])
def test_render_config_turns_culling_on(golden_ckpt, cull):
    import nerf_and_dietnerf_amd as N
    rc = {"n_render_samples_coarse": 8, "n_render_samples_fine": 16, "scene_box": [list(G.GOLDEN_BOX[0]), list(G.GOLDEN_BOX[1])],
          "occupancy_grid": {"resolution": 16, "sigma_threshold": 10.0, "dilate": 0, "cull_samples": cull}}
    m = N.NeRF(S.NET, rc, float(golden_ckpt["near"]), float(golden_ckpt["far"]), precision="f16x3")
    m.set_weights(golden_ckpt["blob_coarse"], golden_ckpt["blob_fine"])
    assert m.ctx.sample_culling is cull
    count = m.update_occupancy_grid()
    assert 0 < count < 16 ** 3
    out = m.render_image(golden_ckpt["c2w_train"], float(golden_ckpt["fov"]), 12, 11, seed=1)
    assert np.isfinite(out[0]).all()
    samples, kept = m.ctx.read_culling()
    if cull:
        assert samples == 12 * 11 * (8 + 8 + 16) and 0 < kept < samples
    else:
        assert (samples, kept) == (0, 0)
    m.ctx.close()


# ---- 10. quality on the shipped checkpoint ---------------------------------------------------------------------------------------
def _psnr(a, b):
    return float(-10 * np.log10(np.mean((np.asarray(a, np.float64) - b) ** 2)))


# PSNR culling may cost on the held-out view: twice the drop measured when the test was written, but at least the seed
# spread of the culling-off figure (0.03 dB).  Measured on an MI355X: off 27.7944, on 27.8354 -- a drop
# of -0.041 dB (culling came out higher), 94.3 % of the samples kept -- so the seed spread is the bar.
QUALITY_MEASURED_DROP_DB = -0.0409
QUALITY_BAR_DB = max(2 * QUALITY_MEASURED_DROP_DB, 0.03)


def test_quality_on_the_shipped_checkpoint(golden_ckpt, capsys):
    """The held-out view, 50 x 50, 64+128, f16x3, box [-1.5, 1.5]^2 x [-2.2, 0.5], grid baked from the fine network at R = 64,
    threshold 5, 2 points per cell, dilate 1: fine PSNR against the golden image, mean of seeds 1-3, culling on against off."""
    import nerf_and_dietnerf_amd as N
    near, far, fov = float(golden_ckpt["near"]), float(golden_ckpt["far"]), float(golden_ckpt["fov"])
    img = golden_ckpt["img_test"].astype(np.float64) / 255.0
    c2w = golden_ckpt["c2w_test"]
    c = N.Context(near=near, far=far, precision="f16x3")
    c.load_weights(0, golden_ckpt["blob_coarse"])
    c.load_weights(1, golden_ckpt["blob_fine"])
    c.set_scene_box(*WIDE_BOX)
    count = c.bake_occupancy_grid(1, 64, 5.0, samples_per_cell=2, dilate=1)
    psnr = {}
    for cull in (False, True):
        c.set_sample_culling(cull)
        c.read_culling()
        psnr[cull] = [_psnr(c.render_image(c2w, fov, 50, 50, 0, 64, 128, seed=s)[0], img) for s in (1, 2, 3)]
    samples, kept = c.read_culling()
    c.close()
    off, on = float(np.mean(psnr[False])), float(np.mean(psnr[True]))
    with capsys.disabled():
        print(f"\n[culling quality] {count} of {64 ** 3} cells occupied; PSNR off {off:.4f} {np.round(psnr[False], 4).tolist()}, on {on:.4f} "
              f"{np.round(psnr[True], 4).tolist()}: drop {off - on:.4f} dB (bar {QUALITY_BAR_DB}); kept {kept} of {samples} samples "
              f"({kept / samples:.3f})", end="")
    assert np.isfinite(on) and np.isfinite(off) and 0 < kept < samples
    assert off - on <= QUALITY_BAR_DB
