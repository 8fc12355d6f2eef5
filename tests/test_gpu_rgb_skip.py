"""The rgb-skipping fine kernel of the f16x3 mode (mlp_f16x3_rgbskip_kernel, csrc/mlp_f16x3.hip; chosen by dev_render_rays,
csrc/nerf_api.hip, when the caller reads rgb but no per-sample rgb): a 128-row tile whose every row has raw sigma <= 0 skips
layer 8's rgb half and the rgb head.  Such a row has alpha = 0 exactly, so the frame must not change by a bit.

The reference is always the path that cannot skip: the same context rendering all six outputs (rgb_samples among them), which
runs the full kernel.  f16x3, bench.py's Glorot blobs 0 / 1, its pose and its bounds unless a case says otherwise."""
import numpy as np
import pytest

import bench
import occupancy_ref as G
import support as S

pytestmark = pytest.mark.gpu

H = W = bench.H
SC, SF = bench.SC, bench.SF
C2W = bench.sphere_matrix(1.0, -30.0, 45.0, 0.0)
# the eight blocks of the CPU measurement: linspace(0, H W - 128, 8) (all even); a 400-ray slab must end inside the frame, so
# the last one starts 272 rays early and still holds its block
SLABS = [min(int(b), H * W - 400) for b in np.linspace(0, H * W - 128, 8)]


def _bench_context(blob_c=None, blob_f=None, near=bench.NEAR, far=bench.FAR):
    """f16x3 on bench.py's bounds; a blob that is not given is bench.py's Glorot blob of that network."""
    import nerf_and_dietnerf_amd as N
    pair = (N.glorot_blob(0) if blob_c is None else blob_c, N.glorot_blob(1) if blob_f is None else blob_f)
    return S.blob_context(pair, near=near, far=far)


def _counts(ctx, which=1):
    """(tiles the rgb-skipping kernel ran, tiles it skipped, launches the gate still sends to the full kernel) of a network"""
    import ctypes as C

    from nerf_and_dietnerf_amd import _lib
    out = (C.c_ulonglong * 3)()
    fn = ctx.lib.nerf_debug_rgb_skip_counts
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_ulonglong)]
    _lib.check(fn(ctx.h, which, out))
    return int(out[0]), int(out[1]), int(out[2])


def _both(ctx, c2w, fov, h, w, sc, sf, seed=2, begin=0, count=0):
    """-> (six-output run incl. depth: the full kernel, rgb_only run incl. depth, (tiles, skipped) the rgb-skipping kernel
    counted during the rgb_only run); the six-output run must not touch that kernel"""
    c0 = _counts(ctx)
    six = ctx.render_image(c2w, fov, h, w, 0, sc, sf, seed=seed, ray_begin=begin, ray_count=count, want_depth=True)
    c1 = _counts(ctx)
    assert c1[:2] == c0[:2], "the six-output run ran the rgb-skipping kernel"
    only = ctx.render_image(c2w, fov, h, w, 0, sc, sf, seed=seed, ray_begin=begin, ray_count=count, want_depth=True,
                            rgb_only=True)
    c2 = _counts(ctx)
    return six, only, (c2[0] - c1[0], c2[1] - c1[1])


def _identity(ctx, c2w, fov, h, w, sc, sf, label, tiles=None, **kw):
    """tiles: the 128-row tiles the rgb-skipping kernel must have run for the rgb_only frame (default: the fine launch's, no
    culling); -> (six-output run, tiles skipped)"""
    six, only, (ran, skipped) = _both(ctx, c2w, fov, h, w, sc, sf, **kw)
    assert np.isfinite(six[0]).all(), label
    S.assert_same_bits(only[0], six[0], label + ": rgb")
    S.assert_same_bits(only[6], six[6], label + ": depth")
    rays = kw.get("count") or h * w
    want = -(-rays * (sc + sf) // 128) if tiles is None else tiles
    assert ran == want if want is not None and want >= 0 else ran > 0, (label, "tiles of the rgb-skipping kernel", ran, want)
    return six, skipped


def _empty_groups(alpha):
    """per 128-row group of the fine launch (rows = ray-major samples): whether every alpha is 0"""
    a = np.asarray(alpha, np.float32).reshape(-1)
    pad = (-a.size) % 128
    a = np.concatenate([a, np.zeros(pad, np.float32)])
    return (a.reshape(-1, 128) == 0).all(axis=1)


def test_mixed_groups_are_bit_identical():
    """400-ray slabs of the bench frame: 76 800 fine rows = 600 groups over at most 256 workgroups, so every workgroup runs two
    or three tiles and skipped and computed tiles follow each other either way round."""
    ctx = _bench_context()
    try:
        empty = []
        for b in SLABS:
            six, skipped = _identity(ctx, C2W, bench.FOV, H, W, SC, SF, f"slab {b}", begin=b, count=400)
            empty.append(_empty_groups(six[3]))
            print(f"slab {b}: {empty[-1].mean():.3f} of {empty[-1].size} groups all empty, the kernel skipped {skipped}")
            # the kernel votes on sigma <= 0, the host count on alpha == 0, which a tiny positive sigma also gives
            assert 0 < skipped <= int(empty[-1].sum()) and skipped >= 0.9 * empty[-1].sum(), (b, skipped, int(empty[-1].sum()))
        assert ctx.read_nonfinite() == 0
        share = float(np.concatenate(empty).mean())
        print(f"all slabs: {share:.3f} of the groups all empty")
        # the CPU oracle gives 0.68 (0.09 .. 1.00 per block): if this fails the inputs no longer exercise both paths
        assert 0.10 <= share <= 0.90, share
    finally:
        ctx.close()


@pytest.mark.parametrize("n_side,sc,sf", [((37, 1), 8, 16), ((3, 1), 2, 3)])
def test_ragged_shapes(n_side, sc, sf):
    """37 rays x (8+16): M = 888 is no multiple of 128, S none of 32, the last group has invalid lanes; 3 rays x (2+3)."""
    ctx = _bench_context()
    try:
        h, w = n_side
        _identity(ctx, C2W, bench.FOV, h, w, sc, sf, f"{h * w} rays x ({sc}+{sf})")
    finally:
        ctx.close()


def test_all_empty_and_none_empty():
    import nerf_and_dietnerf_amd as N
    fine = N.glorot_blob(1)
    for bias, label in ((-50.0, "sigma bias -50"), (1.5, "sigma bias +1.5")):
        blob = fine.copy()
        blob[-1] = bias                                    # the sigma head's bias: the blob's last element
        ctx = _bench_context(blob_f=blob)
        try:
            six, skipped = _identity(ctx, C2W, bench.FOV, 24, 24, 32, 48, label)
            if bias < 0:
                assert _empty_groups(six[3]).all() and not np.asarray(six[0]).any(), label      # rgb exactly 0 everywhere
                assert skipped == 24 * 24 * 80 // 128, (label, skipped)
            else:
                assert not _empty_groups(six[3]).any() and skipped == 0, (label, skipped)
        finally:
            ctx.close()


def test_shipped_checkpoint(golden_ckpt):
    """24 x 24, 32+48: groups with single empty waves and no empty group."""
    g = golden_ckpt
    ctx = _bench_context(g["blob_coarse"], g["blob_fine"], float(g["near"]), float(g["far"]))
    try:
        _identity(ctx, g["c2w_test"], float(g["fov"]), 24, 24, 32, 48, "shipped checkpoint")
    finally:
        ctx.close()


def test_per_sample_rgb_is_never_skipped():
    """A caller that asks for rgb_samples gets every sample's colour, also where alpha is 0: the six-output run's rgb_samples
    on such rows are sigmoid(model_predict's rgb) within 1e-4 (the f16x3 mode's bar on colours), not a skipped row's 0.5."""
    ctx = _bench_context()
    try:
        h = w = 16
        six = ctx.render_image(C2W, bench.FOV, h, w, 0, SC, SF, seed=2)
        alpha, rgb_s, z = (np.asarray(six[i], np.float32) for i in (3, 4, 5))
        d = np.asarray(ctx.get_rays_directions(h, w, bench.FOV, C2W), np.float32).reshape(-1, 4)
        o = C2W[:3, 3].astype(np.float32)
        zz = z.reshape(h * w, -1)
        rows = np.argwhere(alpha.reshape(h * w, -1) == 0)
        assert rows.shape[0] > 1000, rows.shape
        rows = rows[:: max(1, rows.shape[0] // 4096)]
        ray, s = rows[:, 0], rows[:, 1]
        xyz = o[None, :] + d[ray, :3] * zz[ray, s][:, None]
        raw = np.asarray(ctx.model_predict(1, xyz.astype(np.float32), d[ray, :3].copy()), np.float32)
        want = 1.0 / (1.0 + np.exp(-raw[:, :3].astype(np.float64)))
        got = rgb_s.reshape(h * w, -1, 3)[ray, s]
        err = float(np.abs(got - want).max())
        print(f"rgb_samples on alpha == 0 rows vs sigmoid(model_predict): max-abs {err:.3e}")
        assert err <= 1e-4, err
        assert float(np.abs(got - 0.5).max()) > 1e-3
    finally:
        ctx.close()


def test_nonfinite_sigma_is_counted(golden_ckpt, golden_vec):
    """test_nonfinite_watch's network (layer 1 scaled beyond the fp16 range) and rays through renders that read rgb alone: a
    render_rays call (one launch of the rgb-skipping kernel), then a whole rgb_only frame."""
    g = golden_ckpt
    big = g["blob_coarse"].copy()
    big[33 * 256 + 256: 33 * 256 + 256 + 256 * 256] *= 3e4        # layer-1 kernel: activations ~1e5 > 65504
    ctx = _bench_context(big, big, float(g["near"]), float(g["far"]))
    try:
        S.render_rays(ctx, 0, golden_vec["rays_orig"], golden_vec["rays_dirs"], golden_vec["z_coarse"], ("rgb",))
        assert ctx.read_nonfinite() > 0
        ctx.render_image(g["c2w_test"], float(g["fov"]), 8, 8, 0, 16, 16, seed=1, rgb_only=True)
        assert ctx.read_nonfinite() > 0
    finally:
        ctx.close()


def test_culled_launch():
    """The mode-1 launch under sample culling (tools/culling_measure.py's synthetic grid), a small frame."""
    ctx = _bench_context()
    try:
        lo, hi = (-0.4, -0.4, -0.4), (0.4, 0.4, 0.4)
        grid = G.two_balls(128, np.array(lo, np.float32) * 2.5, np.array(hi, np.float32) * 2.5) | \
            (np.random.default_rng(1).random((128, 128, 128)) < 0.02)
        ctx.set_scene_box(lo, hi)
        ctx.set_occupancy_grid(grid)
        ctx.set_sample_culling(True)
        ctx.read_culling()
        _identity(ctx, C2W, bench.FOV, 48, 48, SC, SF, "culled 48x48", tiles=-1)      # the kept rows' tiles: some
        samples, kept = ctx.read_culling()
        assert 0 < kept < samples, (samples, kept)
    finally:
        ctx.close()


def test_gate_falls_back_to_the_full_kernel_and_probes_again():
    """A network that skips nothing (sigma bias +1.5) pays the vote once: when the first launch's counters have reached the
    host, the next launches run the full kernel (the rgb-skipping kernel's tile count stands still), with the same bits; new
    weights reset the gate.  A network that skips (Glorot) stays on the rgb-skipping kernel."""
    import nerf_and_dietnerf_amd as N
    blob = N.glorot_blob(1)
    blob[-1] = 1.5
    ctx = _bench_context(blob_f=blob)
    try:
        tiles = 24 * 24 * 80 // 128

        def frame():
            return ctx.render_image(C2W, bench.FOV, 24, 24, 0, 32, 48, seed=2, rgb_only=True)[0]

        first = frame()
        assert _counts(ctx)[:2] == (tiles, 0)                      # ... and the read drains the stream: the copy has landed
        for _ in range(3):
            S.assert_same_bits(frame(), first, "full kernel behind the gate")
        ran, skipped, full_left = _counts(ctx)
        assert (ran, skipped) == (tiles, 0) and full_left == 63 - 3, (ran, skipped, full_left)
        ctx.load_weights(1, N.glorot_blob(1))                      # new weights: the gate forgets
        for k in range(12):
            frame()
        ran, skipped, full_left = _counts(ctx)
        assert ran == tiles * 13 and skipped > 0 and full_left == 0, (ran, skipped, full_left)
    finally:
        ctx.close()
