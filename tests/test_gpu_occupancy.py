"""The occupancy grid on the device: the walk (nerf_ray_occupancy_bounds) and the depths drawn on it, bit for bit against the
float32 restatement of tests/occupancy_ref.py; the host-to-device round trip of the bits; baking against the public point
query (Context.model_predict) and the numpy oracle; and the layers that draw depths for rays -- render, train_gradients under
both policies, render_image -- against the same calls on substituted draws.  Every test here needs the entry points the grid
adds to the ABI."""
import numpy as np
import pytest

import grad_blocks as GB
import occupancy_ref as G
import sampling_space_ref as R
import scene_box_ref as B
import support as S

pytestmark = pytest.mark.gpu

NEAR, FAR = G.NEAR, G.FAR
NO_GRID = "no occupancy grid"
NEEDS_BOX = "an occupancy grid needs a scene box"


@pytest.fixture(scope="module")
def ctx():
    import nerf_and_dietnerf_amd as N
    c = N.Context(near=NEAR, far=FAR, precision="fp32")
    yield c
    c.close()


@pytest.fixture(scope="module")
def world(ctx):
    """The six hand rays, then 4167 rays of the issue's recipe: 4173 in all."""
    return G.world_scene(4173)


@pytest.fixture(scope="module")
def ndc(ctx):
    """A 65 x 65 image of a forward-facing camera through rays_to_ndc: 4225 NDC rays, bounds 0 and 1."""
    return G.ndc_scene(ctx)


# ---- 1. the walk -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4173])
@pytest.mark.parametrize("r", [4, 8, 16])
@pytest.mark.parametrize("space", ["world", "ndc"])
def test_bounds_equal_the_restatement(ctx, world, ndc, space, r, n):
    o, d, lo, hi, near, far = world if space == "world" else ndc
    o, d = o[:n], d[:n]
    grid = G.grid_for(r, lo, hi)
    G.arm(ctx, lo, hi, near, far, grid)
    want_bounds, want_state = G.ray_occupancy_bounds(o, d, lo, hi, near, far, grid)
    bounds, state = ctx.ray_occupancy_bounds(o, d)
    assert state.dtype == np.int32 and bounds.dtype == np.float32 and bounds.shape == (n, 2)
    np.testing.assert_array_equal(state, want_state)
    np.testing.assert_array_equal(bounds.view(np.uint32), want_bounds.view(np.uint32))
    if n == 4173:
        counts = np.bincount(want_state, minlength=3)
        assert counts[2] >= n // 20 and counts[0] + counts[1] >= n // 20, counts       # the input shows narrowed rays and others
    if n == 65:                                                                        # device memory == host memory
        import torch
        bt, st = ctx.ray_occupancy_bounds(torch.as_tensor(o).cuda(), torch.as_tensor(d).cuda())
        assert bt.is_cuda and st.is_cuda and st.dtype == torch.int32
        np.testing.assert_array_equal(bt.cpu().numpy(), bounds)
        np.testing.assert_array_equal(st.cpu().numpy(), state)


def test_hand_cases_on_the_device(ctx):
    """The hand cases of tests/test_occupancy_host.py (R = 4, planes exact in float32): a single cell, a ray along a cell face,
    the diagonal through cell corners (tie rule), zero direction components, an origin inside the grid, empty and full grids."""
    o, d = G.hand_rays()
    names = [r[2] for r in G.HAND_RAYS]
    cells = [[(2, 2, 1)], [(2, 2, 3), (2, 2, 1)], [(2, 3, 2)], [(3, 2, 2)], [(2, 2, 2)], [(1, 0, 2)], [(0, 1, 2)], [(1, 1, 2)],
             [(1, 0, 2), (1, 1, 2)], [(0, 0, 2), (2, 2, 2)], [(2, 2, 0)], [(2, 2, 0), (2, 2, 1)], []]
    grids = []
    for cs in cells:
        g = np.zeros((4, 4, 4), bool)
        for c in cs:
            g[c] = True
        grids.append(g)
    grids.append(np.ones((4, 4, 4), bool))
    for g in grids:
        G.arm(ctx, G.LO, G.HI, NEAR, FAR, g)
        want_bounds, want_state = G.ray_occupancy_bounds(o, d, G.LO, G.HI, NEAR, FAR, g)
        bounds, state = ctx.ray_occupancy_bounds(o, d)
        np.testing.assert_array_equal(state, want_state)
        np.testing.assert_array_equal(bounds.view(np.uint32), want_bounds.view(np.uint32))
    # and three of them by their numbers
    def get(name):
        bounds, state = ctx.ray_occupancy_bounds(o, d)
        return tuple(bounds[names.index(name)].tolist()), int(state[names.index(name)])
    G.arm(ctx, G.LO, G.HI, NEAR, FAR, grids[0])
    assert get("through_cell_centres") == ((4.0, 4.5), 2)
    G.arm(ctx, G.LO, G.HI, NEAR, FAR, grids[7])
    assert get("through_cell_corners") == ((2.5, 3.0), 2)
    G.arm(ctx, G.LO, G.HI, NEAR, FAR, grids[5])
    assert get("through_cell_corners") == ((2.0, 4.0), 1)                 # (1, 0) is touched in a point: the box alone


# ---- 2. the depths -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2, 55])
@pytest.mark.parametrize("lindisp", [False, True])
def test_depths_equal_the_restatement(ctx, world, oracle, lindisp, s):
    """get_z_values_for_rays under a grid, explicit draws (0 and the float below 1 among them) and on-device draws: bit-equal to
    the restatement; rays of state 0 or 1 bit-equal to the same context with the grid cleared; a full grid is the box alone."""
    o, d, lo, hi, near, far = world
    n = 521
    o, d = o[:n], d[:n]
    grid = G.grid_for(16, lo, hi)
    _, state = G.ray_occupancy_bounds(o, d, lo, hi, near, far, grid)
    assert (state == 2).sum() >= n // 20 and (state == 1).sum() >= n // 20 and (state == 0).sum() >= n // 20
    u = np.random.default_rng(7 + s).random((n, s), dtype=np.float32)
    u[0], u[-1] = 0.0, R.U_BELOW_ONE
    u[np.nonzero(state == 2)[0][:2]] = np.array([[0.0], [R.U_BELOW_ONE]], np.float32)
    up = oracle.philox_uniform(9, np.arange(n, dtype=np.uint64), s, 0)
    G.arm(ctx, lo, hi, near, far, grid)
    if lindisp:
        ctx.set_sampling("lindisp")
    z = ctx.get_z_values_for_rays(o, d, s, uniform_values=u)
    zp = ctx.get_z_values_for_rays(o, d, s, seed=9)
    np.testing.assert_array_equal(z.view(np.uint32), G.z_values(o, d, lo, hi, near, far, grid, u, lindisp).view(np.uint32))
    np.testing.assert_array_equal(zp.view(np.uint32), G.z_values(o, d, lo, hi, near, far, grid, up, lindisp).view(np.uint32))
    np.testing.assert_array_equal(ctx.get_z_values_for_rays(o[31:51], d[31:51], s, seed=9, ray_base=31), zp[31:51])
    assert np.all(np.diff(z, axis=1) >= 0)
    ctx.set_occupancy_grid(None)                                       # the box alone
    assert ctx.occupancy_grid() is None
    z_box, zp_box = ctx.get_z_values_for_rays(o, d, s, uniform_values=u), ctx.get_z_values_for_rays(o, d, s, seed=9)
    np.testing.assert_array_equal(z_box.view(np.uint32), B.z_values(o, d, lo, hi, near, far, u, lindisp).view(np.uint32))
    rest = state != 2
    np.testing.assert_array_equal(z[rest].view(np.uint32), z_box[rest].view(np.uint32))
    np.testing.assert_array_equal(zp[rest].view(np.uint32), zp_box[rest].view(np.uint32))
    assert not np.array_equal(z[state == 2], z_box[state == 2])         # and the grid did act
    ctx.set_occupancy_grid(np.ones((16, 16, 16), bool))
    np.testing.assert_array_equal(ctx.get_z_values_for_rays(o, d, s, uniform_values=u).view(np.uint32), z_box.view(np.uint32))
    np.testing.assert_array_equal(ctx.get_z_values_for_rays(o, d, s, seed=9).view(np.uint32), zp_box.view(np.uint32))
    ctx.set_sampling("linear")


# ---- 3. the bits: host -> device -> host, and what drops or refuses a grid ----------------------------------------------------
def test_round_trip_and_refusals(ctx, world):
    import nerf_and_dietnerf_amd as N
    o, d = world[0][:8], world[1][:8]
    G.arm(ctx, G.LO, G.HI, NEAR, FAR, None)
    assert ctx.occupancy_grid() is None
    with pytest.raises(RuntimeError, match=NO_GRID):
        ctx.ray_occupancy_bounds(o, d)
    for r in (4, 12, 64, 256):
        grid = np.random.default_rng(r).random((r, r, r)) < 0.3
        ctx.set_occupancy_grid(grid)
        back = ctx.occupancy_grid()
        assert back.dtype == bool and back.shape == (r, r, r) and ctx.grid_resolution == r
        np.testing.assert_array_equal(back, grid)
    ctx.set_occupancy_grid(G.pack_bits(grid[:8, :8, :8]))              # packed words
    np.testing.assert_array_equal(ctx.occupancy_grid(), grid[:8, :8, :8])
    ctx.set_scene_box(G.LO, G.HI)                                      # setting the box, even to the same corners, drops the grid
    assert ctx.occupancy_grid() is None and ctx.grid_resolution == 0
    ctx.set_occupancy_grid(grid[:8, :8, :8])
    ctx.set_scene_box(None)
    assert ctx.occupancy_grid() is None
    # the library's own refusals
    words = G.pack_bits(grid[:8, :8, :8])
    count = np.zeros(1, np.int64)
    assert ctx.lib.nerf_ctx_set_occupancy_grid(ctx.h, words.ctypes.data, 8) != 0 and NEEDS_BOX in N._lib.last_error()
    assert ctx.lib.nerf_occupancy_bake(ctx.h, 0, 16, 1.0, 1, 0, 0, count.ctypes.data) != 0 and NEEDS_BOX in N._lib.last_error()
    ctx.set_scene_box(G.LO, G.HI)
    for r in (0, 6, 260):
        assert ctx.lib.nerf_ctx_set_occupancy_grid(ctx.h, words.ctypes.data, r) != 0 and "multiple of 4" in N._lib.last_error()
    assert ctx.lib.nerf_occupancy_bake(ctx.h, 0, 18, 1.0, 1, 0, 0, count.ctypes.data) != 0 and "multiple of 4" in N._lib.last_error()
    for thr in (0.0, -1.0, float("nan"), float("inf")):
        assert ctx.lib.nerf_occupancy_bake(ctx.h, 0, 16, thr, 1, 0, 0, count.ctypes.data) != 0
        assert "sigma_threshold must be finite and > 0" in N._lib.last_error()
    for spc in (0, 9):
        assert ctx.lib.nerf_occupancy_bake(ctx.h, 0, 16, 1.0, spc, 0, 0, count.ctypes.data) != 0
        assert "samples_per_cell must be in 1..8" in N._lib.last_error()
    with pytest.raises(RuntimeError, match="no weights loaded"):       # this context never loaded a network
        ctx.bake_occupancy_grid(0, 16, 1.0)
    assert ctx.occupancy_grid() is None


# ---- 4. baking ---------------------------------------------------------------------------------------------------------------
BAND = 1e-3


@pytest.fixture(scope="module")
def bake_ref(oracle, golden_ckpt):
    """The 4096 float32 centres of a 16^3 grid over G.GOLDEN_BOX in bit order, the numpy oracle's sigma of the fine network there,
    and a threshold chosen on the CPU: the first candidate that leaves fewer than 1 % of the cells inside the band
    |sigma - thr| <= 1e-3 max(1, thr) and marks between 2 % and 50 % of them."""
    centres = G.centres_in_bit_order(*G.GOLDEN_BOX, 16)
    view = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (centres.shape[0], 1))
    sigma = oracle.model_predict(oracle.unpack_blob(golden_ckpt["blob_fine"]), centres, view)[:, 3]
    for thr in (10.0, 20.0, 5.0, 40.0, 2.5):
        band = np.abs(sigma - thr) <= BAND * max(1.0, thr)
        if band.mean() < 0.01 and 0.02 < (sigma > thr).mean() < 0.5:
            return centres, view, sigma, thr, band
    raise AssertionError("no candidate threshold leaves fewer than 1 % of the cells inside the band")


def _golden_ctx(golden_ckpt, precision, box=G.GOLDEN_BOX):
    import nerf_and_dietnerf_amd as N
    c = N.Context(near=float(golden_ckpt["near"]), far=float(golden_ckpt["far"]), precision=precision)
    c.load_weights(0, golden_ckpt["blob_coarse"])
    c.load_weights(1, golden_ckpt["blob_fine"])
    if box is not None:
        c.set_scene_box(*box)
    return c


def _bit_order(grid):
    return grid.transpose(2, 1, 0).ravel()


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_bake_against_the_point_query(golden_ckpt, bake_ref, precision, capsys):
    centres, view, sigma, thr, band = bake_ref
    assert band.mean() < 0.01
    c = _golden_ctx(golden_ckpt, precision)
    count = c.bake_occupancy_grid(1, 16, thr, samples_per_cell=1, dilate=0)
    grid = c.occupancy_grid()
    assert grid.shape == (16, 16, 16) and count == int(grid.sum()) and 0 < count < 4096
    # the same kernel on the same float32 centres: exactly its verdict
    raw = c.model_predict(1, centres, view)
    np.testing.assert_array_equal(_bit_order(grid), raw[:, 3] > np.float32(thr))
    # the numpy oracle, outside the band
    clear = ~band
    np.testing.assert_array_equal(_bit_order(grid)[clear], (sigma > thr)[clear])
    with capsys.disabled():
        print(f"\n[bake, {precision}] thr {thr:g}: {count} of 4096 cells occupied, {int(band.sum())} inside the band; "
              f"max |sigma - oracle| {np.abs(raw[:, 3] - sigma).max():.2e}", end="")
    # dilation against numpy
    for steps in (1, 2):
        n_dilated = c.bake_occupancy_grid(1, 16, thr, samples_per_cell=1, dilate=steps)
        want = grid
        for _ in range(steps):
            want = G.dilate26(want)
        got = c.occupancy_grid()
        np.testing.assert_array_equal(got, want)
        assert n_dilated == int(want.sum()) > count
    # more points per cell can only add cells; the jitter is a function of the seed
    n4 = c.bake_occupancy_grid(1, 16, thr, samples_per_cell=4, dilate=0, seed=3)
    g4 = c.occupancy_grid()
    assert np.all(g4[grid]) and n4 == int(g4.sum()) >= count
    c.bake_occupancy_grid(1, 16, thr, samples_per_cell=4, dilate=0, seed=3)
    np.testing.assert_array_equal(c.occupancy_grid(), g4)
    # the coarse network is another network
    c.bake_occupancy_grid(0, 16, thr, samples_per_cell=1, dilate=0)
    raw_c = c.model_predict(0, centres, view)
    np.testing.assert_array_equal(_bit_order(c.occupancy_grid()), raw_c[:, 3] > np.float32(thr))
    c.close()


def test_bake_in_chunks(golden_ckpt):
    """R = 128 at one point per cell is two chunks of 2^20 points, R = 64 at 5 points per cell a chunk of 209664 cells and a
    shorter one: the centre verdicts of runs of cells (the first, across the chunk seam, the last) equal the point query's, and
    the count is the sum of the bits."""
    c = _golden_ctx(golden_ckpt, "f16x3")
    for r, spc in ((128, 1), (64, 5)):
        count = c.bake_occupancy_grid(1, r, 10.0, samples_per_cell=spc, dilate=0)
        grid = c.occupancy_grid()
        assert count == int(grid.sum()) and 0 < count < r ** 3
        if spc == 1:
            centres = G.centres_in_bit_order(*G.GOLDEN_BOX, r)
            for begin in (0, (1 << 20) - 2048, r ** 3 - 4096):         # the grid's first cells, across the chunk seam, its last cells
                x = np.ascontiguousarray(centres[begin:begin + 4096])
                raw = c.model_predict(1, x, np.tile(np.array([0.0, 0.0, 1.0], np.float32), (4096, 1)))
                np.testing.assert_array_equal(_bit_order(grid)[begin:begin + 4096], raw[:, 3] > np.float32(10.0))
    c.close()


def test_render_config_bakes_on_request(golden_ckpt):
    import nerf_and_dietnerf_amd as N
    net = {"hidden_layer_dim": 256, "last_hidden_layer_dim": 128, "leaky_relu_alpha": 0.05, "n_pos_enc_dim_xyz": 5,
           "n_pos_enc_view_dir": 4, "n_angles_for_model": 2}
    rc = {"n_render_samples_coarse": 8, "n_render_samples_fine": 16, "scene_box": [list(G.GOLDEN_BOX[0]), list(G.GOLDEN_BOX[1])],
          "occupancy_grid": {"resolution": 16, "sigma_threshold": 10.0, "dilate": 0}}
    m = N.NeRF(net, rc, float(golden_ckpt["near"]), float(golden_ckpt["far"]), precision="fp32")
    m.set_weights(golden_ckpt["blob_coarse"], golden_ckpt["blob_fine"])
    assert m.ctx.occupancy_grid() is None                              # set_weights does not bake
    count = m.update_occupancy_grid()
    fine = m.ctx.occupancy_grid()
    assert count == int(fine.sum()) > 0
    direct = _golden_ctx(golden_ckpt, "fp32")
    assert direct.bake_occupancy_grid(1, 16, 10.0, 1, 0) == count      # the fine network, since it is loaded
    np.testing.assert_array_equal(direct.occupancy_grid(), fine)
    m.ctx.close()
    direct.close()


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------
SIZES = [(130, 8, 16), (521, 16, 24)]


@pytest.fixture(scope="module")
def golden_scene(oracle, golden_ckpt, bake_ref):
    """Rays of the golden training camera (the last ten turned round, so that they miss the box), the grid the oracle's sigma
    gives at the chosen threshold, and the restatement's verdict."""
    _, _, sigma, thr, _ = bake_ref
    grid = np.ascontiguousarray((sigma > thr).reshape(16, 16, 16).transpose(2, 1, 0))
    near, far = float(golden_ckpt["near"]), float(golden_ckpt["far"])
    out = {}
    for n, (h, w) in ((130, (12, 11)), (521, (23, 23))):
        o, d = R.world_rays(oracle, golden_ckpt["c2w_train"], float(golden_ckpt["fov"]), h, w)
        o, d = np.ascontiguousarray(o[:n]), np.ascontiguousarray(d[:n])
        d[-10:, :3] *= -1.0
        _, state = G.ray_occupancy_bounds(o, d, *G.GOLDEN_BOX, near, far, grid)
        assert (state == 2).sum() >= n // 4 and (state == 1).sum() >= n // 20 and (state == 0).sum() >= 10, np.bincount(state)
        out[n] = (o, d, state)
    return grid, near, far, out


def _substituted(oracle, z, near, far):
    """Draws that put a context without box or grid on the depths z, up to rounding (draws outside [0, 1) are fine when they
    are explicit): u' = (z - linspace(near, far, S)[s]) S / (far - near)."""
    s = z.shape[1]
    return ((z.astype(np.float64) - oracle.linspace_f32(near, far, s)[None, :]) * s / (far - near)).astype(np.float32)


@pytest.mark.parametrize("n,sc,sf", SIZES)
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_render_follows_the_grid(oracle, golden_ckpt, golden_scene, precision, n, sc, sf, capsys):
    """render under box + grid against render of a context with neither on substituted draws that reproduce the restatement's
    coarse depths, and against render_rays on exactly those depths: RGB within 1e-4, the project's parity bar (measured on an
    MI355X: at most 6.4e-6)."""
    grid, near, far, rays = golden_scene
    o, d, state = rays[n]
    rng = np.random.default_rng(n)
    u_c, u_f = rng.random((n, sc), dtype=np.float32), rng.random((n, sf), dtype=np.float32)
    z_ref = G.z_values(o, d, *G.GOLDEN_BOX, near, far, grid, u_c)
    c = _golden_ctx(golden_ckpt, precision)
    c.set_occupancy_grid(grid)
    out = c.render(o, d, sc, sf, u_c, u_f)
    z_dev = c.get_z_values_for_rays(o, d, sc, uniform_values=u_c)
    np.testing.assert_array_equal(z_dev.view(np.uint32), z_ref.view(np.uint32))
    coarse_only = c.render_rays(0, o, d, z_ref)[0]                        # the coarse network on the restatement's depths
    c.set_occupancy_grid(None)
    box_only = c.render(o, d, sc, sf, u_c, u_f)
    c.close()
    plain = _golden_ctx(golden_ckpt, precision, box=None)
    u_sub = _substituted(oracle, z_ref, near, far)
    z_sub = plain.get_z_values_for_rays(o, d, sc, uniform_values=u_sub)
    assert np.abs(z_sub - z_ref).max() <= 4 * B.U * far                   # the same depths, to rounding
    want = plain.render(o, d, sc, sf, u_sub, u_f)
    want_coarse = plain.render(o, d, sc, 0, u_sub, None)[0]
    plain.close()
    err = float(np.abs(out[0] - want[0]).max())
    err_c = float(np.abs(coarse_only - want_coarse).max())
    with capsys.disabled():
        print(f"\n[{precision}, {n} x ({sc}+{sf})] grid vs substituted draws: max-abs RGB {err:.2e} (coarse alone {err_c:.2e}); "
              f"grid vs box only {np.abs(out[0] - box_only[0]).max():.2e}; states {np.bincount(state, minlength=3).tolist()}", end="")
    assert np.isfinite(out[0]).all() and err <= 1e-4 and err_c <= 1e-4
    rest = state != 2
    np.testing.assert_array_equal(out[0][rest], box_only[0][rest])         # rays the grid leaves alone: the box-only render
    assert not np.array_equal(out[5][state == 2], box_only[5][state == 2])


@pytest.mark.parametrize("n,sc,sf", SIZES)
@pytest.mark.parametrize("policy", ["float32", "mixed_float16"])
def test_train_gradients_follow_the_grid(oracle, golden_ckpt, golden_scene, policy, n, sc, sf, capsys):
    """One train_gradients call under box + grid against the same call without either on substituted draws.  Blob-wide, the
    bars the scene box's training test holds the same comparison to (tests/test_gpu_scene_box.py): loss within 2e-6 relative
    (2e-3 under mixed_float16), both blobs within 5e-2 of max|g|, cosine > 0.999.  Block by block (tests/grad_blocks.py: every
    kernel, bias and row group against ITS OWN max; blocks under the module's floor absolutely, at most two of them):
      float32        5 x FP32_BAR = 1e-3.  FP32_BAR (2e-4) is what one float32 gradient is held to against the exact gradient at
                     its depths; here two float32 gradients are compared, each with that error of its own (2 x), at depths that
                     differ by up to 4 * 2^-24 * far = 6e-7 -- about 1.5e-4 of a stratum where the grid leaves a ray one cell
                     (0.06 / 16 strata), and alpha = 1 - exp(-sigma dz) moves relatively by as much: one more FP32_BAR, the
                     rest is room for blocks that are sums with cancellation.
      mixed_float16  MIXED_LEAST = 2e-2, the module's least bar for that policy: fp16 roundings flip under the depth change.
    No block is named for a blob-relative bar.  Measured on an MI355X: gradients within 9.0e-5 (float32) and 6.7e-4
    (mixed_float16) of max|g|; the worst block within 1.8e-4 / 2.4e-3 of its own max."""
    grid, near, far, rays = golden_scene
    o, d, state = rays[n]
    rng = np.random.default_rng(n + 1)
    u_c, u_f = rng.random((n, sc), dtype=np.float32), rng.random((n, sf), dtype=np.float32)
    tgt = rng.random((n, 3), dtype=np.float32)
    mixed = policy == "mixed_float16"
    z_ref = G.z_values(o, d, *G.GOLDEN_BOX, near, far, grid, u_c)
    res = {}
    for mode in ("grid", "substituted", "box"):
        c = _golden_ctx(golden_ckpt, "fp32", box=None if mode == "substituted" else G.GOLDEN_BOX)
        if mode == "grid":
            c.set_occupancy_grid(grid)
        u = _substituted(oracle, z_ref, near, far) if mode == "substituted" else u_c
        c.train_begin(5e-4, mixed_float16=mixed)
        res[mode] = c.train_gradients(o, d, tgt, sc, sf, u, u_f)
        c.train_end()
        c.close()
    (m0, gc0, gf0), (m1, gc1, gf1), (m2, _, _) = res["grid"], res["substituted"], res["box"]
    blks = GB.blocks(5, 4, 2)
    with capsys.disabled():
        print(f"\n[{policy}, {n} x ({sc}+{sf})] grid vs substituted draws: loss {m0['loss']:.7f} / {m1['loss']:.7f} (box only: "
              f"{m2['loss']:.7f}), gradients {S.relerr(gc0, gc1):.2e} (coarse), {S.relerr(gf0, gf1):.2e} (fine) of max|g|; "
              f"coarse {GB.summary(GB.block_errors(gc0, gc1, blks))}; fine {GB.summary(GB.block_errors(gf0, gf1, blks))}", end="")
    assert np.isfinite(gc0).all() and np.isfinite(gf0).all()
    assert abs(m0["loss"] - m1["loss"]) <= (2e-3 if mixed else 2e-6) * m1["loss"]
    assert S.relerr(gc0, gc1) <= 5e-2 and S.cos(gc0, gc1) > 0.999
    assert S.relerr(gf0, gf1) <= 5e-2 and S.cos(gf0, gf1) > 0.999
    bar = GB.MIXED_LEAST if mixed else 5 * GB.FP32_BAR
    GB.assert_blocks(gc0, gc1, blks, bar, "max", "coarse")
    GB.assert_blocks(gf0, gf1, blks, bar, "max", "fine")
    assert abs(m2["loss"] - m0["loss"]) > 1e-4 * m0["loss"]                 # and the grid matters


def test_render_image_is_slab_and_batch_invariant_with_a_grid(golden_ckpt, golden_scene):
    """render_image under box + grid: the whole image at two batch sizes and a slab of it are bit-identical, and equal render on
    the image's own rays."""
    grid, near, far, _ = golden_scene
    (h, w), sc, sf, seed = (16, 24), 16, 24, 5
    c2w, fov = golden_ckpt["c2w_train"], float(golden_ckpt["fov"])
    c = _golden_ctx(golden_ckpt, "fp32")
    c.set_occupancy_grid(grid)
    dirs = c.get_rays_directions(h, w, fov, c2w).reshape(-1, 4)
    orig = np.tile(np.asarray(c2w, np.float32)[:, 3], (h * w, 1))
    _, state = c.ray_occupancy_bounds(orig, dirs)
    assert (state == 2).sum() >= h * w // 4 and (state != 2).sum() >= h * w // 20
    want = c.render(orig, dirs, sc, sf, seed=seed, want_depth=True)
    for batch in (0, 100):
        got = c.render_image(c2w, fov, h, w, batch, sc, sf, seed=seed, want_depth=True)
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a.reshape(b.shape), b)
    begin, count = 37, 101
    got = c.render_image(c2w, fov, h, w, 64, sc, sf, seed=seed, ray_begin=begin, ray_count=count, want_depth=True)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b[begin:begin + count])
    c.set_occupancy_grid(None)
    assert not np.array_equal(c.render_image(c2w, fov, h, w, 0, sc, sf, seed=seed)[5].reshape(want[5].shape), want[5])
    c.close()
