"""The occupancy grid without a GPU: the float32 restatement of the ray rule (tests/occupancy_ref.py) against the same walk
in float64 and against brute force, the rule's hand cases, the bit packing, the Python layer's refusals and the hooks in
NeRF.load_weights and dataset.fit.  The walk tests and hand cases exercise the restatement alone (the float64 walk is their
reference), so they do not depend on the library: what ties the library's walk to this restatement is
tests/test_gpu_occupancy.py, which holds the device to it bit for bit.  The packing, refusal, config and hook tests call the
package's new code."""
import numpy as np
import pytest

import occupancy_ref as G
import scene_box_ref as B
import support as S

NEAR, FAR = G.NEAR, G.FAR
NEEDS_BOX = "an occupancy grid needs a scene box"
BAD_R = "multiple of 4 in \\[4, 256\\]"


@pytest.fixture(scope="module")
def scene():
    """The issue's input: the two-ball 16^3 grid in [-1, 1]^3 and 4096 seeded rays from the radius-4 sphere aimed at points of
    [-1.2, 1.2]^3; walked once in float32 and once in float64."""
    grid = G.two_balls(16)
    o, d = G.sphere_rays(4096, seed=11)
    w32 = G.ray_grid_interval(o, d, G.LO, G.HI, NEAR, FAR, grid, G.F32)
    w64 = G.ray_grid_interval(o, d, G.LO, G.HI, NEAR, FAR, grid, G.F64)
    return grid, o, d, w32, w64


def test_the_box_steps_are_the_scene_box_rule():
    o, d = B.recipe_rays()
    a, b, hit, narrowed = G.box_interval(o, d, B.LO, B.HI, B.NEAR, B.FAR, G.F32)
    wa, wb, whit, wnar = B.ray_box_interval(o, d, B.LO, B.HI, B.NEAR, B.FAR)
    np.testing.assert_array_equal(a.view(np.uint32), wa.view(np.uint32))
    np.testing.assert_array_equal(b.view(np.uint32), wb.view(np.uint32))
    np.testing.assert_array_equal(hit, whit)
    np.testing.assert_array_equal(narrowed, wnar)


def test_float32_walk_against_the_float64_walk(scene, capsys):
    """Bar 4e-6 on a and b (8 x the 4.8e-7 measured when the rule was written; depths are <= 6); at most 0.5 % of the rays may
    be set aside for changing kind (missed / no occupied cell / narrowed) between the two walks."""
    grid, o, d, (a32, b32, s32, h32), (a64, b64, s64, h64) = scene
    assert 100 < grid.sum() < grid.size // 4
    k32, k64 = G.kind(s32, h32), G.kind(s64, h64)
    assert all((k64 == k).mean() >= 0.05 for k in (0, 1, 2))            # the input shows all three kinds
    changed = k32 != k64
    keep = ~changed
    ea, eb = np.abs(a32[keep] - a64[keep]).max(), np.abs(b32[keep] - b64[keep]).max()
    with capsys.disabled():
        print(f"\n[occupancy, float32 vs float64 walk] {int(changed.sum())} of 4096 rays change kind; max |da| {ea:.2e}, "
              f"max |db| {eb:.2e} (bar 4e-6); kinds {np.bincount(k64, minlength=3).tolist()}", end="")
    assert changed.sum() <= 0.005 * 4096
    assert ea <= 4e-6 and eb <= 4e-6
    # the states of the rays that kept their kind: 1 or 0 by the box alone, the same in both
    np.testing.assert_array_equal(s32[keep], s64[keep])


def test_no_occupied_point_lies_outside_a_narrowed_interval(scene):
    """Soundness against brute force: 2000 float64 points along [a0, b0] of every narrowed ray; none whose cell is occupied lies
    outside [a - 1e-5, b + 1e-5]."""
    grid, o, d, (a, b, state, hit), _ = scene
    a0, b0, _, _ = G.box_interval(o, d, G.LO, G.HI, NEAR, FAR, G.F64)
    sel = state == 2
    assert sel.sum() > 400
    o64, d64 = o[sel, :3].astype(np.float64), d[sel, :3].astype(np.float64)
    t = a0[sel, None] + (b0[sel] - a0[sel])[:, None] * np.linspace(0.0, 1.0, 2000)[None, :]
    p = o64[:, None, :] + t[:, :, None] * d64[:, None, :]
    r = grid.shape[0]
    cell = (G.HI.astype(np.float64) - G.LO) / r
    idx = np.floor((p - G.LO.astype(np.float64)) / cell).astype(np.int64)
    inside = ((idx >= 0) & (idx < r)).all(axis=-1)
    idx = np.clip(idx, 0, r - 1)
    occupied = inside & grid[idx[..., 0], idx[..., 1], idx[..., 2]]
    outside = (t < a[sel, None].astype(np.float64) - 1e-5) | (t > b[sel, None].astype(np.float64) + 1e-5)
    assert occupied.any(axis=1).mean() > 0.9                  # the brute force does see the occupied cells
    assert not (occupied & outside).any()
    # and a narrowed interval lies inside the ray's box interval
    assert np.all(a[sel] >= a0[sel] - 1e-6) and np.all(b[sel] <= b0[sel] + 1e-6) and np.all(b[sel] > a[sel])


# ---- hand cases: the box [-1, 1]^3 at R = 4 (cells of 0.5, all planes exact in float32), near 2, far 6 ------------------------------
def _walk(grid, names=None):
    o, d = G.hand_rays()
    a, b, state, hit = G.ray_grid_interval(o, d, G.LO, G.HI, NEAR, FAR, grid, G.F32)
    res = {r[2]: (float(a[i]), float(b[i]), int(state[i])) for i, r in enumerate(G.HAND_RAYS)}
    return res if names is None else [res[n] for n in names]


def _grid(*cells):
    g = np.zeros((4, 4, 4), bool)
    for c in cells:
        g[c] = True
    return g


BOX_ONLY = {"through_cell_centres": (3.0, 5.0, 1), "along_a_cell_face": (3.0, 5.0, 1), "through_cell_corners": (2.0, 4.0, 1),
            "axis_y": (3.0, 5.0, 1), "origin_inside_box_ends_before_near": (2.0, 6.0, 0), "origin_inside": (2.0, 5.0, 1)}


def test_hand_case_one_occupied_cell():
    # x, y = 0.25 -> cell 2 on both; along -z the ray crosses iz = 3, 2, 1, 0 at t = 3 .. 5
    res = _walk(_grid((2, 2, 1)))
    assert res["through_cell_centres"] == (4.0, 4.5, 2)
    assert res["axis_y"] == BOX_ONLY["axis_y"]                                    # that ray never sees the cell
    res = _walk(_grid((2, 2, 3), (2, 2, 1)))
    assert res["through_cell_centres"] == (3.0, 4.5, 2)                           # first entered .. last left, the gap included
    assert _walk(_grid((2, 2, 3), (2, 2, 0)))["through_cell_centres"] == BOX_ONLY["through_cell_centres"]   # all of [a0, b0]
    assert _walk(_grid((2, 3, 2)))["axis_y"] == (3.0, 3.5, 2)                     # z = 0.25 -> cell 2


def test_hand_case_ray_along_a_cell_face():
    # x = 0.5 is the plane between cells 2 and 3: floor puts the ray in cell 3, and it never steps in x
    assert _walk(_grid((3, 2, 2)))["along_a_cell_face"] == (3.5, 4.0, 2)
    assert _walk(_grid((2, 2, 2)))["along_a_cell_face"] == BOX_ONLY["along_a_cell_face"]


def test_hand_case_ray_through_cell_corners_takes_the_lowest_axis_first():
    # the diagonal enters at (-1, -1) at t = 2 and meets an x and a y plane together every 0.5: x steps first, so it passes
    # through (1, 0), (2, 1), (3, 2) in a point each -- which does not count -- and never through (0, 1)
    assert _walk(_grid((1, 0, 2)))["through_cell_corners"] == BOX_ONLY["through_cell_corners"]
    assert _walk(_grid((0, 1, 2)))["through_cell_corners"] == BOX_ONLY["through_cell_corners"]
    assert _walk(_grid((1, 1, 2)))["through_cell_corners"] == (2.5, 3.0, 2)
    assert _walk(_grid((1, 0, 2), (1, 1, 2)))["through_cell_corners"] == (2.5, 3.0, 2)     # a' = the corner itself
    assert _walk(_grid((0, 0, 2), (2, 2, 2)))["through_cell_corners"] == (2.0, 3.5, 2)


def test_hand_case_zero_direction_components():
    # one zero component (the diagonal, z fixed in cell 2) and two (the axis rays): cells off the fixed index are never met
    g = _grid((1, 1, 0), (1, 1, 1), (1, 1, 3))
    assert _walk(g)["through_cell_corners"] == BOX_ONLY["through_cell_corners"]
    g = np.ones((4, 4, 4), bool)
    g[2, 2, :] = False
    assert _walk(g)["through_cell_centres"] == BOX_ONLY["through_cell_centres"]


def test_hand_case_origin_inside_the_grid():
    # the origin sits in cell (2, 2, 2); near = 2 puts the start at z = -0.25 (cell 1), cell 0 runs from t = 3 to the box's end at 5
    assert _walk(_grid((2, 2, 2)))["origin_inside"] == BOX_ONLY["origin_inside"]      # the origin's own cell lies before near
    assert _walk(_grid((2, 2, 1)))["origin_inside"] == (2.0, 3.0, 2)
    assert _walk(_grid((2, 2, 0)))["origin_inside"] == (3.0, 5.0, 2)
    assert _walk(_grid((2, 2, 0), (2, 2, 1)))["origin_inside"] == BOX_ONLY["origin_inside"]   # all of [a0, b0]: the box alone
    assert _walk(_grid((2, 2, 1)))["origin_inside_box_ends_before_near"] == (2.0, 6.0, 0)     # no hit: untouched


def test_all_empty_and_all_full_grids(scene):
    assert _walk(np.zeros((4, 4, 4), bool)) == BOX_ONLY
    assert _walk(np.ones((4, 4, 4), bool)) == BOX_ONLY          # full along the ray: the box interval, by the box rule itself
    # on the 4096 rays: both give the box rule's bounds and flags
    _, o, d, _, _ = scene
    want_bounds, want_flag = B.ray_box_bounds(o, d, G.LO, G.HI, NEAR, FAR)
    for grid in (np.zeros((16, 16, 16), bool), np.ones((16, 16, 16), bool)):
        bounds, state = G.ray_occupancy_bounds(o, d, G.LO, G.HI, NEAR, FAR, grid)
        np.testing.assert_array_equal(bounds.view(np.uint32), want_bounds.view(np.uint32))
        np.testing.assert_array_equal(state, want_flag)
    u = np.random.default_rng(2).random((4096, 5), dtype=np.float32)
    for lindisp in (False, True):
        np.testing.assert_array_equal(G.z_values(o, d, G.LO, G.HI, NEAR, FAR, np.ones((16, 16, 16), bool), u, lindisp),
                                      B.z_values(o, d, G.LO, G.HI, NEAR, FAR, u, lindisp))


# ---- bit packing ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [4, 8, 12])
def test_bit_packing_round_trip(r):
    from nerf_and_dietnerf_amd import render
    grid = np.random.default_rng(r).random((r, r, r)) < 0.3
    words = render.pack_occupancy_grid(grid)
    assert words.dtype == np.uint32 and words.shape == (r ** 3 // 32,)
    np.testing.assert_array_equal(words, G.pack_bits(grid))              # bit ix + R (iy + R iz), written out bit by bit
    np.testing.assert_array_equal(render.unpack_occupancy_grid(words), grid)
    np.testing.assert_array_equal(render.unpack_occupancy_grid(words, r), grid)
    one = np.zeros((r, r, r), bool)
    one[1, 2, 3] = True
    w = render.pack_occupancy_grid(one)
    bit = 1 + r * (2 + r * 3)
    assert w[bit >> 5] == 1 << (bit & 31) and np.count_nonzero(w) == 1


# ---- refusals of the Python layer ------------------------------------------------------------------------------------------------
class _RecordingLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append(name)
            return 0
        return call


def _bare_context(box=True):
    import nerf_and_dietnerf_amd as N
    ctx = object.__new__(N.Context)
    ctx.h, ctx.lib = None, _RecordingLib()
    ctx.cfg = N._lib.NerfConfig(5, 4, 2, 256, 128, 0.05, 2.0, 6.0, 0, 0)
    ctx.scene_box, ctx.grid_resolution = None, 0
    if box:
        ctx.set_scene_box([-1, -1, -1], [1, 1, 1])
        ctx.lib.calls.clear()
    return ctx


def test_a_grid_needs_a_box():
    ctx = _bare_context(box=False)
    with pytest.raises(RuntimeError, match=NEEDS_BOX):
        ctx.set_occupancy_grid(np.ones((4, 4, 4), bool))
    with pytest.raises(RuntimeError, match=NEEDS_BOX):
        ctx.bake_occupancy_grid(0, 16, 1.0)
    assert ctx.lib.calls == []
    ctx.set_occupancy_grid(None)                                     # clearing needs none
    assert ctx.lib.calls == ["nerf_ctx_set_occupancy_grid"]


def test_changing_or_clearing_the_box_drops_the_grid():
    ctx = _bare_context()
    ctx.set_occupancy_grid(np.ones((8, 8, 8), bool))
    assert ctx.grid_resolution == 8
    ctx.set_scene_box([-2, -2, -2], [2, 2, 2])
    assert ctx.grid_resolution == 0
    ctx.set_occupancy_grid(G.pack_bits(np.ones((12, 12, 12), bool)))     # packed words: R from their count
    assert ctx.grid_resolution == 12
    ctx.set_scene_box(None)
    assert ctx.grid_resolution == 0 and ctx.scene_box is None


@pytest.mark.parametrize("r", [0, 2, 6, 260, 10, 16.5])
def test_bad_resolution(r):
    ctx = _bare_context()
    with pytest.raises(ValueError, match=BAD_R):
        ctx.bake_occupancy_grid(0, r, 1.0)
    if r == int(r) and r > 0:
        with pytest.raises(ValueError, match=BAD_R):
            ctx.set_occupancy_grid(np.ones((int(r),) * 3, bool))
    assert ctx.lib.calls == []


def test_bad_threshold_and_counts():
    ctx = _bare_context()
    for thr in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sigma_threshold must be finite and > 0"):
            ctx.bake_occupancy_grid(0, 16, thr)
    for spc in (0, 9):
        with pytest.raises(ValueError, match="samples_per_cell must be in 1..8"):
            ctx.bake_occupancy_grid(0, 16, 1.0, samples_per_cell=spc)
    with pytest.raises(ValueError, match="dilate must be 0, 1 or 2"):
        ctx.bake_occupancy_grid(0, 16, 1.0, dilate=3)
    with pytest.raises(ValueError, match="\\(R, R, R\\)"):
        ctx.set_occupancy_grid(np.ones((4, 4, 8), bool))
    assert ctx.lib.calls == []


# ---- render_config["occupancy_grid"] ---------------------------------------------------------------------------------------------
BOX = [[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]]


class _RecordingContext:
    def __init__(self, **kw):
        self.calls, self.scene_box, self.grid_resolution, self.loaded = [], None, 0, [True, False]

    def set_scene_box(self, lo, hi=None):
        self.scene_box = (lo, hi)

    def set_occupancy_grid(self, grid):
        self.calls.append(("set_occupancy_grid", grid))
        self.grid_resolution = 0

    def bake_occupancy_grid(self, which, resolution, sigma_threshold, samples_per_cell=1, dilate=1, seed=0):
        self.calls.append(("bake", which, resolution, sigma_threshold, samples_per_cell, dilate))
        self.grid_resolution = resolution
        return 7


def _model(monkeypatch, render_config, fine=8):
    from nerf_and_dietnerf_amd import render
    monkeypatch.setattr(render, "Context", _RecordingContext)
    return render.NeRF(S.NET, dict({"n_render_samples_coarse": 8, "n_render_samples_fine": fine}, **render_config), NEAR, FAR)


def test_render_config_without_the_key_leaves_everything_as_it_was(monkeypatch):
    m = _model(monkeypatch, {"scene_box": BOX})
    assert m.grid_config is None and m.update_occupancy_grid() is None and m.ctx.calls == []
    m.occupancy_grid_epoch()
    assert m.ctx.calls == []


def test_render_config_errors(monkeypatch):
    with pytest.raises(ValueError, match=NEEDS_BOX):
        _model(monkeypatch, {"occupancy_grid": {"resolution": 16, "sigma_threshold": 1.0}})
    with pytest.raises(ValueError, match=BAD_R):
        _model(monkeypatch, {"scene_box": BOX, "occupancy_grid": {"resolution": 18, "sigma_threshold": 1.0}})
    for thr in (0.0, float("nan")):
        with pytest.raises(ValueError, match="sigma_threshold must be finite and > 0"):
            _model(monkeypatch, {"scene_box": BOX, "occupancy_grid": {"resolution": 16, "sigma_threshold": thr}})
    with pytest.raises(ValueError, match="needs 'sigma_threshold'"):
        _model(monkeypatch, {"scene_box": BOX, "occupancy_grid": {"resolution": 16}})
    with pytest.raises(ValueError, match="unknown keys"):
        _model(monkeypatch, {"scene_box": BOX, "occupancy_grid": {"resolution": 16, "sigma_threshold": 1.0, "threshold": 2}})


def test_update_bakes_from_the_fine_network_when_it_is_loaded_and_fit_follows_the_schedule(monkeypatch):
    cfg = {"resolution": 32, "sigma_threshold": 0.5, "samples_per_cell": 2, "dilate": 0, "update_every": 2, "warmup_epochs": 1}
    m = _model(monkeypatch, {"scene_box": BOX, "occupancy_grid": cfg})
    assert m.ctx.calls == []                                         # nothing is baked before there are weights
    assert m.update_occupancy_grid() == 7
    assert m.ctx.calls == [("bake", 0, 32, 0.5, 2, 0)]               # the fine network is not loaded: the coarse one
    m.ctx.loaded[1] = True
    m.update_occupancy_grid()
    assert m.ctx.calls[-1] == ("bake", 1, 32, 0.5, 2, 0)
    m.ctx.calls.clear()
    for _ in range(5):                                               # epochs 0 .. 4: off, bake, -, bake, -
        m.occupancy_grid_epoch()
    assert [c[0] for c in m.ctx.calls] == ["set_occupancy_grid", "bake", "bake"] and m.ctx.calls[0][1] is None
    # a model without a fine network bakes from the coarse one
    m = _model(monkeypatch, {"scene_box": BOX, "occupancy_grid": cfg}, fine=0)
    m.ctx.loaded[1] = True
    m.update_occupancy_grid()
    assert m.ctx.calls == [("bake", 0, 32, 0.5, 2, 0)]


def test_load_weights_bakes_the_configured_grid(monkeypatch):
    from nerf_and_dietnerf_amd import keras_h5
    cfg = {"resolution": 16, "sigma_threshold": 2.0}
    blobs = (np.zeros(3, np.float32), np.ones(3, np.float32))
    monkeypatch.setattr(keras_h5, "load_nerf_checkpoint", lambda path: blobs)
    for rc, want in (({"scene_box": BOX, "occupancy_grid": cfg}, [("load", 0), ("load", 1), ("bake", 1, 16, 2.0, 1, 1)]),
                     ({"scene_box": BOX}, [("load", 0), ("load", 1)])):
        m = _model(monkeypatch, rc)

        def load(which, blob, ctx=m.ctx):
            ctx.calls.append(("load", which))
            ctx.loaded[which] = True
        m.ctx.load_weights = load
        m.load_weights("checkpoint.h5")
        assert m.ctx.calls == want                                   # after both networks are in, from the fine one
        m.ctx.calls.clear()
        m.set_weights(*blobs)                                        # set_weights never bakes
        assert [c[0] for c in m.ctx.calls] == ["load", "load"]


def test_fit_runs_the_schedule_at_the_start_of_every_epoch(monkeypatch):
    from nerf_and_dietnerf_amd import dataset
    cfg = {"resolution": 16, "sigma_threshold": 2.0, "update_every": 2, "warmup_epochs": 1}
    m = _model(monkeypatch, {"scene_box": BOX, "occupancy_grid": cfg})
    m.ctx.grid_resolution = 16                                       # as after load_weights
    m.ctx.train_read_metric_sums = lambda: ({"loss": 0.0}, 1)
    m.train_step = lambda batch, group=None, want_metrics=True: m.ctx.calls.append(("step", batch))
    history = dataset.fit(m, [0, 1], epochs=4)
    assert len(history) == 4
    kinds = [c[0] for c in m.ctx.calls]
    # epoch 0: the warm-up turns the grid off; epochs 1 and 3: baked before the epoch's first step; epoch 2: nothing
    assert kinds == ["set_occupancy_grid", "step", "step", "bake", "step", "step", "step", "step", "bake", "step", "step"]
    assert m.ctx.calls[0][1] is None
    # a model without the key: fit calls nothing but the steps
    m = _model(monkeypatch, {"scene_box": BOX})
    m.ctx.train_read_metric_sums = lambda: ({"loss": 0.0}, 1)
    m.train_step = lambda batch, group=None, want_metrics=True: m.ctx.calls.append(("step", batch))
    dataset.fit(m, [0], epochs=2)
    assert [c[0] for c in m.ctx.calls] == ["step", "step"]


def test_packed_words_give_their_resolution_and_other_arrays_are_refused():
    ctx = _bare_context()
    ctx.set_occupancy_grid(np.zeros(256 ** 3 // 32, np.uint32))      # R from the count, without unpacking 16.7 M cells
    assert ctx.grid_resolution == 256
    ctx.lib.calls.clear()
    for bad in (np.ones(64, bool), np.zeros(3, np.uint32), np.zeros(6 ** 3 * 4, np.uint32), np.zeros((4, 4), np.uint32),
                np.zeros(2, np.float32)):
        with pytest.raises(ValueError):
            ctx.set_occupancy_grid(bad)
    assert ctx.lib.calls == []
