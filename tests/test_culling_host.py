"""Sample culling without a GPU: the float32 restatement of the per-sample rule (tests/culling_ref.py) against the same rule
in float64, its hand cases, and the Python layer's new config key and bindings.  The conditioning test and the hand cases
exercise the restatement alone; what ties the library to it is tests/test_gpu_culling.py, which holds the device to it bit for
bit.  The config and binding tests call the package's new code."""
import numpy as np
import pytest

import culling_ref as K
import occupancy_ref as G

NEAR, FAR = G.NEAR, G.FAR
BOX = [[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]]


def scene_rays():
    """The six hand rays of the grid's tests, then 4090 rays of its recipe: 4096 in all."""
    ho, hd = G.hand_rays()
    o, d = G.sphere_rays(4096 - len(ho), seed=11)
    return np.concatenate([ho, o]), np.concatenate([hd, d])


def scene_grid(r):
    """The two balls on an r^3 grid over [-1, 1]^3, plus 3 % scattered cells (seeded by r)."""
    return G.two_balls(r) | (np.random.default_rng(r).random((r, r, r)) < 0.03)


@pytest.mark.parametrize("s", [1, 55, 64])
@pytest.mark.parametrize("r", [4, 16, 64])
def test_float32_verdict_against_the_float64_verdict(r, s, capsys):
    """Depths drawn on the grid's own bounds, as a render draws them.  The two verdicts may differ on at most 1e-4 of the samples
    (tried when the rule was written: none at r <= 16, at most 6 of 262144 at r = 64: samples within a rounding of a cell face)."""
    o, d = scene_rays()
    grid = scene_grid(r)
    u = np.random.default_rng(s).random((4096, s), dtype=np.float32)
    z = G.z_values(o, d, G.LO, G.HI, NEAR, FAR, grid, u)
    k32 = K.sample_keep(o, d, z, G.LO, G.HI, grid, K.F32)
    k64 = K.sample_keep(o, d, z, G.LO, G.HI, grid, K.F64)
    differ = int((k32 != k64).sum())
    whole = int((~k32).all(axis=1).sum())
    untouched = int(k32.all(axis=1).sum())
    with capsys.disabled():
        print(f"\n[culling, r {r}, s {s}] float32 vs float64 verdict: {differ} of {k32.size} samples differ (bar 1e-4 of them); "
              f"kept share {k32.mean():.3f}, {whole} rays wholly culled, {untouched} rays with no culled sample", end="")
    assert k32.shape == (4096, s) and k32.dtype == bool
    assert differ <= 1e-4 * k32.size
    if (r, s) == (16, 64):                                         # the inputs are worth testing
        assert 0.2 <= k32.mean() <= 0.7
        assert whole >= 1 and untouched >= 100


# ---- hand cases (tests/culling_ref.py: the box [-1, 1]^3 at R = 4) ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", [K.F32, K.F64])
def test_hand_cases(dtype):
    for grid, want in K.hand_grids():
        keep = K.sample_keep(K.HAND_O, K.HAND_D, K.HAND_Z, K.HAND_LO, K.HAND_HI, grid, dtype)
        assert keep.tolist() == [want]
    inside, idx = K.sample_cells(K.HAND_O, K.HAND_D, K.HAND_Z, K.HAND_LO, K.HAND_HI, 4, dtype)
    assert inside.tolist() == [[True, True, False, False]]
    assert idx[0, 0].tolist() == [2, 2, 3] and idx[0, 1].tolist() == [2, 2, 3]
    assert idx[0, 3].tolist() == [0, 0, 0]                         # NaN (0 * NaN on x and y too): the index is held in the grid


def test_zeroing_and_scattering_rows():
    keep = np.array([[True, False, True], [False, False, True]])
    raw = np.arange(24, dtype=np.float32).reshape(2, 3, 4) + 1
    z3 = K.zero_culled(raw, keep)
    assert (z3[keep] == raw[keep]).all() and (z3[~keep] == 0).all() and raw.min() == 1
    np.testing.assert_array_equal(K.zero_culled(raw.reshape(6, 4), keep), z3.reshape(6, 4))
    np.testing.assert_array_equal(K.zero_culled(raw[..., 3], keep), z3[..., 3])
    np.testing.assert_array_equal(K.scatter_rows(raw[keep], keep), z3)


# ---- render_config["occupancy_grid"]["cull_samples"] and the bindings ---------------------------------------------------------------
def test_grid_config_takes_cull_samples_as_a_bool_only():
    from nerf_and_dietnerf_amd import render
    base = {"resolution": 16, "sigma_threshold": 2.0}
    plain = render.NeRF._grid_config(dict(base), BOX)
    assert plain == {"resolution": 16, "sigma_threshold": 2.0, "samples_per_cell": 1, "dilate": 1, "update_every": 1,
                     "warmup_epochs": 0}                           # without the key the config is what it was
    assert "cull_samples" in render._GRID_KEYS
    for flag in (True, False):
        cfg = render.NeRF._grid_config(dict(base, cull_samples=flag), BOX)
        assert cfg["cull_samples"] is flag and {k: v for k, v in cfg.items() if k != "cull_samples"} == plain
    for bad in (1, "yes", None, 0.0):
        with pytest.raises(ValueError, match="cull_samples"):
            render.NeRF._grid_config(dict(base, cull_samples=bad), BOX)


class _RecordingContext:
    def __init__(self, **kw):
        self.calls, self.scene_box, self.grid_resolution, self.loaded = [], None, 0, [True, False]

    def set_scene_box(self, lo, hi=None):
        self.scene_box = (lo, hi)

    def set_sample_culling(self, on):
        self.calls.append(("set_sample_culling", on))


def test_the_model_sets_the_flag_on_its_context(monkeypatch):
    from nerf_and_dietnerf_amd import render
    monkeypatch.setattr(render, "Context", _RecordingContext)
    net = {"hidden_layer_dim": 256, "last_hidden_layer_dim": 128, "leaky_relu_alpha": 0.05, "n_pos_enc_dim_xyz": 5,
           "n_pos_enc_view_dir": 4, "n_angles_for_model": 2}

    def model(grid_cfg):
        rc = {"n_render_samples_coarse": 8, "n_render_samples_fine": 8, "scene_box": BOX}
        if grid_cfg is not None:
            rc["occupancy_grid"] = grid_cfg
        return render.NeRF(net, rc, NEAR, FAR)
    assert model({"resolution": 16, "sigma_threshold": 2.0, "cull_samples": True}).ctx.calls == [("set_sample_culling", True)]
    assert model({"resolution": 16, "sigma_threshold": 2.0, "cull_samples": False}).ctx.calls == []
    assert model({"resolution": 16, "sigma_threshold": 2.0}).ctx.calls == []
    assert model(None).ctx.calls == []
    with pytest.raises(ValueError, match="cull_samples"):
        model({"resolution": 16, "sigma_threshold": 2.0, "cull_samples": "yes"})


def test_the_binding_declares_the_new_entries():
    import nerf_and_dietnerf_amd as N
    names = {s[0]: s for s in N._lib.SYMBOLS}
    for name, n_args in (("nerf_ctx_set_sample_culling", 2), ("nerf_sample_occupancy", 8), ("nerf_ctx_read_culling", 3)):
        assert name in names and len(names[name][2]) == n_args, name
    assert N._lib.NERF_ABI_VERSION == 6
    for method in ("set_sample_culling", "sample_occupancy", "read_culling"):
        assert callable(getattr(N.Context, method))
