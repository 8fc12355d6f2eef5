"""Training under sample culling without a GPU: the torch restatement of the culled training graph (tests/train_culling_ref.py)
against the oracle it restates, and the Python layer's new switch -- header, ctypes table, Context methods and the
render_config key.  What ties the library to the restatement is tests/test_gpu_train_culling.py."""
import os
import re

import numpy as np
import pytest

import support as S
import train_culling_ref as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = [[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]]


@pytest.fixture(scope="module")
def problem(oracle, golden_ckpt):
    n, sc, sf = 12, 6, 7
    rng = np.random.default_rng(5)
    c2w = oracle.get_sphere_matrix(1.0, -20, 30, 0).astype(np.float32)
    d = np.ascontiguousarray(oracle.get_rays_directions(8, 8, 0.46, c2w).reshape(-1, 4)[rng.choice(64, n, replace=False)])
    o = np.tile(c2w[:, 3], (n, 1)).astype(np.float32)
    near, far = float(golden_ckpt["near"]), float(golden_ckpt["far"])
    u_c, u_f = rng.random((n, sc), dtype=np.float32), rng.random((n, sf), dtype=np.float32)
    return dict(o=o, d=d, u_c=u_c, u_f=u_f, tgt=rng.random((n, 3), dtype=np.float32),
                d_rgb=(rng.standard_normal((n, 3)) * 0.1).astype(np.float32), near=near, far=far,
                z=oracle.get_z_values(near, far, u_c), bc=golden_ckpt["blob_coarse"], bf=golden_ckpt["blob_fine"])


# ---- 1. an all-True mask is the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss_scale", [None, 1024.0])
@pytest.mark.parametrize("sampler_grad", [True, False])
def test_all_kept_train_gradients_are_the_oracles(problem, sampler_grad, loss_scale):
    from oracle import train_oracle as T
    p = problem
    kw = dict(sampler_grad=sampler_grad, fp16_loss_scale=loss_scale)
    want = T.train_gradients(p["bc"], p["bf"], p["o"], p["d"], p["tgt"], p["near"], p["far"], p["u_c"], p["u_f"], **kw)
    got = TC.train_gradients(p["bc"], p["bf"], p["o"], p["d"], p["tgt"], p["z"], p["u_f"], TC.keep_all, **kw)
    assert got["loss"] == want["loss"] and got["psnr_coarse"] == want["psnr_coarse"] and got["psnr_fine"] == want["psnr_fine"]
    np.testing.assert_array_equal(got["grad_coarse"], want["grad_coarse"])
    np.testing.assert_array_equal(got["grad_fine"], want["grad_fine"])
    np.testing.assert_array_equal(got["z_fine"], want["z_fine"])
    assert want["grad_coarse"].any() and want["grad_fine"].any()
    assert [k.shape for k in got["keeps"]] == [(12, 6), (12, 7)] and all(k.all() for k in got["keeps"])


@pytest.mark.parametrize("sampler_grad", [True, False])
def test_all_kept_render_gradients_are_the_oracles(problem, sampler_grad):
    from oracle import train_oracle as T
    p = problem
    want = T.render_gradients(p["bc"], p["bf"], p["o"], p["d"], p["d_rgb"], p["near"], p["far"], p["u_c"], p["u_f"],
                              sampler_grad=sampler_grad)
    got = TC.render_gradients(p["bc"], p["bf"], p["o"], p["d"], p["d_rgb"], p["z"], p["u_f"], TC.keep_all, sampler_grad=sampler_grad)
    for k in ("rgb", "grad_coarse", "grad_fine"):
        np.testing.assert_array_equal(got[k], want[k])
    assert want["grad_fine"].any() and want["grad_coarse"].any() == sampler_grad
    assert [k.shape for k in got["keeps"]] == [(12, 6), (12, 13)]          # the fine pass is masked on the merged depths


def test_coarse_only_restatement(problem):
    from oracle import train_oracle as T
    p = problem
    want = T.train_gradients(p["bc"], None, p["o"], p["d"], p["tgt"], p["near"], p["far"], p["u_c"], None)
    got = TC.train_gradients(p["bc"], None, p["o"], p["d"], p["tgt"], p["z"], None)
    assert got["loss"] == want["loss"] and got["grad_fine"] is None
    np.testing.assert_array_equal(got["grad_coarse"], want["grad_coarse"])


# ---- 2. an all-False mask: nothing reaches a network -------------------------------------------------------------------------------
@pytest.mark.parametrize("loss_scale", [None, 1024.0])
def test_nothing_kept_gives_exact_zeros(problem, loss_scale):
    p = problem
    got = TC.train_gradients(p["bc"], p["bf"], p["o"], p["d"], p["tgt"], p["z"], p["u_f"], TC.keep_none, fp16_loss_scale=loss_scale)
    assert not got["grad_coarse"].any() and not got["grad_fine"].any()
    black = float(np.mean(p["tgt"].astype(np.float64) ** 2))              # both passes render black
    assert np.isfinite(got["loss"]) and abs(got["loss"] - 2 * black) <= 1e-12
    r = TC.render_gradients(p["bc"], p["bf"], p["o"], p["d"], p["d_rgb"], p["z"], p["u_f"], TC.keep_none)
    assert not r["grad_coarse"].any() and not r["grad_fine"].any() and not r["rgb"].any()


def test_a_partial_mask_cuts_the_culled_rows_out(problem):
    """Under a half-full grid the gradients differ from the all-kept ones, and the mask is taken on each pass's own depths."""
    p = problem
    lo, hi = (-0.6, -0.4, -1.3), (0.4, 0.8, -0.4)
    grid = np.random.default_rng(16).random((16, 16, 16)) < 0.5
    full = TC.train_gradients(p["bc"], p["bf"], p["o"], p["d"], p["tgt"], p["z"], p["u_f"])
    got = TC.train_gradients(p["bc"], p["bf"], p["o"], p["d"], p["tgt"], p["z"], p["u_f"], TC.grid_keep(lo, hi, grid))
    import culling_ref as K
    np.testing.assert_array_equal(got["keeps"][0], K.sample_keep(p["o"], p["d"], p["z"], lo, hi, grid, K.F64))
    np.testing.assert_array_equal(got["keeps"][1], K.sample_keep(p["o"], p["d"], got["z_fine"], lo, hi, grid, K.F64))
    assert not got["keeps"][0].all() and got["keeps"][0].any()
    assert not np.array_equal(got["grad_coarse"], full["grad_coarse"]) and np.isfinite(got["grad_fine"]).all()
    assert TC.face_margin(p["o"], p["d"], p["z"], lo, hi, 16) >= 0.0


def test_face_margin_on_hand_points():
    o = np.array([[0.25, 0.25, 4.0, 1.0]], np.float32)
    d = np.array([[0.0, 0.0, -1.0, 0.0]], np.float32)
    lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)                       # R = 4: cells of 0.5
    assert TC.face_margin(o, d, np.array([[3.5]], np.float32), lo, hi, 4) == 0.0          # p_z = 0.5: a cell face
    assert TC.face_margin(o, d, np.array([[3.0]], np.float32), lo, hi, 4) == 0.0          # p_z = 1.0: the box face
    assert abs(TC.face_margin(o, d, np.array([[3.3]], np.float32), lo, hi, 4) - 0.4) < 1e-6    # p = (.25, .25, .7): z plane .5 is 0.4 cells away
    assert abs(TC.face_margin(o, d, np.array([[2.5]], np.float32), lo, hi, 4) - 1.0) < 1e-6    # p_z = 1.5: one cell outside


# ---- 3. header, ctypes table, Context and render_config are in step ----------------------------------------------------------------
def test_the_header_declares_the_switch_as_abi_6_plus():
    text = open(os.path.join(ROOT, "include", "nerf_mi355.h")).read()
    assert re.search(r"\bint\s+nerf_ctx_set_train_sample_culling\s*\(\s*nerf_ctx\s*\*\s*ctx\s*,\s*int\s+on\s*\)\s*;", text)
    comment = text[:text.index("int nerf_ctx_set_train_sample_culling")].rsplit("/*", 1)[1]
    assert comment.lstrip().startswith("ABI 6+") and "synchronise" in comment and "NOT asynchronous" in comment
    assert re.search(r"#define\s+NERF_ABI_VERSION\s+6\b", text)
    # the render flag's comment still says the trainer ignores THAT flag
    render = text[:text.index("int nerf_ctx_set_sample_culling")].rsplit("/*", 1)[1]
    assert "IGNORE it" in render


def test_the_binding_declares_the_new_entry():
    import ctypes as C
    import nerf_and_dietnerf_amd as N
    names = {s[0]: s for s in N._lib.SYMBOLS}
    assert "nerf_ctx_set_train_sample_culling" in names
    _, res, args = names["nerf_ctx_set_train_sample_culling"]
    assert res is C.c_int and len(args) == 2 and args[1] is C.c_int
    assert N._lib.NERF_ABI_VERSION == 6
    assert callable(N.Context.set_train_sample_culling) and isinstance(N.Context.train_sample_culling, property)
    assert getattr(N._lib.load(), "nerf_ctx_set_train_sample_culling") is not None


def test_grid_config_takes_cull_train_samples_as_a_bool_only():
    from nerf_and_dietnerf_amd import render
    base = {"resolution": 16, "sigma_threshold": 2.0}
    plain = render.NeRF._grid_config(dict(base), BOX)
    assert "cull_train_samples" not in plain and "cull_train_samples" in render._GRID_KEYS
    assert render.GRID_CULL_TRAIN_SAMPLES == "cull_train_samples"
    for flag in (True, False):
        cfg = render.NeRF._grid_config(dict(base, cull_train_samples=flag), BOX)
        assert cfg["cull_train_samples"] is flag and {k: v for k, v in cfg.items() if k != "cull_train_samples"} == plain
    both = render.NeRF._grid_config(dict(base, cull_train_samples=True, cull_samples=False), BOX)
    assert both["cull_train_samples"] is True and both["cull_samples"] is False
    for bad in (1, "yes", None, 0.0):
        with pytest.raises(ValueError, match="cull_train_samples"):
            render.NeRF._grid_config(dict(base, cull_train_samples=bad), BOX)


class _RecordingContext:
    def __init__(self, **kw):
        self.calls, self.scene_box, self.grid_resolution, self.loaded = [], None, 0, [True, False]

    def set_scene_box(self, lo, hi=None):
        self.scene_box = (lo, hi)

    def set_sample_culling(self, on):
        self.calls.append(("set_sample_culling", on))

    def set_train_sample_culling(self, on):
        self.calls.append(("set_train_sample_culling", on))


def _model(render, grid_cfg, box=BOX):
    rc = {"n_render_samples_coarse": 8, "n_render_samples_fine": 8}
    if box is not None:
        rc["scene_box"] = box
    if grid_cfg is not None:
        rc["occupancy_grid"] = grid_cfg
    return render.NeRF(S.NET, rc, 2.0, 6.0)


def test_the_model_sets_the_train_flag_on_its_context(monkeypatch):
    from nerf_and_dietnerf_amd import render
    monkeypatch.setattr(render, "Context", _RecordingContext)
    base = {"resolution": 16, "sigma_threshold": 2.0}
    assert _model(render, dict(base, cull_train_samples=True)).ctx.calls == [("set_train_sample_culling", True)]
    assert _model(render, dict(base, cull_train_samples=False)).ctx.calls == []
    assert _model(render, dict(base)).ctx.calls == []
    assert _model(render, None).ctx.calls == []
    # the two switches are read side by side and are independent
    assert _model(render, dict(base, cull_samples=True, cull_train_samples=True)).ctx.calls == [
        ("set_sample_culling", True), ("set_train_sample_culling", True)]
    assert _model(render, dict(base, cull_samples=True)).ctx.calls == [("set_sample_culling", True)]


# ---- 4. the key needs a box and a grid config, as "cull_samples" does ---------------------------------------------------------------
def test_cull_train_samples_needs_a_scene_box_and_a_grid_config(monkeypatch):
    from nerf_and_dietnerf_amd import render
    monkeypatch.setattr(render, "Context", _RecordingContext)
    for key in ("cull_train_samples", "cull_samples"):
        with pytest.raises(ValueError, match=render.GRID_NEEDS_BOX):
            _model(render, {"resolution": 16, "sigma_threshold": 2.0, key: True}, box=None)
        with pytest.raises(ValueError, match="needs 'resolution'"):       # the key alone is no grid config
            _model(render, {key: True})
        with pytest.raises(ValueError, match=key):
            _model(render, {"resolution": 16, "sigma_threshold": 2.0, key: "yes"})
