"""The scene box on the host side, no device needed: the float32 restatement the GPU tests rely on (tests/scene_box_ref.py)
on hand-made rays; the three new entry points in header, binding and library; the ``scene_box`` key of ``render_config``
reaches the context's setter and its absence leaves a context without a box; the setter's Python wrapper passes the corners
on and refuses what the library refuses, with the library's words."""
import os
import re

import numpy as np
import pytest

import scene_box_ref as B
import support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nerf_ctx_set_scene_box", "nerf_ray_box_bounds", "nerf_get_z_values_rays")
BOX_MESSAGE = "scene box needs finite lo < hi on every axis"


# ---- the reference itself ------------------------------------------------------------------------------------------------
def test_reference_on_the_hand_made_rays():
    o, d = B.edge_rays()
    a, b, hit, narrowed = B.ray_box_interval(o, d, B.LO, B.HI, B.NEAR, B.FAR)
    bounds, flag = B.ray_box_bounds(o, d, B.LO, B.HI, B.NEAR, B.FAR)
    for i, (_, _, name, want) in enumerate(B.EDGE_RAYS):
        if want is None:
            assert not hit[i] and not narrowed[i] and flag[i] == 0, name
            assert tuple(bounds[i]) == (B.NEAR, B.FAR), name
        else:
            assert hit[i] and narrowed[i] and flag[i] == 1, name
            assert (float(a[i]), float(b[i])) == want == tuple(float(v) for v in bounds[i]), name
    assert flag.dtype == np.int32 and bounds.dtype == np.float32
    # the categories are what their names say
    assert np.signbit(d[6, 0]) and np.signbit(d[6, 1]) and d[6, 0] == 0
    assert o[2, 0] == B.HI[0] and d[2, 0] == 0                            # on the face, parallel to it
    assert o[1, 0] > B.HI[0] and d[1, 0] == 0                             # parallel and outside


def test_a_box_that_contains_every_frustum_narrows_nothing():
    o, d = B.recipe_rays()
    big = np.full(3, 100.0, np.float32)
    a, b, hit, narrowed = B.ray_box_interval(o, d, -big, big, B.NEAR, B.FAR)
    assert hit.all() and not narrowed.any()
    assert np.all(a == np.float32(B.NEAR)) and np.all(b == np.float32(B.FAR))
    u = np.random.default_rng(1).random((o.shape[0], 5), dtype=np.float32)
    for lindisp in (False, True):
        np.testing.assert_array_equal(B.z_values(o, d, -big, big, B.NEAR, B.FAR, u, lindisp),
                                      B.z_values(o, d, None, None, B.NEAR, B.FAR, u, lindisp))


def test_reference_depths_without_a_box_are_the_oracles(oracle):
    """Step 6 rests on it: without a box the restatement is oracle.get_z_values / sampling_space_ref.lindisp_f32, bit for bit."""
    import sampling_space_ref as R
    o, d = B.recipe_rays()
    for s in (1, 2, 5, 64):
        u = np.random.default_rng(s).random((o.shape[0], s), dtype=np.float32)
        np.testing.assert_array_equal(B.z_values(o, d, None, None, B.NEAR, B.FAR, u), oracle.get_z_values(B.NEAR, B.FAR, u))
        np.testing.assert_array_equal(B.z_values(o, d, None, None, B.NEAR, B.FAR, u, True), R.lindisp_f32(B.NEAR, B.FAR, u))


def test_reference_depths_of_narrowed_rays_stay_in_their_interval():
    o, d = B.recipe_rays()
    a, b, hit, narrowed = B.ray_box_interval(o, d, B.LO, B.HI, B.NEAR, B.FAR)
    assert narrowed.mean() >= 0.25 and (~hit).mean() >= 0.25              # the recipe shows both
    rng = np.random.default_rng(2)
    for s in (1, 2, 5, 64):
        u = rng.random((o.shape[0], s), dtype=np.float32)
        u[0], u[-1] = 0.0, np.nextafter(np.float32(1), np.float32(0))
        z = B.z_values(o, d, B.LO, B.HI, B.NEAR, B.FAR, u)
        zn, an, bn = z[narrowed], a[narrowed, None], b[narrowed, None]
        assert np.all(zn >= an) and np.all(zn <= bn + (bn - an) / np.float32(s)) and np.all(np.diff(zn, axis=1) >= 0)
        if s > 1:                                                        # u = 0: the first and last depths are a and b exactly
            z0 = B.z_values(o, d, B.LO, B.HI, B.NEAR, B.FAR, np.zeros_like(u))
            assert np.all(z0[narrowed, 0] == a[narrowed]) and np.all(z0[narrowed, -1] == b[narrowed])
        zd = B.z_values(o, d, B.LO, B.HI, B.NEAR, B.FAR, u, lindisp=True)
        zdn = zd[narrowed]
        assert np.all(zdn >= an) and np.all(zdn < bn) and np.all(np.diff(zdn, axis=1) >= 0)
        ref = B.lindisp_f64(a[narrowed], b[narrowed], u[narrowed])
        assert np.all(np.abs(zdn - ref) <= B.lindisp_bar(a[narrowed], b[narrowed])[:, None] * ref)
        # rays the box leaves alone keep the depths of a context without a box
        np.testing.assert_array_equal(z[~narrowed], B.z_values(o, d, None, None, B.NEAR, B.FAR, u)[~narrowed])


# ---- the entries -----------------------------------------------------------------------------------------------------------
def test_new_entries_in_header_binding_and_library():
    import nerf_and_dietnerf_amd as N
    hdr = open(os.path.join(ROOT, "include", "nerf_mi355.h")).read()
    lib = N._lib.load()
    assert int(re.search(r"#define\s+NERF_ABI_VERSION\s+(\d+)", hdr).group(1)) == N._lib.NERF_ABI_VERSION == lib.nerf_abi_version() == 6
    bound = {name for name, _, _ in N._lib.SYMBOLS}
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in bound and getattr(lib, name) is not None
    assert BOX_MESSAGE.encode() in open(N._lib.LIB_PATH, "rb").read()
    import ctypes
    assert ctypes.sizeof(N._lib.NerfConfig) == 40 and ctypes.sizeof(N._lib.NerfOutputs) == 7 * ctypes.sizeof(ctypes.c_void_p)


# ---- render_config -----------------------------------------------------------------------------------------------------------
class _RecordingContext:
    """Stands in for render.Context (which needs a device) and records the setter calls."""

    def __init__(self, **kw):
        self.kw, self.calls = kw, []
        self.sampling, self.ray_space, self.ndc_near_plane, self.scene_box = "linear", "world", 1.0, None

    def set_sampling(self, mode):
        self.calls.append(("set_sampling", mode))

    def set_ray_space(self, space, ndc_near_plane=1.0):
        self.calls.append(("set_ray_space", space, ndc_near_plane))

    def set_scene_box(self, lo, hi=None):
        self.calls.append(("set_scene_box", lo, hi))
        self.scene_box = (lo, hi)


def _model(monkeypatch, render_config, near=2.0, far=6.0):
    from nerf_and_dietnerf_amd import render
    monkeypatch.setattr(render, "Context", _RecordingContext)
    return render.NeRF(S.NET, dict({"n_render_samples_coarse": 8, "n_render_samples_fine": 8}, **render_config), near, far)


def test_render_config_without_the_key_leaves_the_context_without_a_box(monkeypatch):
    m = _model(monkeypatch, {})
    assert m.ctx.calls == [] and m.ctx.scene_box is None and m.scene_box is None
    m = _model(monkeypatch, {"scene_box": None})
    assert m.ctx.calls == []


def test_render_config_key_calls_the_setter(monkeypatch):
    box = [[-1.0, -0.75, -0.5], [1.0, 0.75, 0.5]]
    m = _model(monkeypatch, {"scene_box": box})
    assert m.ctx.calls == [("set_scene_box", box[0], box[1])] and m.scene_box == box
    m = _model(monkeypatch, {"scene_box": box, "lindisp": True})
    assert sorted(c[0] for c in m.ctx.calls) == ["set_sampling", "set_scene_box"]
    with pytest.raises(ValueError, match="scene_box"):
        _model(monkeypatch, {"scene_box": [[0, 0, 0]]})


def test_dietnerf_takes_the_key_through_the_same_constructor():
    from nerf_and_dietnerf_amd import config, dietnerf, render
    assert config.SCENE_BOX == render.SCENE_BOX == "scene_box"
    assert issubclass(dietnerf.DietNeRF, render.NeRF) and "scene_box" not in dietnerf.DietNeRF.__init__.__code__.co_varnames


# ---- the setter's wrapper ------------------------------------------------------------------------------------------------------
class _RecordingLib:
    def __init__(self):
        self.calls = []

    def nerf_ctx_set_scene_box(self, h, lo, hi):
        import ctypes
        read = lambda p: None if p is None else tuple((ctypes.c_float * 3).from_address(p))
        self.calls.append((read(lo), read(hi)))
        return 0


def _bare_context():
    import nerf_and_dietnerf_amd as N
    ctx = object.__new__(N.Context)
    ctx.h, ctx.lib = None, _RecordingLib()
    ctx.cfg = N._lib.NerfConfig(5, 4, 2, 256, 128, 0.05, 2.0, 6.0, 0, 0)
    ctx.scene_box = None
    return ctx


def test_setter_passes_the_corners_and_none_turns_the_box_off():
    ctx = _bare_context()
    ctx.set_scene_box([-1, -0.75, -0.5], (1, 0.75, 0.5))
    assert ctx.lib.calls == [((-1.0, -0.75, -0.5), (1.0, 0.75, 0.5))]
    assert ctx.scene_box == ((-1.0, -0.75, -0.5), (1.0, 0.75, 0.5))
    ctx.set_scene_box(None)
    assert ctx.lib.calls[-1] == (None, None) and ctx.scene_box is None


@pytest.mark.parametrize("lo,hi", [((-1, 0.75, -0.5), (1, 0.75, 0.5)),          # lo == hi on one axis
                                   ((-1, -0.75, 0.6), (1, 0.75, 0.5)),          # lo > hi on one axis
                                   ((-1, float("nan"), -0.5), (1, 0.75, 0.5)),
                                   ((-1, -0.75, -0.5), (1, float("inf"), 0.5))])
def test_setter_refuses_what_the_library_refuses(lo, hi):
    ctx = _bare_context()
    with pytest.raises(RuntimeError, match=BOX_MESSAGE):
        ctx.set_scene_box(lo, hi)
    assert ctx.lib.calls == [] and ctx.scene_box is None


def test_setter_refuses_malformed_corners():
    ctx = _bare_context()
    with pytest.raises(ValueError, match="3 components"):
        ctx.set_scene_box([0, 0], [1, 1])
    with pytest.raises(ValueError, match="both corners"):
        ctx.set_scene_box([0, 0, 0], None)
    assert ctx.lib.calls == []
