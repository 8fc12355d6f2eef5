"""Forward-facing scenes on the host side, no device needed: the three new entry points in header, binding and library; the two optional
``render_config`` keys (``lindisp``, ``use_ndc`` with ``ndc_near_plane``) reach the context's setters and their absence leaves a
context as it was created (linear depths, world rays); mode strings are checked; disparity sampling refuses near <= 0 with the
library's message; and the float64 / float32 restatements the GPU tests rely on (tests/sampling_space_ref.py) have the
properties the transform is defined by."""
import os
import re

import numpy as np
import pytest

import sampling_space_ref as R
import support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINDISP_MESSAGE = "lindisp needs near_boundary > 0"


def test_new_entries_in_header_binding_and_library():
    import nerf_and_dietnerf_amd as N
    hdr = open(os.path.join(ROOT, "include", "nerf_mi355.h")).read()
    # the entries are additive: header, binding and library agree on the version, whatever its number
    lib = N._lib.load()
    assert int(re.search(r"#define\s+NERF_ABI_VERSION\s+(\d+)", hdr).group(1)) == N._lib.NERF_ABI_VERSION == lib.nerf_abi_version()
    for name in ("nerf_ctx_set_sampling", "nerf_ctx_set_ray_space", "nerf_rays_to_ndc"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
    enum = {m.group(1): int(m.group(2)) for m in re.finditer(r"(NERF_(?:SAMPLING|RAYS)_\w+)\s*=\s*(\d+)", hdr)}
    assert enum == {"NERF_SAMPLING_LINEAR": 0, "NERF_SAMPLING_LINDISP": 1, "NERF_RAYS_WORLD": 0, "NERF_RAYS_NDC": 1}
    for name, value in enum.items():
        assert getattr(N._lib, name) == value
    bound = {name for name, _, _ in N._lib.SYMBOLS}
    for name in ("nerf_ctx_set_sampling", "nerf_ctx_set_ray_space", "nerf_rays_to_ndc"):
        assert name in bound and getattr(lib, name) is not None
    # the layouts the issue freezes
    import ctypes
    assert ctypes.sizeof(N._lib.NerfConfig) == 40 and ctypes.sizeof(N._lib.NerfOutputs) == 7 * ctypes.sizeof(ctypes.c_void_p)


class _RecordingContext:
    """Stands in for render.Context (which needs a device): starts as nerf_ctx_create leaves a context and records the
    setter calls."""

    def __init__(self, **kw):
        self.kw, self.calls = kw, []
        self.sampling, self.ray_space, self.ndc_near_plane = "linear", "world", 1.0

    def set_sampling(self, mode):
        self.calls.append(("set_sampling", mode))
        self.sampling = mode

    def set_ray_space(self, space, ndc_near_plane=1.0):
        self.calls.append(("set_ray_space", space, ndc_near_plane))
        self.ray_space, self.ndc_near_plane = space, ndc_near_plane


def _model(monkeypatch, render_config, near=2.0, far=6.0):
    from nerf_and_dietnerf_amd import render
    monkeypatch.setattr(render, "Context", _RecordingContext)
    return render.NeRF(S.NET, dict({"n_render_samples_coarse": 8, "n_render_samples_fine": 8}, **render_config), near, far)


def test_render_config_without_the_keys_leaves_the_context_linear_and_world(monkeypatch):
    m = _model(monkeypatch, {})
    assert m.ctx.calls == [] and (m.ctx.sampling, m.ctx.ray_space) == ("linear", "world")
    assert (m.lindisp, m.use_ndc, m.ndc_near_plane) == (False, False, 1.0)
    m = _model(monkeypatch, {"lindisp": False, "use_ndc": False, "ndc_near_plane": 0.5})
    assert m.ctx.calls == []


def test_render_config_keys_call_the_setters(monkeypatch):
    m = _model(monkeypatch, {"lindisp": True})
    assert m.ctx.calls == [("set_sampling", "lindisp")] and m.ctx.ray_space == "world"
    m = _model(monkeypatch, {"use_ndc": True}, near=0.0, far=1.0)
    assert m.ctx.calls == [("set_ray_space", "ndc", 1.0)] and m.ctx.sampling == "linear"
    m = _model(monkeypatch, {"use_ndc": True, "lindisp": True, "ndc_near_plane": 0.5}, near=0.25, far=1.0)
    assert sorted(m.ctx.calls) == [("set_ray_space", "ndc", 0.5), ("set_sampling", "lindisp")]


def test_config_names_the_keys_render_reads():
    from nerf_and_dietnerf_amd import config, render
    assert (config.LINDISP, config.USE_NDC, config.NDC_NEAR_PLANE) == (render.LINDISP, render.USE_NDC, render.NDC_NEAR_PLANE) \
        == ("lindisp", "use_ndc", "ndc_near_plane")


class _RecordingLib:
    """The new entry points of a library that accepts everything."""

    def __init__(self):
        self.calls = []

    def nerf_ctx_set_sampling(self, h, mode):
        self.calls.append(("nerf_ctx_set_sampling", mode))
        return 0

    def nerf_ctx_set_ray_space(self, h, space, near_plane):
        self.calls.append(("nerf_ctx_set_ray_space", space, near_plane))
        return 0


def _bare_context(near, far):
    """A render.Context without a device: the real methods over a recording library."""
    import nerf_and_dietnerf_amd as N
    ctx = object.__new__(N.Context)
    ctx.h, ctx.lib = None, _RecordingLib()
    ctx.cfg = N._lib.NerfConfig(5, 4, 2, 256, 128, 0.05, near, far, 0, 0)
    ctx.sampling, ctx.ray_space, ctx.ndc_near_plane = "linear", "world", 1.0
    return ctx


def test_setters_map_the_names_and_refuse_unknown_ones():
    import nerf_and_dietnerf_amd as N
    ctx = _bare_context(2.0, 6.0)
    ctx.set_sampling("lindisp")
    ctx.set_sampling("linear")
    ctx.set_ray_space("ndc", 0.5)
    ctx.set_ray_space("world")
    assert ctx.lib.calls == [("nerf_ctx_set_sampling", N._lib.NERF_SAMPLING_LINDISP),
                             ("nerf_ctx_set_sampling", N._lib.NERF_SAMPLING_LINEAR),
                             ("nerf_ctx_set_ray_space", N._lib.NERF_RAYS_NDC, 0.5),
                             ("nerf_ctx_set_ray_space", N._lib.NERF_RAYS_WORLD, 1.0)]
    assert (ctx.sampling, ctx.ray_space, ctx.ndc_near_plane) == ("linear", "world", 0.5)
    with pytest.raises(ValueError, match=r"'lindisp'.*'linear'|'linear'.*'lindisp'"):
        ctx.set_sampling("disparity")
    with pytest.raises(ValueError, match=r"'ndc'.*'world'|'world'.*'ndc'"):
        ctx.set_ray_space("screen")
    assert len(ctx.lib.calls) == 4                       # nothing reached the library


@pytest.mark.parametrize("near", [0.0, -1.0])
def test_lindisp_refuses_a_near_bound_that_is_not_positive(near):
    """Context.set_sampling raises the library's message before any device call; the text is the one the library itself
    gives (nerf_ctx_set_sampling, and every call that draws depths: tests/test_gpu_sampling_space.py runs those)."""
    import nerf_and_dietnerf_amd as N
    ctx = _bare_context(near, 1.0)
    with pytest.raises(RuntimeError, match=LINDISP_MESSAGE):
        ctx.set_sampling("lindisp")
    assert ctx.lib.calls == [] and ctx.sampling == "linear"
    assert LINDISP_MESSAGE.encode() in open(N._lib.LIB_PATH, "rb").read()


def test_reference_formulas_have_the_defining_properties(oracle):
    """tests/sampling_space_ref.py itself: lindisp depths run from near to (just below) far, uniformly in 1/z; NDC origins lie
    on z = -1, o' + d' on z = +1, and the NDC point at t' = 1 - p_z / (p_z + t d_z) is the perspective projection of p + t d."""
    u = np.full((1, 8), 0.5)
    z = R.lindisp_f64(1.0, 8.0, u)
    assert np.allclose(np.diff(1.0 / z), (1 / 8.0 - 1.0) / 8) and z[0, 0] > 1.0 and z[0, -1] < 8.0
    assert R.lindisp_f64(0.5, 64.0, np.zeros((1, 4)))[0, 0] == 0.5
    edge = np.array([[0.0, R.U_BELOW_ONE, 0.3, R.U_BELOW_ONE]], np.float32)
    for near, far in ((1.0, 8.0), (0.5, 64.0)):
        z32 = R.lindisp_f32(near, far, edge)
        assert np.all(z32 >= near) and np.all(z32 < far) and np.all(np.diff(z32) > 0)
        assert np.all(np.abs(z32 - R.lindisp_f64(near, far, edge)) <= R.lindisp_bar(near, far) * R.lindisp_f64(near, far, edge))
    rig, fov = R.forward_facing_poses()
    assert rig.shape == (3, 4, 4) and np.all(rig[:, 2, 2] > 0.9)          # viewing axis -R[:, 2] within 26 degrees of -z
    n, k = 0.5, float(R.ndc_scale(fov))
    for c2w in rig:
        o, d = R.world_rays(oracle, c2w, fov, 16, 24)
        oo, dd, p = R.rays_to_ndc_f64(o, d, fov, n)
        assert np.allclose(oo[:, 2], -1.0, atol=1e-12) and np.allclose(oo[:, 2] + dd[:, 2], 1.0, atol=1e-12)
        assert np.all(oo[:, 3] == 1.0) and np.all(dd[:, 3] == 0.0)
        for t in (0.1, 1.0, 10.0, 1000.0):
            pt = p + t * d[:, :3].astype(np.float64)
            proj = np.stack([-k * pt[:, 0] / pt[:, 2], -k * pt[:, 1] / pt[:, 2], 1.0 + 2 * n / pt[:, 2]], axis=1)
            tp = 1.0 - p[:, 2] / (p[:, 2] + t * d[:, 2].astype(np.float64))
            assert np.allclose(oo[:, :3] + tp[:, None] * dd[:, :3], proj, atol=1e-12)
        o32, d32 = R.rays_to_ndc_f32(o, d, fov, n)
        bars = R.ndc_bars(o, d, fov, n)
        assert R.within(o32[:, :2], oo[:, :2], bars["oxy"]) and R.within(o32[:, 2], oo[:, 2], bars["oz"])
        assert R.within(d32[:, :2], dd[:, :2], bars["dxy"]) and R.within(d32[:, 2], dd[:, 2], bars["dz"])
