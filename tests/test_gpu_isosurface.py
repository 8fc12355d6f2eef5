"""Mesh extraction on the device: the isosurface against the numpy restatement of tests/isosurface_ref.py, bit for bit (vertices,
normals, triangles, both counts), the scans at the largest lattice, the density lattice and the vertex colours against the
public point query (Context.model_predict), and NeRF.extract_mesh on the shipped checkpoint."""
import numpy as np
import pytest

import isosurface_ref as R
from occupancy_ref import GOLDEN_BOX
import support as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import nerf_and_dietnerf_amd as N
    c = N.Context(precision="fp32")
    yield c
    c.close()


def _assert_same_mesh(got, want):
    v, t, nrm = got
    rv, rn, rt = want
    assert v.dtype == np.float32 and nrm.dtype == np.float32 and t.dtype == np.int32
    assert v.shape == rv.shape and nrm.shape == rn.shape and t.shape == rt.shape, (v.shape, t.shape, rv.shape, rt.shape)
    np.testing.assert_array_equal(t, rt)
    np.testing.assert_array_equal(v.view(np.uint32), rv.view(np.uint32))
    np.testing.assert_array_equal(nrm.view(np.uint32), rn.view(np.uint32))


def _check(ctx, s, iso=0.0):
    want = R.isosurface(s, R.LO, R.HI, iso)
    _assert_same_mesh(ctx.isosurface(s, R.LO, R.HI, iso), want)
    return want


# ---- 1. the isosurface against the restatement ----------------------------------------------------------------------------------
def test_all_patterns_of_one_cube(ctx):
    rng = np.random.default_rng(0)
    for pattern in range(256):
        sign = np.array([1.0 if pattern >> k & 1 else -1.0 for k in range(8)], np.float32).reshape(2, 2, 2)
        rv, _, rt = _check(ctx, sign * rng.uniform(0.1, 2.0, (2, 2, 2)).astype(np.float32))
        assert (len(rv) == 0) == (pattern in (0, 255)) and (len(rt) == 0) == (pattern in (0, 255))


@pytest.mark.parametrize("n", [3, 5, 17])
def test_random_fields(ctx, n):
    rv, _, rt = _check(ctx, np.random.default_rng(n).standard_normal((n, n, n)).astype(np.float32))
    assert len(rv) > 0 and len(rt) > 0


@pytest.mark.parametrize("name", ["ball", "torus", "tie"])
def test_fields_at_33(ctx, name):
    s = R.tie_field(31) if name == "tie" else {"ball": R.ball, "torus": R.torus}[name](33)
    assert s.shape == (33, 33, 33)
    rv, _, rt = _check(ctx, s)
    assert len(R.unmatched_edges(rt)) == 0
    if name == "ball":
        assert (len(rv), len(rt)) == (6018, 12032)


def test_nan_and_inf_entries(ctx):
    rng = np.random.default_rng(4)
    s = rng.standard_normal((9, 9, 9)).astype(np.float32)
    for i, (a, b, c) in enumerate(rng.integers(0, 9, (90, 3))):
        s[a, b, c] = (np.nan, np.inf, -np.inf)[i % 3]
    rv, rn, _ = _check(ctx, s)
    assert np.isfinite(rv).all() and np.isfinite(rn).all()
    _check(ctx, s, iso=0.25)


@pytest.mark.parametrize("value", [-1.0, 1.0])
def test_empty_surface(ctx, value):
    v, t, nrm = ctx.isosurface(np.full((5, 5, 5), value, np.float32), R.LO, R.HI, 0.0)
    assert v.shape == (0, 3) and nrm.shape == (0, 3) and t.shape == (0, 3) and t.dtype == np.int32
    v, t, nrm = ctx.isosurface(np.full((5, 5, 5), value, np.float32), R.LO, R.HI, 0.0, normals=False)
    assert v.shape == (0, 3) and nrm is None


def test_device_arrays_give_the_same_bits(ctx):
    import torch
    s = np.random.default_rng(8).standard_normal((17, 17, 17)).astype(np.float32)
    v, t, nrm = ctx.isosurface(s, R.LO, R.HI, 0.1)
    dv, dt, dn = ctx.isosurface(torch.as_tensor(s).cuda(), R.LO, R.HI, 0.1)
    assert dv.is_cuda and dt.is_cuda and dn.is_cuda and dt.dtype == torch.int32
    np.testing.assert_array_equal(dv.cpu().numpy().view(np.uint32), v.view(np.uint32))
    np.testing.assert_array_equal(dn.cpu().numpy().view(np.uint32), nrm.view(np.uint32))
    np.testing.assert_array_equal(dt.cpu().numpy(), t)
    v2, t2, none = ctx.isosurface(s, R.LO, R.HI, 0.1, normals=False)
    assert none is None
    np.testing.assert_array_equal(v2, v)
    np.testing.assert_array_equal(t2, t)


def test_refusals(ctx):
    import ctypes as C
    import nerf_and_dietnerf_amd as N
    fresh = N.Context(precision="fp32")
    buf = np.zeros(16, np.float32)
    assert fresh.lib.nerf_isosurface_fetch(fresh.h, buf.ctypes.data, None, buf.ctypes.data, 0) != 0
    assert "no pending mesh" in N._lib.last_error()
    fresh.close()
    with pytest.raises(RuntimeError, match=r"n must be in 2\.\.512"):
        ctx.isosurface(np.zeros((1, 1, 1), np.float32), R.LO, R.HI, 0.0)
    with pytest.raises(RuntimeError, match="finite lo < hi"):
        ctx.isosurface(np.zeros((3, 3, 3), np.float32), R.HI, R.LO, 0.0)
    with pytest.raises(RuntimeError, match="iso must be finite"):
        ctx.isosurface(np.zeros((3, 3, 3), np.float32), R.LO, R.HI, float("nan"))
    with pytest.raises(ValueError, match=r"\(n, n, n\)"):
        ctx.isosurface(np.zeros((3, 3, 4), np.float32), R.LO, R.HI, 0.0)
    nv, nt = C.c_int64(-1), C.c_int64(-1)
    assert ctx.lib.nerf_isosurface(ctx.h, buf.ctypes.data, 513, buf.ctypes.data, buf.ctypes.data, 0.0, C.byref(nv), C.byref(nt), 0) != 0
    assert "n must be in 2..512" in N._lib.last_error()


# ---- 2. the scans at the largest lattice ----------------------------------------------------------------------------------------
def test_full_size_lattice(ctx):
    """n = 512: -1 everywhere but a ball of radius 6 cells centred 10 cells from the far corner, so the only output comes after
    almost every element of both scans (134 M points in 32768 tiles: every level of the scan carries a non-trivial prefix
    only in its last elements, and the zeros before them must stay zeros).  Equal to the restatement on the 24^3 block that
    holds the ball: its numbering is the whole lattice's, since nothing lies before it."""
    import torch
    n, m, centre, radius = 512, 24, 501.0, 6.0
    i = np.arange(n - m, n, dtype=np.float64) - centre
    d = np.sqrt(i[:, None, None] ** 2 + i[None, :, None] ** 2 + i[None, None, :] ** 2)
    block = np.where(radius - d > 0, radius - d, -1.0).astype(np.float32)
    s = torch.full((n, n, n), -1.0, dtype=torch.float32, device="cuda")
    s[n - m:, n - m:, n - m:] = torch.as_tensor(block).cuda()
    rv, rn, rt = R.isosurface(block, R.LO, R.HI, 0.0, n=n, offset=(n - m,) * 3)
    assert len(rv) > 500 and len(R.unmatched_edges(rt)) == 0
    v, t, nrm = ctx.isosurface(s, R.LO, R.HI, 0.0)
    del s
    _assert_same_mesh((v.cpu().numpy(), t.cpu().numpy(), nrm.cpu().numpy()), (rv, rn, rt))
    # a second, small call on the same context: the large scratch is reused, not trusted
    _check(ctx, R.ball(9))


# ---- 3. the density lattice -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_lattice_equals_the_point_query(precision):
    c = S.glorot_context(precision)
    c.set_scene_box(R.LO, R.HI)
    for n, which, view in ((5, 0, None), (17, 1, (0.6, -0.48, 0.64)), (102, 0, None)) if precision == "f16x3" else \
            ((5, 1, (0.0, 1.0, 0.0)), (17, 0, None)):
        pts = R.lattice_points(R.LO, R.HI, n)
        vd = np.tile(np.array((0.0, 0.0, 1.0) if view is None else view, np.float32), (len(pts), 1))
        want = c.model_predict(which, pts, vd)[:, 3]
        got = c.density_lattice(which, n, view_dir=view)
        assert got.shape == (n, n, n) and got.dtype == np.float32
        np.testing.assert_array_equal(got.ravel().view(np.uint32), want.view(np.uint32))
        assert np.unique(got).size > n                          # a field, not a constant
    import torch
    dev = c.density_lattice(1, 17, view_dir=(0.6, -0.48, 0.64), device_out=True)
    assert dev.is_cuda and tuple(dev.shape) == (17, 17, 17)
    np.testing.assert_array_equal(dev.cpu().numpy(), c.density_lattice(1, 17, view_dir=(0.6, -0.48, 0.64)))
    c.close()


def test_lattice_without_directions_ignores_view_dir():
    c = S.glorot_context("fp32", n_angles=0)
    c.set_scene_box(R.LO, R.HI)
    a = c.density_lattice(0, 5)
    b = c.density_lattice(0, 5, view_dir=(1.0, 0.0, 0.0))
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    want = c.model_predict(0, R.lattice_points(R.LO, R.HI, 5), None)[:, 3]
    np.testing.assert_array_equal(a.ravel().view(np.uint32), want.view(np.uint32))
    c.close()


def test_lattice_refusals():
    import nerf_and_dietnerf_amd as N
    c = N.Context(precision="fp32")
    out = np.zeros(8, np.float32)
    with pytest.raises(RuntimeError, match="needs a scene box"):
        c.density_lattice(0, 5)
    assert c.lib.nerf_density_lattice(c.h, 0, 2, None, out.ctypes.data, 0) != 0 and "needs a scene box" in N._lib.last_error()
    c.set_scene_box(R.LO, R.HI)
    with pytest.raises(RuntimeError, match="no weights loaded"):
        c.density_lattice(0, 5)
    c.load_weights(0, N.glorot_blob(0))
    for n in (1, 513):
        with pytest.raises(ValueError, match=r"n must be in 2\.\.512"):
            c.density_lattice(0, n)
        assert c.lib.nerf_density_lattice(c.h, 0, n, None, out.ctypes.data, 0) != 0
        assert "n must be in 2..512" in N._lib.last_error()
    assert c.density_lattice(0, 2).shape == (2, 2, 2)
    c.close()


# ---- 4. vertex colours ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_colors_equal_the_point_query(precision):
    c = S.glorot_context(precision)
    v, nrm, _ = R.isosurface(R.ball(17), R.LO, R.HI, 0.0)
    v, nrm = v.copy(), nrm.copy()
    assert len(v) > 1024 and len(v) % 64 != 0
    nrm[::7] = 0.0                                             # zero normals look down +z
    view = np.where((nrm == 0).all(axis=1)[:, None], np.array([0.0, 0.0, 1.0], np.float32), -nrm).astype(np.float32)
    raw = c.model_predict(1, v, view)
    want = 1.0 / (1.0 + np.exp(-raw[:, :3].astype(np.float64)))
    got = c.mesh_colors(1, v, nrm)
    assert got.shape == v.shape and got.dtype == np.float32
    err = np.abs(got - want).max()
    print(f"[mesh_colors, {precision}] max |rgb - sigmoid(model_predict)| = {err:.2e}")
    assert err <= 1e-6
    assert np.ptp(got) > 1e-3
    import torch
    dev = c.mesh_colors(1, torch.as_tensor(v).cuda(), torch.as_tensor(nrm).cuda())
    assert dev.is_cuda
    np.testing.assert_array_equal(dev.cpu().numpy(), got)
    assert c.mesh_colors(1, v[:0], nrm[:0]).shape == (0, 3)
    c.close()


# ---- 5. end to end on the shipped checkpoint --------------------------------------------------------------------------------------
def test_extract_mesh_on_the_shipped_checkpoint(golden_ckpt, tmp_path):
    import nerf_and_dietnerf_amd as N
    rc = {"n_render_samples_coarse": 8, "n_render_samples_fine": 16, "scene_box": [list(GOLDEN_BOX[0]), list(GOLDEN_BOX[1])]}
    m = N.NeRF(S.NET, rc, float(golden_ckpt["near"]), float(golden_ckpt["far"]), precision="f16x3")
    m.set_weights(golden_ckpt["blob_coarse"], golden_ckpt["blob_fine"])
    n = 65
    sigma = m.ctx.density_lattice(1, n)
    positive = sigma[sigma > 0]
    assert positive.size > 100
    thr = float(np.median(positive))                           # the surface cannot be empty
    path = tmp_path / "scene.ply"
    mesh = m.extract_mesh(resolution=n, sigma_threshold=thr, path=path)
    v, nrm, t, rgb = mesh["vertices"], mesh["normals"], mesh["triangles"], mesh["colors"]
    assert len(v) > 0 and len(t) > 0 and t.dtype == np.int32 and t.min() >= 0 and t.max() < len(v)
    # the same mesh as the three calls made by hand on host arrays (which = None is the fine network)
    hv, ht, hn = m.ctx.isosurface(sigma, GOLDEN_BOX[0], GOLDEN_BOX[1], thr)
    np.testing.assert_array_equal(hv, v)
    np.testing.assert_array_equal(ht, t)
    np.testing.assert_array_equal(hn, nrm)
    # closed except where the surface leaves the box: an unmatched edge has both ends on a face of the lattice
    lo, hi = np.array(GOLDEN_BOX[0], np.float32), np.array(GOLDEN_BOX[1], np.float32)
    last = lo + R.lattice_step(lo, hi, n) * np.float32(n - 1)
    on_face = ((v == lo) | (v == last)).any(axis=1)
    open_edges = R.unmatched_edges(t)
    assert on_face[open_edges.ravel()].all()
    assert len(open_edges) < len(R.directed_edges(t))
    length = np.linalg.norm(nrm.astype(np.float64), axis=1)
    assert (np.abs(length - 1.0) < 1e-6).sum() + (length == 0).sum() == len(v)
    assert rgb.shape == v.shape and rgb.dtype == np.float32 and rgb.min() >= 0.0 and rgb.max() <= 1.0
    back = N.read_ply(path)
    np.testing.assert_array_equal(back["vertices"].view(np.uint32), v.view(np.uint32))
    np.testing.assert_array_equal(back["normals"].view(np.uint32), nrm.view(np.uint32))
    np.testing.assert_array_equal(back["triangles"], t)
    np.testing.assert_array_equal(back["colors"], np.rint(rgb.astype(np.float64) * 255).astype(np.uint8))
    # no colours, the coarse network
    plain = m.extract_mesh(resolution=17, sigma_threshold=thr, which=0, colors=False)
    assert "colors" not in plain and plain["triangles"].shape[1] == 3 and plain["normals"].shape == plain["vertices"].shape
    m.ctx.close()
    box_less = N.NeRF(S.NET, {"n_render_samples_coarse": 8, "n_render_samples_fine": 16}, 2.0, 6.0, precision="fp32")
    with pytest.raises(ValueError, match="scene_box"):
        box_less.extract_mesh()
    box_less.ctx.close()
