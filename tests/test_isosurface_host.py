"""The isosurface rule without a device: the numpy restatement (tests/isosurface_ref.py) on analytic fields -- closed, consistently
oriented, the right topology, the right size -- and on random and tie fields; the PLY round trip; and the declarations of the
mesh entry points."""
import os
import re

import numpy as np
import pytest

import isosurface_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESH_ENTRIES = ("nerf_density_lattice", "nerf_isosurface", "nerf_isosurface_fetch", "nerf_mesh_colors")


@pytest.fixture(scope="module")
def analytic():
    """name -> (vertices, normals, triangles) at n = 33, iso = 0; computed once and never written to."""
    out = {name: R.isosurface(field(33), R.LO, R.HI, 0.0) for name, field in (("ball", R.ball), ("torus", R.torus),
                                                                              ("two_balls", R.two_balls))}
    for mesh in out.values():
        for a in mesh:
            a.setflags(write=False)
    return out


@pytest.mark.parametrize("name,chi", [("ball", 2), ("torus", 0), ("two_balls", 4)])
def test_analytic_fields_are_closed_oriented_surfaces(analytic, name, chi):
    v, nrm, t = analytic[name]
    assert v.dtype == np.float32 and nrm.dtype == np.float32 and t.dtype == np.int32
    assert len(R.unmatched_edges(t)) == 0                      # every directed edge once, its reverse once
    assert len(np.unique(t)) == len(v)                         # every vertex is used
    assert R.euler_characteristic(len(v), t) == chi
    assert R.signed_volume(v, t) > 0                           # counter-clockwise from outside
    length = np.linalg.norm(nrm.astype(np.float64), axis=1)
    assert np.abs(length - 1.0).max() < 1e-6


def test_ball_figures(analytic):
    """n = 33: volume 0.9953 of the analytic ball's (the surface is inscribed: below 1), area 0.9976, 6018 vertices, 12032
    triangles, farthest vertex 0.037 of a step off the sphere; at n = 17 the volume ratio is 0.981."""
    v, nrm, t = analytic["ball"]
    ratio = R.signed_volume(v, t) / (4.0 / 3.0 * np.pi * R.BALL_R ** 3)
    area_ratio = R.area(v, t) / (4.0 * np.pi * R.BALL_R ** 2)
    step = R.lattice_step(R.LO, R.HI, 33).astype(np.float64)
    off = np.abs(np.linalg.norm(v.astype(np.float64) - np.array(R.BALL_C), axis=1) - R.BALL_R).max() / step.min()
    print(f"ball n=33: volume ratio {ratio:.4f}, area ratio {area_ratio:.4f}, {len(v)} vertices, {len(t)} triangles, "
          f"farthest vertex {off:.3f} step")
    assert 0.99 <= ratio <= 1.0
    assert off <= 0.05
    radial = (v.astype(np.float64) - np.array(R.BALL_C)) / R.BALL_R
    assert (np.einsum("ij,ij->i", radial, nrm.astype(np.float64)) > 0.99).all()        # normals point out of the ball
    v17, _, t17 = R.isosurface(R.ball(17), R.LO, R.HI, 0.0)
    ratio17 = R.signed_volume(v17, t17) / (4.0 / 3.0 * np.pi * R.BALL_R ** 3)
    print(f"ball n=17: volume ratio {ratio17:.4f}")
    assert ratio17 < ratio


@pytest.mark.parametrize("n", [2, 3, 5, 9])
def test_random_fields_stay_closed(n):
    v, _, t = R.isosurface(R.random_field(n, seed=n), R.LO, R.HI, 0.0)
    assert len(t) > 0 and len(R.unmatched_edges(t)) == 0
    assert len(np.unique(t)) == len(v)


def test_tie_field_stays_closed():
    """Many lattice values equal iso: vertices coincide and triangles degenerate, which breaks an orientation taken from
    vertex positions -- the combinatorial one does not notice."""
    s = R.tie_field()
    assert (s == 0).sum() > 100
    v, _, t = R.isosurface(s, R.LO, R.HI, 0.0)
    assert len(np.unique(v, axis=0)) < len(v)                  # coincident vertices are there
    assert len(t) > 0 and len(R.unmatched_edges(t)) == 0
    assert len(np.unique(t)) == len(v)


def test_nan_is_outside_and_t_falls_back():
    s = R.padded(np.full((3, 3, 3), 1.0, np.float32))
    s[0, 0, 0], s[2, 2, 2] = np.nan, np.inf                    # an outside NaN corner, an inside +inf centre
    v, nrm, t = R.isosurface(s, R.LO, R.HI, 0.0)
    assert np.isfinite(v).all() and np.isfinite(nrm).all()
    assert len(R.unmatched_edges(t)) == 0


def test_block_of_a_larger_lattice():
    """A block with an offset gives the whole lattice's positions and its own numbering (what the full-size device test uses)."""
    s = R.padded(np.random.default_rng(5).standard_normal((3, 3, 3)).astype(np.float32), -1.0)       # 5^3
    whole = np.full((9, 9, 9), -1.0, np.float32)
    whole[3:8, 2:7, 4:9] = s                                                                         # [iz, iy, ix]
    vw, _, tw = R.isosurface(whole, R.LO, R.HI, 0.0)
    vb, _, tb = R.isosurface(s, R.LO, R.HI, 0.0, n=9, offset=(4, 2, 3))
    np.testing.assert_array_equal(vb.view(np.uint32), vw.view(np.uint32))
    np.testing.assert_array_equal(tb, tw)


def test_ply_round_trip(tmp_path):
    from nerf_and_dietnerf_amd.mesh import read_ply, write_ply
    v, nrm, t = R.isosurface(R.ball(9), R.LO, R.HI, 0.0)
    rgb = np.random.default_rng(0).random((len(v), 3)).astype(np.float32)
    rgb[0], rgb[1] = 0.0, 1.0
    path = tmp_path / "ball.ply"
    write_ply(path, v, t, nrm, rgb)
    head = open(path, "rb").read(400)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\n")
    assert b"property uchar red" in head and b"property list uchar int vertex_indices" in head
    back = read_ply(path)
    np.testing.assert_array_equal(back["vertices"].view(np.uint32), v.view(np.uint32))
    np.testing.assert_array_equal(back["normals"].view(np.uint32), nrm.view(np.uint32))
    np.testing.assert_array_equal(back["triangles"], t)
    assert back["colors"].dtype == np.uint8
    np.testing.assert_array_equal(back["colors"], np.rint(rgb.astype(np.float64) * 255).astype(np.uint8))
    write_ply(path, v, t)                                      # positions and faces alone
    back = read_ply(path)
    assert back["normals"] is None and back["colors"] is None
    np.testing.assert_array_equal(back["triangles"], t)
    write_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8))
    back = read_ply(path)
    assert back["vertices"].shape == (0, 3) and back["triangles"].shape == (0, 3)
    with pytest.raises(ValueError, match="outside the vertex array"):
        write_ply(path, v, t + len(v))


def test_mesh_entry_points_are_declared_and_bound():
    """The header declares the mesh entry points, the binding lists them, and the package exports the file functions."""
    import nerf_and_dietnerf_amd as N
    text = open(os.path.join(ROOT, "include", "nerf_mi355.h")).read()
    declared = set(re.findall(r"\bint (nerf_[a-z_]+)\s*\(nerf_ctx\* ctx", text))
    bound = {name for name, _, _ in N._lib.SYMBOLS}
    for name in MESH_ENTRIES:
        assert name in declared, name
        assert name in bound, name
    for name in ("density_lattice", "isosurface", "mesh_colors"):
        assert callable(getattr(N.Context, name))
    assert callable(N.NeRF.extract_mesh) and callable(N.write_ply) and callable(N.read_ply)
