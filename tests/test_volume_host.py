"""The radiance volume's rules on the CPU: the numpy restatement of tests/volume_ref.py (what tests/test_gpu_volume.py holds
the kernels to) against the properties the rules are meant to have -- trilinear sampling reproduces an affine field, a constant
medium has the closed-form opacity for every step count, early termination costs at most t_min, and the bake's camera
directions are the ray generator's."""
import numpy as np
import pytest

import volume_ref as V
from volume_ref import HI, LO, march_bar, random_volume, rays_through_box

F = np.float32
NEAR, FAR = 2.0, 6.0


def test_sampling_reproduces_an_affine_field():
    n = 9
    rng = np.random.default_rng(0)
    slope, offset = rng.uniform(-2.0, 2.0, (4, 3)), rng.uniform(-1.0, 1.0, 4)
    vertices = V.lattice_points(LO, HI, n).astype(np.float64)
    field = (vertices @ slope.T + offset).reshape(n, n, n, 4)
    p = rng.uniform(np.array(LO) * 0.999, np.array(HI) * 0.999, (1000, 3)).astype(F)
    got = V.sample(field.astype(F), LO, HI, p)
    want = p.astype(np.float64) @ slope.T + offset
    bar = 4 * float(np.spacing(F(np.abs(field).max())))
    err = float(np.abs(got - want).max())
    print(f"[affine field] max error {err:.3e}, bar {bar:.3e}")
    assert got.dtype == F and err <= bar


def test_sampling_at_vertices_faces_and_outside():
    n = 5
    v = random_volume(n, 1)
    pts = V.lattice_points(LO, HI, n)
    # at a vertex: its value, up to the rounding of (p - lo) / step and of v0 + f (v1 - v0) at f = 1; at the first, exactly
    at_vertices = V.sample(v, LO, HI, pts)
    assert np.abs(at_vertices - v.reshape(-1, 4)).max() <= 4 * np.spacing(v.max())
    np.testing.assert_array_equal(at_vertices[0], v[0, 0, 0])
    outside = pts + np.sign(pts) * F(10.0)                                               # clamped to the nearest face value
    on_face = np.clip(outside, np.array(LO, F), pts.max(axis=0))
    np.testing.assert_array_equal(V.sample(v, LO, HI, outside), V.sample(v, LO, HI, on_face))
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]], F)
    out = V.sample(v, LO, HI, bad)
    assert np.isnan(out[0]).all() and np.isfinite(out[1:]).all()


@pytest.mark.parametrize("n_steps", [1, 2, 7, 48])
def test_constant_medium_has_the_closed_form_opacity(n_steps):
    s, colour = 0.9, np.array([0.25, 0.5, 0.75], F)
    v = np.empty((3, 3, 3, 4), F)
    v[..., :3], v[..., 3] = colour, F(s)
    o, d = rays_through_box(64, 2)
    rgb, depth, opacity = V.march(v, LO, HI, NEAR, FAR, o, d, n_steps)
    a, b, hit, _ = V.ray_box_interval(o, d, LO, HI, NEAR, FAR)
    assert hit.all()
    want = 1.0 - np.exp(-float(F(s)) * (b.astype(np.float64) - a.astype(np.float64)))
    err_o = float(np.abs(opacity - want).max())
    err_c = float(np.abs(rgb - want[:, None] * colour.astype(np.float64)[None, :]).max())
    print(f"[constant medium, {n_steps} steps] opacity error {err_o:.3e}, rgb error {err_c:.3e}, bar {march_bar(n_steps):.3e}")
    assert err_o <= march_bar(n_steps) and err_c <= march_bar(n_steps)
    assert (depth >= a * opacity * F(0.999)).all() and (depth <= b * opacity * F(1.001)).all()


@pytest.mark.parametrize("tau", [1e-2, 1.0 / 512.0])
def test_termination_costs_at_most_t_min(tau):
    v = random_volume(9, 3, sigma_scale=40.0)
    o, d = rays_through_box(128, 4)
    _, b, hit, _ = V.ray_box_interval(o, d, LO, HI, NEAR, FAR)
    full = V.march(v, LO, HI, NEAR, FAR, o, d, 48)
    cut = V.march(v, LO, HI, NEAR, FAR, o, d, 48, t_min=tau)
    stopped = cut[2] != full[2]
    assert hit.all() and stopped.sum() > 16                      # the cut acts on this medium
    assert np.abs(cut[0] - full[0]).max() <= tau and np.abs(cut[2] - full[2]).max() <= tau
    assert (np.abs(cut[1] - full[1]) <= tau * b).all()
    assert (cut[0] <= full[0]).all() and (cut[2] <= full[2]).all()      # only a tail is dropped


@pytest.mark.parametrize("n_steps", [1, 7, 48])
def test_march_bar_covers_an_expf_one_ulp_off(n_steps):
    """The device's expf may differ from np.exp by an ulp: every exponential pushed one ulp up, or down, stays inside the bar."""
    v = random_volume(9, 7)
    o, d = rays_through_box(128, 8)
    want = V.march(v, LO, HI, NEAR, FAR, o, d, n_steps)
    worst = 0.0
    for toward in (np.inf, -np.inf):
        got = V.march(v, LO, HI, NEAR, FAR, o, d, n_steps, exp=lambda x: np.nextafter(np.exp(x.astype(F)).astype(F), F(toward)))
        worst = max(worst, float(np.abs(got[0] - want[0]).max()), float(np.abs(got[2] - want[2]).max()),
                    float(np.abs(got[1] - want[1]).max()) / FAR)
    print(f"[expf one ulp off, {n_steps} steps] worst {worst:.3e}, bar {march_bar(n_steps):.3e}")
    assert 0 < worst <= march_bar(n_steps)


def test_misses_and_nonfinite_rays_are_exact_zeros():
    v = random_volume(5, 5)
    o = np.array([[0, 0, 4, 1], [3, 0, 4, 1], [0, 0, 4, 1], [np.nan, 0, 4, 1], [0, 0, 4, 1]], F)
    d = np.array([[0, 0, -1, 0], [0, 0, -1, 0], [0, 0, 1, 0], [0, 0, -1, 0], [0, np.inf, -1, 0]], F)
    rgb, depth, opacity = V.march(v, LO, HI, NEAR, FAR, o, d, 7)
    assert opacity[0] > 0 and rgb[0].max() > 0 and NEAR < depth[0] / opacity[0] < FAR
    for out in (rgb[1:], depth[1:], opacity[1:]):
        assert (out.view(np.uint32) == 0).all()


def test_camera_directions_are_the_ray_generators(oracle):
    c2w = oracle.get_sphere_matrix(4.0, -30.0, 45.0, 10.0).astype(F)
    h, w, fov = 13, 11, 0.6911112
    d = oracle.get_rays_directions(h, w, fov, c2w).reshape(-1, 4)[:, :3]
    rng = np.random.default_rng(6)
    worst = 0.0
    for _ in range(4):
        s = rng.uniform(2.0, 6.0, len(d))
        p = (c2w[:3, 3].astype(np.float64)[None, :] + s[:, None] * d.astype(np.float64)).astype(F)
        got = V.camera_directions(p, c2w)
        # the point itself is a float32: it pins the direction to ulp(|p|) / s at best, which for these depths is below one
        # ulp of the direction's largest component -- the unit the four ulps are counted in
        ulp = np.spacing(np.abs(d).max(axis=1))[:, None]
        worst = max(worst, float((np.abs(got - d) / ulp).max()))
    print(f"[camera directions] worst error {worst:.2f} ulp of the direction's largest component, bar 4")
    assert worst <= 4.0
    # behind the camera, and at it: the central ray
    behind = (c2w[:3, 3].astype(np.float64)[None, :] - 2.0 * d[:5].astype(np.float64)).astype(F)
    at = c2w[:3, 3][None, :]
    central = -c2w[:3, 2]
    np.testing.assert_array_equal(V.camera_directions(np.concatenate([behind, at]), c2w), np.tile(central, (6, 1)))
