"""Test-side restatement of the radiance volume (include/nerf_mi355.h: nerf_radiance_lattice, nerf_volume_sample,
nerf_volume_march): the per-vertex camera directions of the bake, trilinear sampling and the march, in numpy float32 with the
kernels' operations in the kernels' order, every operation rounded on its own; np.exp in float32 stands for expf.  Imported
by tests/test_volume_host.py and tests/test_gpu_volume.py; nothing here touches the library.

A volume is (n, n, n, 4) indexed [iz, iy, ix, channel] over a box (lo, hi): vertex i of axis a lies at lo_a + step_a i,
step_a = (hi_a - lo_a) / (n - 1)."""
import numpy as np

from isosurface_ref import lattice_points, lattice_step      # the density lattice's vertex positions: the volume's too
from scene_box_ref import ray_box_interval

F = np.float32
LO, HI = (-1.0, -1.2, -0.9), (1.1, 1.0, 1.3)          # the box of the volume tests: three different extents


def camera_directions(points, c2w):
    """The direction the ray generator gives the pixel whose ray passes through each point (M, 3): q = p - t,
    s = -((c02 q_x + c12 q_y) + c22 q_z), q / s where s > 0 and finite, the central ray's (-c02, -c12, -c22) elsewhere."""
    p, c = np.asarray(points, F), np.asarray(c2w, F).reshape(4, 4)
    q = (p - c[:3, 3][None, :]).astype(F)
    with np.errstate(all="ignore"):
        s = -(((c[0, 2] * q[:, 0]).astype(F) + (c[1, 2] * q[:, 1]).astype(F)).astype(F) + (c[2, 2] * q[:, 2]).astype(F)).astype(F)
        front = (s > 0) & np.isfinite(s)
        d = (q / np.where(front, s, F(1))[:, None]).astype(F)
    return np.where(front[:, None], d, (-c[:3, 2])[None, :]).astype(F)


def _cell(p, lo, step, n):
    """One axis -> (cell in [0, n - 2], weight of the upper vertex in [0, 1] or NaN)."""
    with np.errstate(all="ignore"):
        g = ((p - lo).astype(F) / step).astype(F)
        inside = (g >= 0) & (g < F(n - 1))
        i = np.where(g >= 0, np.where(inside, np.floor(np.where(inside, g, F(0))), n - 2), 0).astype(np.int64)
        f = (g - i.astype(F)).astype(F)
    f = np.where(f < 0, F(0), np.where(f > 1, F(1), f)).astype(F)
    return i, f


def _lerp(a, b, f):
    with np.errstate(all="ignore"):
        return (a + (f * (b - a).astype(F)).astype(F)).astype(F)


def sample(volume, lo, hi, points):
    """Trilinear (M, 4): along x first, then y, then z; v0 + f (v1 - v0) as subtract, multiply, add."""
    v, p = np.asarray(volume, F), np.asarray(points, F)
    n = v.shape[0]
    assert v.shape == (n, n, n, 4) and 2 <= n
    lo, step = np.asarray(lo, F), lattice_step(lo, hi, n)
    ix, fx = _cell(p[:, 0], lo[0], step[0], n)
    iy, fy = _cell(p[:, 1], lo[1], step[1], n)
    iz, fz = _cell(p[:, 2], lo[2], step[2], n)
    assert min(ix.min(), iy.min(), iz.min()) >= 0 and max(ix.max(), iy.max(), iz.max()) <= n - 2
    fx, fy, fz = fx[:, None], fy[:, None], fz[:, None]
    v00 = _lerp(v[iz, iy, ix], v[iz, iy, ix + 1], fx)
    v10 = _lerp(v[iz, iy + 1, ix], v[iz, iy + 1, ix + 1], fx)
    v01 = _lerp(v[iz + 1, iy, ix], v[iz + 1, iy, ix + 1], fx)
    v11 = _lerp(v[iz + 1, iy + 1, ix], v[iz + 1, iy + 1, ix + 1], fx)
    return _lerp(_lerp(v00, v10, fy), _lerp(v01, v11, fy), fz)


def march(volume, lo, hi, near, far, rays_orig, rays_dirs, n_steps, t_min=0.0, exp=None):
    """-> (rgb (N, 3), depth (N,), opacity (N,)) float32.  ``exp``: a float32 -> float32 stand-in for expf (default np.exp in
    float32), so a test can push every exponential one ulp either way."""
    o, d = np.asarray(rays_orig, F), np.asarray(rays_dirs, F)
    exp = exp or (lambda x: np.exp(x.astype(F)).astype(F))
    a, b, hit, _ = ray_box_interval(o, d, lo, hi, near, far)
    hit = hit & np.isfinite(o[:, :3]).all(axis=1) & np.isfinite(d[:, :3]).all(axis=1)
    n = o.shape[0]
    rgb, depth, T = np.zeros((n, 3), F), np.zeros(n, F), np.ones(n, F)
    alive = hit.copy()
    t_min = F(t_min)
    with np.errstate(all="ignore"):
        delta = ((b - a).astype(F) / F(n_steps)).astype(F)
        for k in range(n_steps):
            if not alive.any():
                break
            z = (a + ((F(k) + F(0.5)) * delta).astype(F)).astype(F)
            p = (o[:, :3] + (d[:, :3] * z[:, None]).astype(F)).astype(F)
            v = sample(volume, lo, hi, np.where(alive[:, None], p, F(0)))
            e = exp(-(v[:, 3] * delta).astype(F))
            alpha = (F(1) - e).astype(F)
            w = (alpha * T).astype(F)
            rgb = np.where(alive[:, None], (rgb + (w[:, None] * v[:, :3]).astype(F)).astype(F), rgb)
            depth = np.where(alive, (depth + (w * z).astype(F)).astype(F), depth)
            T = np.where(alive, (T * (F(1) - alpha).astype(F)).astype(F), T)
            alive = alive & ~(T < t_min)
    return rgb, depth, (F(1) - T).astype(F)


# ---- the media, rays and bar of tests/test_volume_host.py and tests/test_gpu_volume.py -------------------------------------------
def march_bar(n_steps):
    """(n_steps + 4) 2^-23 on rgb and opacity (times far on depth): a step adds about four roundings of quantities bounded
    by 1 and one expf ulp."""
    return (n_steps + 4) * 2.0 ** -23


def rays_through_box(n, seed):
    """Origins on the sphere of radius 4, aimed at points of the box: every ray hits between the tests' bounds 2 and 6."""
    rng = np.random.default_rng(seed)
    g = rng.normal(size=(n, 3))
    o = 4.0 * g / np.linalg.norm(g, axis=1, keepdims=True)
    t = rng.uniform(np.array(LO) * 0.8, np.array(HI) * 0.8, size=(n, 3))
    d = (t - o) / np.linalg.norm(t - o, axis=1, keepdims=True)
    o4 = np.concatenate([o, np.ones((n, 1))], axis=1).astype(F)
    d4 = np.concatenate([d, np.zeros((n, 1))], axis=1).astype(F)
    return o4, d4


def random_volume(n, seed, sigma_scale=3.0):
    rng = np.random.default_rng(seed)
    v = rng.random((n, n, n, 4), dtype=F)
    v[..., 3] = (v[..., 3] * F(sigma_scale)).astype(F)
    v[..., 3][rng.random((n, n, n)) < 0.3] = 0.0        # empty vertices, as after the ReLU
    return v
