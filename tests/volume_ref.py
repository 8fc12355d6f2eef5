"""Test-side restatement of the radiance volume (include/nerf_mi355.h: nerf_radiance_lattice, nerf_volume_sample,
nerf_volume_march): the per-vertex camera directions of the bake, trilinear sampling and the march, in numpy float32 with the
kernels' operations in the kernels' order, every operation rounded on its own; np.exp in float32 stands for expf.  Imported
by tests/test_volume_host.py and tests/test_gpu_volume.py, and by tests/sh_volume_ref.py, which states the SH volume's vertex
value and leaves the cell, the lerps (``trilinear``) and the march (``march``) to this module; nothing here touches the library.

A volume is (n, n, n, 4) indexed [iz, iy, ix, channel] over a box (lo, hi): vertex i of axis a lies at lo_a + step_a i,
step_a = (hi_a - lo_a) / (n - 1)."""
import functools

import numpy as np

from isosurface_ref import lattice_points, lattice_step      # the density lattice's vertex positions: the volume's too
from scene_box_ref import ray_box_interval
import support as S

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


def trilinear(volume, lo, hi, points, vertex):
    """The scaffolding of both formats' samplers -> (M, 4): the cell of every point, ``vertex(texels (M, C)) -> (M, 4)`` at its
    eight vertices, and the lerps along x first, then y, then z; v0 + f (v1 - v0) as subtract, multiply, add."""
    v, p = np.asarray(volume, F), np.asarray(points, F)
    n = v.shape[0]
    assert v.shape[:3] == (n, n, n) and 2 <= n
    lo, step = np.asarray(lo, F), lattice_step(lo, hi, n)
    ix, fx = _cell(p[:, 0], lo[0], step[0], n)
    iy, fy = _cell(p[:, 1], lo[1], step[1], n)
    iz, fz = _cell(p[:, 2], lo[2], step[2], n)
    assert min(ix.min(), iy.min(), iz.min()) >= 0 and max(ix.max(), iy.max(), iz.max()) <= n - 2
    fx, fy, fz = fx[:, None], fy[:, None], fz[:, None]
    v00 = _lerp(vertex(v[iz, iy, ix]), vertex(v[iz, iy, ix + 1]), fx)
    v10 = _lerp(vertex(v[iz, iy + 1, ix]), vertex(v[iz, iy + 1, ix + 1]), fx)
    v01 = _lerp(vertex(v[iz + 1, iy, ix]), vertex(v[iz + 1, iy, ix + 1]), fx)
    v11 = _lerp(vertex(v[iz + 1, iy + 1, ix]), vertex(v[iz + 1, iy + 1, ix + 1]), fx)
    return _lerp(_lerp(v00, v10, fy), _lerp(v01, v11, fy), fz)


def sample(volume, lo, hi, points):
    """Trilinear (M, 4) of an (n, n, n, 4) volume: a vertex's value is its texel."""
    assert np.ndim(volume) == 4 and np.shape(volume)[3] == 4
    return trilinear(volume, lo, hi, points, lambda texels: texels)


def march(volume, lo, hi, near, far, rays_orig, rays_dirs, n_steps, t_min=0.0, exp=None, value=None):
    """-> (rgb (N, 3), depth (N,), opacity (N,)) float32.  ``exp``: a float32 -> float32 stand-in for expf (default np.exp in
    float32), so a test can push every exponential one ulp either way.  ``value(points (N, 3), alive (N,)) -> (N, 4)``: the
    volume at every ray's point of one step (default: ``sample``); ``alive`` marks the rays that composite it."""
    o, d = np.asarray(rays_orig, F), np.asarray(rays_dirs, F)
    exp = exp or (lambda x: np.exp(x.astype(F)).astype(F))
    value = value or (lambda p, alive: sample(volume, lo, hi, p))
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
            v = value(np.where(alive[:, None], p, F(0)), alive)
            e = exp(-(v[:, 3] * delta).astype(F))
            alpha = (F(1) - e).astype(F)
            w = (alpha * T).astype(F)
            rgb = np.where(alive[:, None], (rgb + (w[:, None] * v[:, :3]).astype(F)).astype(F), rgb)
            depth = np.where(alive, (depth + (w * z).astype(F)).astype(F), depth)
            T = np.where(alive, (T * (F(1) - alpha).astype(F)).astype(F), T)
            alive = alive & ~(T < t_min)
    return rgb, depth, (F(1) - T).astype(F)


# ---- the media, points, rays and bar of the volume tests, plain and SH, host and device -------------------------------------------
NEAR, FAR = 0.5, 4.5            # the device tests' context: rays from the radius-4 sphere enter near 3 and some leave past 4.5
same_f32 = functools.partial(S.assert_same_bits, dtype=F)      # what the library returns is float32 already


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


def sample_points(n, m=257, seed=0):
    """Vertices, points on faces, points outside on every side, NaN and +-Inf coordinates, and random points in and around the
    box -> ((m, 3), which have a NaN)."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(LO, F), np.array(HI, F)
    vertices = lattice_points(LO, HI, n)
    vertices = vertices[rng.permutation(len(vertices))[:32]]
    inner = rng.uniform(lo, hi, (32, 3)).astype(F)
    faces = inner.copy()
    for k in range(len(faces)):
        faces[k, k % 3] = (lo, hi)[(k // 3) % 2][k % 3]
    outside = inner[:12].copy()
    for k in range(12):
        outside[k, k % 3] = (lo - F(0.5 + k), hi + F(0.25 + k))[(k // 3) % 2][k % 3]
    odd = np.array([[np.nan, 0, 0], [0, np.nan, 0], [0, 0, np.nan], [np.nan, np.nan, np.nan], [np.inf, 0, 0], [0, -np.inf, 0],
                    [0, 0, np.inf], [-np.inf, np.inf, -np.inf], [3e38, -3e38, 0]], F)
    fixed = np.concatenate([vertices, faces, outside, odd])
    rest = rng.uniform(lo - F(0.3), hi + F(0.3), (m - len(fixed), 3)).astype(F)
    p = np.concatenate([fixed, rest])
    return p, np.isnan(p).any(axis=1)


def march_rays(n_rays, seed):
    """Hits from the radius-4 sphere (some leave past FAR), origins inside the box and close to it (cut by NEAR), misses, rays
    with a direction component exactly 0 inside and outside that slab, one NaN ray, every fifth direction un-normalised
    -> (o, d)."""
    rng = np.random.default_rng(seed)
    special_o = np.array([[0.2, -0.3, 0.1, 1], [0.0, 0.1, 0.3, 1], [0.5, 0.2, 1.6, 1],       # inside, inside, just outside
                          [3.0, 0.0, 4.0, 1], [0.0, 0.0, 4.0, 1], [0.0, 0.0, -4.0, 1],       # three misses
                          [0.3, 0.2, 4.0, 1], [1.5, 0.2, 4.0, 1], [0.3, 0.2, 4.0, 1],        # d_x = d_y = 0: in, out, -0.0
                          [np.nan, 0.0, 4.0, 1]], F)
    special_d = np.array([[0.3, 0.5, -0.8, 0], [-1, 0, 0, 0], [0.0, 0.1, -1, 0],
                          [0, 0, -1, 0], [0, 0, 1, 0], [0, 0, -1, 0],
                          [0, 0, -1, 0], [0, 0, -1, 0], [-0.0, -0.0, -1, 0],
                          [0, 0, -1, 0]], F)
    o, d = rays_through_box(n_rays - len(special_o), seed)
    d[::5] *= F(1.7)                                                          # un-normalised directions
    order = rng.permutation(n_rays)
    return np.concatenate([o, special_o])[order], np.concatenate([d, special_d])[order]


def random_volume(n, seed, sigma_scale=3.0):
    rng = np.random.default_rng(seed)
    v = rng.random((n, n, n, 4), dtype=F)
    v[..., 3] = (v[..., 3] * F(sigma_scale)).astype(F)
    v[..., 3][rng.random((n, n, n)) < 0.3] = 0.0        # empty vertices, as after the ReLU
    return v
