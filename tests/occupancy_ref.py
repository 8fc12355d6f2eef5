"""Test-side restatement of the occupancy grid ("Occupancy grid"; include/nerf_mi355.h:
nerf_ctx_set_occupancy_grid has the rule): the walk of a ray through the cells of its box interval and the coarse depths it
then draws, in numpy with the kernels' operations in the kernels' order, vectorised over rays.  ``dtype=F32`` rounds every
operation on its own, as the device function does; ``dtype=F64`` is the same walk in float64 on the same float32 inputs, the
reference the float32 walk is judged against.  Imported by tests/test_occupancy_host.py and tests/test_gpu_occupancy.py;
nothing here touches the library.

A grid is a bool array (R, R, R) indexed [ix, iy, iz]; cell (ix, iy, iz) is bit ix + R (iy + R iz) of the packed words.
  1. (a0, b0) = steps 1-3 of the box rule (scene_box_ref); no hit -> the ray is untouched
  2. cell_a = (hi_a - lo_a) / R; start cell = clamp(floor(((o_a + a0 d_a) - lo_a) / cell_a), 0, R - 1)
  3. plane k of an axis lies at ((lo_a + cell_a k) - o_a) / d_a, recomputed from k at every step; d_a == 0 never steps
  4. walk from t = a0: next axis = smallest plane parameter tm (ties: lowest axis, strict <); segment [t, te], te = tm held
     in [t, b0]; an occupied cell sets a' = t the first time, b' = te every time; stop when not tm < b0, when the stepped
     index leaves the grid, or after 3R + 3 steps
  5. occupied cell met, b' > a', and a' > a0 or b' < b0: narrowed by the grid to [a', b'] (state 2)
  6. otherwise what the box alone gives: (a0, b0) if the box narrows the ray (state 1), (near, far) if not (state 0)"""
import numpy as np

import scene_box_ref as B

F32, F64 = np.float32, np.float64

# the issue's scene: the box [-1, 1]^3, two balls on a 16^3 grid, rays from the radius-4 sphere, near 2, far 6
LO = np.array([-1.0, -1.0, -1.0], F32)
HI = -LO
NEAR, FAR = 2.0, 6.0
BALLS = (((-0.4, -0.3, 0.2), 0.35), ((0.45, 0.3, -0.25), 0.3))


def cell_centres(lo, hi, r):
    """(R, R, R, 3) float32 centres lo_a + cell_a (i_a + 0.5), indexed [ix, iy, iz]: grid_points_kernel's point 0."""
    lo, hi = np.asarray(lo, F32), np.asarray(hi, F32)
    cell = ((hi - lo) / F32(r)).astype(F32)
    i = (np.arange(r, dtype=F32) + F32(0.5)).astype(F32)
    ax = [(lo[a] + (cell[a] * i).astype(F32)).astype(F32) for a in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).astype(F32)


def centres_in_bit_order(lo, hi, r):
    """(R^3, 3): row c is the centre of the cell whose bit is c."""
    return np.ascontiguousarray(cell_centres(lo, hi, r).transpose(2, 1, 0, 3).reshape(-1, 3))


def two_balls(r=16, lo=LO, hi=HI):
    c = cell_centres(lo, hi, r).astype(F64)
    g = np.zeros((r, r, r), bool)
    for centre, radius in BALLS:
        g |= ((c - np.array(centre)) ** 2).sum(-1) <= radius ** 2
    return g


def sphere_rays(n=4096, seed=11, radius=4.0, half=1.2):
    """Origins radius * unit(normal), directions unit(target - o), targets uniform in [-half, half]^3 -> (o (n,4), d (n,4))."""
    rng = np.random.default_rng(seed)
    g = rng.normal(size=(n, 3))
    o = radius * g / np.linalg.norm(g, axis=1, keepdims=True)
    t = rng.uniform(-half, half, size=(n, 3))
    d = (t - o) / np.linalg.norm(t - o, axis=1, keepdims=True)
    return (np.concatenate([o, np.ones((n, 1))], axis=1).astype(F32),
            np.concatenate([d, np.zeros((n, 1))], axis=1).astype(F32))


def pack_bits(grid):
    """(R, R, R) bool [ix, iy, iz] -> R^3 / 32 little-endian uint32 words, written out bit by bit."""
    g = np.asarray(grid, bool)
    r = g.shape[0]
    words = np.zeros(r ** 3 // 32, np.uint32)
    ix, iy, iz = np.nonzero(g)
    bit = ix + r * (iy + r * iz)
    np.bitwise_or.at(words, bit >> 5, (np.uint32(1) << (bit & 31).astype(np.uint32)))
    return words


def dilate26(grid):
    """One step of 26-neighbour growth of an (R, R, R) bool array."""
    g = np.asarray(grid, bool)
    r = g.shape[0]
    p = np.zeros((r + 2,) * 3, bool)
    p[1:-1, 1:-1, 1:-1] = g
    out = np.zeros_like(g)
    for dx in range(3):
        for dy in range(3):
            for dz in range(3):
                out |= p[dx:dx + r, dy:dy + r, dz:dz + r]
    return out


def box_interval(o, d, lo, hi, near, far, dtype=F32):
    """Steps 1-3 of the box rule in ``dtype`` -> (a0, b0, hit, box_narrowed); for F32 these are scene_box_ref's operations."""
    T = dtype
    o, d = np.asarray(o, F32)[:, :3].astype(T), np.asarray(d, F32)[:, :3].astype(T)
    lo, hi = np.asarray(lo, F32).astype(T), np.asarray(hi, F32).astype(T)
    near, far = T(F32(near)), T(F32(far))
    n = o.shape[0]
    tn, tf = np.full(n, -np.inf, T), np.full(n, np.inf, T)
    miss = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for ax in range(3):
            oa, da = o[:, ax], d[:, ax]
            zero = da == 0
            den = np.where(zero, T(1), da)
            t0 = ((lo[ax] - oa) / den).astype(T)
            t1 = ((hi[ax] - oa) / den).astype(T)
            first = t0 < t1
            low, high = np.where(first, t0, t1), np.where(first, t1, t0)
            miss |= zero & ~((lo[ax] <= oa) & (oa <= hi[ax]))
            tn = np.where(~zero & (low > tn), low, tn)
            tf = np.where(~zero & (high < tf), high, tf)
    a = np.where(tn > near, tn, near).astype(T)
    b = np.where(tf < far, tf, far).astype(T)
    hit = ~miss & (b > a)
    return a, b, hit, hit & ((a > near) | (b < far))


def ray_grid_interval(o, d, lo, hi, near, far, grid, dtype=F32):
    """-> (a, b, state, hit): the bounds every ray draws on, in ``dtype``; state int32 0 / 1 / 2; hit bool (the box rule's)."""
    T = dtype
    grid = np.asarray(grid, bool)
    r = grid.shape[0]
    a0, b0, hit, box_narrowed = box_interval(o, d, lo, hi, near, far, T)
    o, d = np.asarray(o, F32)[:, :3].astype(T), np.asarray(d, F32)[:, :3].astype(T)
    lo, hi = np.asarray(lo, F32).astype(T), np.asarray(hi, F32).astype(T)
    n = o.shape[0]
    zero, pos = d == 0, d > 0
    den = np.where(zero, T(1), d)
    step = np.where(pos, 1, -1).astype(np.int64)
    with np.errstate(all="ignore"):
        cell = ((hi - lo) / T(r)).astype(T)
        p = (o + (a0[:, None] * d).astype(T)).astype(T)
        f = np.floor(((p - lo).astype(T) / cell).astype(T))
        idx = np.where(f >= 0, np.where(f <= r - 1, f, r - 1), 0).astype(np.int64)          # NaN -> 0

        def planes(k):
            t = (((lo + (cell * k.astype(T)).astype(T)).astype(T) - o).astype(T) / den).astype(T)
            return np.where(zero, T(np.inf), t).astype(T)

        plane = idx + pos
        tp = planes(plane)
        t = a0.copy()
        ga, gb = np.zeros(n, T), np.zeros(n, T)
        found = np.zeros(n, bool)
        active = hit.copy()
        axes = np.arange(3)[None, :]
        for _ in range(3 * r + 3):
            if not active.any():
                break
            ax, tm = np.zeros(n, np.int64), tp[:, 0]
            for k in (1, 2):
                less = tp[:, k] < tm
                ax, tm = np.where(less, k, ax), np.where(less, tp[:, k], tm)
            te = np.where(tm > b0, b0, tm)
            te = np.where(te < t, t, te)
            occ = grid[idx[:, 0], idx[:, 1], idx[:, 2]] & active
            ga = np.where(occ & ~found, t, ga)
            gb = np.where(occ, te, gb)
            found |= occ
            active &= tm < b0
            stepped = active[:, None] & (axes == ax[:, None])
            idx = idx + np.where(stepped, step, 0)
            plane = plane + np.where(stepped, step, 0)
            tp = np.where(stepped, planes(plane), tp)
            active &= ((idx >= 0) & (idx < r)).all(axis=1)
            idx = np.clip(idx, 0, r - 1)                   # (rays that left the grid are no longer read)
            t = np.where(active, te, t)
    by_grid = found & (gb > ga) & ((ga > a0) | (gb < b0))
    state = np.where(by_grid, 2, np.where(box_narrowed, 1, 0)).astype(np.int32)
    near, far = T(F32(near)), T(F32(far))
    a = np.where(by_grid, ga, np.where(box_narrowed, a0, near)).astype(T)
    b = np.where(by_grid, gb, np.where(box_narrowed, b0, far)).astype(T)
    return a, b, state, hit


def ray_occupancy_bounds(o, d, lo, hi, near, far, grid):
    """What nerf_ray_occupancy_bounds returns: bounds (N,2) float32, state (N,) int32."""
    a, b, state, _ = ray_grid_interval(o, d, lo, hi, near, far, grid, F32)
    return np.stack([a, b], axis=1).astype(F32), state


def kind(state, hit):
    """0: the ray misses the box, 1: it hits and meets no occupied cell, 2: the grid narrows it."""
    return np.where(state == 2, 2, np.where(hit, 1, 0))


def z_values(o, d, lo, hi, near, far, grid, u, lindisp=False):
    """The coarse depths (N,S) of a context with the box (lo, hi) and the grid: scene_box_ref.z_values' formulas on the grid's
    bounds (a ray of state 0 draws with the host's constants)."""
    u = np.asarray(u, F32)
    n, s_count = u.shape
    near32, far32 = F32(near), F32(far)
    a, b, state, _ = ray_grid_interval(o, d, lo, hi, near, far, grid, F32)
    own = state != 0
    with np.errstate(all="ignore"):
        if lindisp:
            inv_near_h, dinv_h = F32(1.0 / float(near)), F32(1.0 / float(far) - 1.0 / float(near))
            inv_a = (F32(1) / a).astype(F32)
            dinv_r = ((F32(1) / b).astype(F32) - inv_a).astype(F32)
            below = np.where(own, np.nextafter(b, F32(-np.inf)), np.nextafter(far32, near32)).astype(F32)
            return B._lindisp(a, below, np.where(own, inv_a, inv_near_h).astype(F32), np.where(own, dinv_r, dinv_h).astype(F32), u)
        delta_h = (far32 - near32) / F32(s_count - 1) if s_count > 1 else F32(0)
        span_h = F32(float(far) - float(near))
        span_r = (b - a).astype(F32)
        delta_r = (span_r / F32(s_count - 1)).astype(F32) if s_count > 1 else np.zeros(n, F32)
        return B._linear(a, b, np.where(own, delta_r, delta_h).astype(F32), np.where(own, span_r, span_h).astype(F32), u)


# (origin, direction, name) on the box [-1, 1]^3 at R = 4 (cells of 0.5), near 2, far 6; see test_occupancy_host.py for what
# each must give
HAND_RAYS = [
    ((0.25, 0.25, 4.0), (0, 0, -1), "through_cell_centres"),        # d = 0 on two axes
    ((0.5, 0.25, 4.0), (0, 0, -1), "along_a_cell_face"),            # x on the plane between cells 2 and 3
    ((-3.0, -3.0, 0.25), (1, 1, 0), "through_cell_corners"),        # d = 0 on one axis; x and y planes tie at every step
    ((0.25, 4.0, 0.25), (0, -1, 0), "axis_y"),
    ((0.25, 0.25, 0.25), (0, 0, -1), "origin_inside_box_ends_before_near"),
    ((0.25, 0.25, 0.25), (0, 0, -0.25), "origin_inside"),           # near = 2 -> z = -0.25 (cell 1), cell 0 from t = 3, out at t = 5
]


def hand_rays():
    o = np.array([list(r[0]) + [1.0] for r in HAND_RAYS], F32)
    d = np.array([list(r[1]) + [0.0] for r in HAND_RAYS], F32)
    return o, d


# ---- the scenes of tests/test_gpu_occupancy.py and tests/test_gpu_culling.py -----------------------------------------------------
NDC_NEAR = 0.5
NDC_BOX = ((-0.5, -0.4, -0.6), (0.5, 0.4, 0.4))            # NDC rays run from z = -1 (t = 0) to z = +1 (t = 1)
GOLDEN_BOX = ((-0.6, -0.4, -1.3), (0.4, 0.8, -0.4))        # around the golden scene's content, as seen from its cameras


def grid_for(r, lo, hi):
    """The two balls on an r^3 grid over (lo, hi), plus 3 % scattered cells (seeded by r)."""
    return two_balls(r, lo, hi) | (np.random.default_rng(r).random((r, r, r)) < 0.03)


def arm(ctx, lo, hi, near, far, grid):
    ctx.set_sampling("linear")
    ctx.set_bounds(near, far)
    ctx.set_scene_box(lo, hi)
    if grid is not None:
        ctx.set_occupancy_grid(grid)


def world_scene(n):
    """The six hand rays, then rays of the issue's recipe, n in all -> (o, d, lo, hi, near, far)."""
    ho, hd = hand_rays()
    o, d = sphere_rays(n - len(ho), seed=11)
    return np.concatenate([ho, o]), np.concatenate([hd, d]), LO, HI, NEAR, FAR


def ndc_scene(ctx, n=65 * 65):
    """The first n rays of a 65 x 65 image of a forward-facing camera through ctx.rays_to_ndc (4225 NDC rays), bounds 0 and 1."""
    import sampling_space_ref as R
    poses, fov = R.forward_facing_poses()
    c2w = poses[1]
    dirs = ctx.get_rays_directions(65, 65, fov, c2w).reshape(-1, 4)
    orig = np.tile(c2w[:, 3], (65 * 65, 1)).astype(np.float32)
    o, d = ctx.rays_to_ndc(orig, dirs, fov, NDC_NEAR)
    return (np.ascontiguousarray(o[:n]), np.ascontiguousarray(d[:n]), np.array(NDC_BOX[0], np.float32),
            np.array(NDC_BOX[1], np.float32), 0.0, 1.0)
