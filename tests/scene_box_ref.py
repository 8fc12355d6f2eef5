"""Test-side restatement of the scene bounding box ("Scene box"): the ray / box interval and the
coarse depths a narrowed ray draws, in numpy float32 with the kernels' operations in the kernels' order, every operation
rounded on its own.  Imported by tests/test_scene_box_host.py and tests/test_gpu_scene_box.py; nothing here touches the
library.

For a ray (o, d) depths are the parameter t of o + t d; d is not normalised.
  1. per axis with d_a != 0: t0 = (lo_a - o_a) / d_a, t1 = (hi_a - o_a) / d_a, axis interval [min, max]
  2. per axis with d_a == 0 (either zero): no constraint if lo_a <= o_a <= hi_a, otherwise the ray misses
  3. tn = largest lower end, tf = smallest upper end; a = max(tn, near), b = min(tf, far)
  4. hit: no axis missed and b > a; narrowed: hit and (a > near or b < far)
  5. a narrowed ray draws the mode's own formula on [a, b] with float32 constants of its own
  6. any other ray draws with the constants of a context without a box"""
import numpy as np

F32 = np.float32
U = 2.0 ** -24

# the issue's box and bounds
LO = np.array([-1.0, -0.75, -0.5], F32)
HI = -LO
NEAR, FAR = 2.0, 6.0

# (origin, direction, category, expected interval or None for a miss) on LO / HI at NEAR / FAR
EDGE_RAYS = [
    ((0, 0, 4), (0, 0, -1), "through", (3.5, 4.5)),
    ((2, 0, 4), (0, 0, -1), "parallel_outside", None),
    ((1, 0, 4), (0, 0, -1), "on_the_face", (3.5, 4.5)),
    ((0, 0, 0), (0, 0, -1), "origin_inside", None),              # tf = 0.5 < near
    ((0, 0, -4), (0, 0, -1), "box_behind", None),
    ((0, 0, 4), (0, 0, -0.25), "beyond_far", None),              # tn = 14 > far
    ((0, 0, 4), (-0.0, -0.0, -1), "negative_zero", (3.5, 4.5)),
]


def edge_rays():
    """-> (o (7,4), d (7,4)) homogeneous rows, origin w = 1, direction w = 0."""
    o = np.array([list(r[0]) + [1.0] for r in EDGE_RAYS], F32)
    d = np.array([list(r[1]) + [0.0] for r in EDGE_RAYS], F32)
    return o, d


def ray_box_interval(o, d, lo, hi, near, far):
    """Steps 1-4 -> (a, b, hit, narrowed), float32 / bool (N,).  min and max are written as the comparisons the device
    function makes, so nothing depends on how a library's min / max treats NaN or the sign of zero."""
    o, d = np.asarray(o, F32), np.asarray(d, F32)
    lo, hi = np.asarray(lo, F32), np.asarray(hi, F32)
    near, far = F32(near), F32(far)
    n = o.shape[0]
    tn, tf = np.full(n, -np.inf, F32), np.full(n, np.inf, F32)
    miss = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for ax in range(3):
            oa, da = o[:, ax], d[:, ax]
            zero = da == 0
            den = np.where(zero, F32(1), da)
            t0 = ((lo[ax] - oa) / den).astype(F32)
            t1 = ((hi[ax] - oa) / den).astype(F32)
            first = t0 < t1
            low, high = np.where(first, t0, t1), np.where(first, t1, t0)
            miss |= zero & ~((lo[ax] <= oa) & (oa <= hi[ax]))
            tn = np.where(~zero & (low > tn), low, tn)
            tf = np.where(~zero & (high < tf), high, tf)
    a = np.where(tn > near, tn, near).astype(F32)
    b = np.where(tf < far, tf, far).astype(F32)
    hit = ~miss & (b > a)
    narrowed = hit & ((a > near) | (b < far))
    return a, b, hit, narrowed


def ray_box_bounds(o, d, lo, hi, near, far):
    """What nerf_ray_box_bounds returns: bounds (N,2) = (a, b) of a narrowed ray and (near, far) of any other, narrowed (N,) int32."""
    a, b, _, narrowed = ray_box_interval(o, d, lo, hi, near, far)
    bounds = np.stack([np.where(narrowed, a, F32(near)), np.where(narrowed, b, F32(far))], axis=1).astype(F32)
    return bounds, narrowed.astype(np.int32)


def _linear(start, stop, delta, span, u):
    s_count = u.shape[1]
    lin = (start[:, None] + (delta[:, None] * np.arange(s_count, dtype=F32)[None, :]).astype(F32)).astype(F32)
    lin[:, 0] = start
    if s_count > 1:
        lin[:, -1] = stop
    return (lin + ((u * span[:, None]).astype(F32) / F32(s_count)).astype(F32)).astype(F32)


def _lindisp(low, high_below, inv_near, dinv, u):
    s_count = u.shape[1]
    s = np.arange(s_count, dtype=F32)[None, :]
    v = (s + u).astype(F32)
    v = np.where(v >= s + F32(1), np.nextafter(s + F32(1), F32(0)), v).astype(F32)
    t = (v / F32(s_count)).astype(F32)
    z = (F32(1) / (inv_near[:, None] + (dinv[:, None] * t).astype(F32)).astype(F32)).astype(F32)
    return np.minimum(np.maximum(z, low[:, None]), high_below[:, None]).astype(F32)


def z_values(o, d, lo, hi, near, far, u, lindisp=False):
    """Steps 5-6: the coarse depths (N,S) of a context with the box (lo, hi); lo = None: a context without one."""
    u = np.asarray(u, F32)
    n, s_count = u.shape
    near32, far32 = F32(near), F32(far)
    if lo is None:
        a, b, narrowed = np.full(n, near32), np.full(n, far32), np.zeros(n, bool)
    else:
        a, b, _, narrowed = ray_box_interval(o, d, lo, hi, near, far)
    a, b = np.where(narrowed, a, near32).astype(F32), np.where(narrowed, b, far32).astype(F32)
    with np.errstate(all="ignore"):
        if lindisp:
            # the host's constants: double, rounded once; a ray's own: float32, every operation rounded
            inv_near_h, dinv_h = F32(1.0 / float(near)), F32(1.0 / float(far) - 1.0 / float(near))
            inv_a = (F32(1) / a).astype(F32)
            dinv_r = ((F32(1) / b).astype(F32) - inv_a).astype(F32)
            below = np.where(narrowed, np.nextafter(b, F32(-np.inf)), np.nextafter(far32, near32)).astype(F32)
            return _lindisp(a, below, np.where(narrowed, inv_a, inv_near_h).astype(F32),
                            np.where(narrowed, dinv_r, dinv_h).astype(F32), u)
        delta_h = (far32 - near32) / F32(s_count - 1) if s_count > 1 else F32(0)
        span_h = F32(float(far) - float(near))
        span_r = (b - a).astype(F32)
        delta_r = (span_r / F32(s_count - 1)).astype(F32) if s_count > 1 else np.zeros(n, F32)
        return _linear(a, b, np.where(narrowed, delta_r, delta_h).astype(F32), np.where(narrowed, span_r, span_h).astype(F32), u)


def lindisp_f64(a, b, u):
    """z = 1 / (1/a + (1/b - 1/a) (s + u) / S) in float64 on the float32 (a, b) of every ray; u (N,S)."""
    a, b, u = np.asarray(a, np.float64)[:, None], np.asarray(b, np.float64)[:, None], np.asarray(u, np.float64)
    t = (np.arange(u.shape[1], dtype=np.float64)[None, :] + u) / u.shape[1]
    return 1.0 / (1.0 / a + (1.0 / b - 1.0 / a) * t)


def lindisp_bar(a, b):
    """|dz| / z <= 9 * 2^-24 * b / a per ray, derived as sampling_space_ref.lindisp_bar derives its six: the denominator
    D = 1/a + (1/b - 1/a) t lies in [1/b, 1/a], and every float32 rounding on the way to it moves it by at most 2^-24 / a,
    that is by 2^-24 b / a of D; z = 1 / D moves by the same relative amount.  There the six are: s + u, the division by S,
    the product, the sum, the final division, and one more for s + u held just below s + 1 -- the bounds are powers of two,
    so 1/near and 1/far - 1/near are exact.  Here a and b are arbitrary and three more roundings count: 1/a (it enters D
    as (1 - t) / a: at most 2^-24 / a), 1/b (2^-24 t / b) and their difference (2^-24 t |1/b - 1/a|): 6 + 3 = 9."""
    return 9 * U * np.asarray(b, np.float64) / np.asarray(a, np.float64)


def recipe_rays(seed=5, n=130):
    """The issue's rays: origins 4 * unit(normal), directions unit(target - o) with targets uniform in [-1.6, 1.6]^3, then the
    seven edge rays -> (o (n+7,4), d (n+7,4))."""
    rng = np.random.default_rng(seed)
    g = rng.normal(size=(n, 3))
    o = 4.0 * g / np.linalg.norm(g, axis=1, keepdims=True)
    t = rng.uniform(-1.6, 1.6, size=(n, 3))
    d = (t - o) / np.linalg.norm(t - o, axis=1, keepdims=True)
    o4 = np.concatenate([o, np.ones((n, 1))], axis=1).astype(F32)
    d4 = np.concatenate([d, np.zeros((n, 1))], axis=1).astype(F32)
    eo, ed = edge_rays()
    return np.concatenate([o4, eo]), np.concatenate([d4, ed])
