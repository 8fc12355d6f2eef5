"""Test-side restatements of the ray and sampling space: the disparity-linear coarse depths and the
NDC ray transform in float64 (what the kernels are held to), the same two in float32 with the kernels' operation order
(what the CPU oracle is fed, through the entries it already has for given rays and depths), the error bars derived from
the operation counts, and the forward-facing poses of the golden LLFF rig.  Imported by tests/test_sampling_space_host.py
and tests/test_gpu_sampling_space.py; nothing here touches the library."""
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U = 2.0 ** -24                       # unit roundoff of fp32 (round to nearest)
U_BELOW_ONE = np.nextafter(F32(1), F32(0))


def tan_half(fov) -> np.float32:
    """The raygen's tangent (oracle.get_rays_directions): tan of fp32(fov / 2), evaluated in double, rounded once."""
    return F32(math.tan(float(F32(fov / 2))))


def ndc_scale(fov) -> np.float32:
    """k = 1 / tan_half for BOTH axes (one tangent, no aspect term), inverted in double and rounded once."""
    return F32(1.0 / float(tan_half(fov)))


# ---- disparity-linear depths -------------------------------------------------------------------------------------------
def lindisp_f64(near, far, u) -> np.ndarray:
    """z = 1 / (1/near + (1/far - 1/near) (s + u) / S) in float64; u (..., S)."""
    u = np.asarray(u, np.float64)
    s_count = u.shape[-1]
    t = (np.arange(s_count, dtype=np.float64) + u) / s_count
    return 1.0 / (1.0 / near + (1.0 / far - 1.0 / near) * t)


def lindisp_bar(near, far) -> float:
    """|dz| / z <= 6 * 2^-24 * far / near.  The denominator D = 1/near + (1/far - 1/near) t lies in (1/far, 1/near].  Each
    fp32 rounding on the way to it (of 1/near, of 1/far - 1/near, of s + u, of the division by S, of the product, of the
    sum) moves D by at most 2^-24 / near, i.e. by at most 2^-24 far / near of D, and z = 1 / D moves by the same relative
    amount; the final division adds 2^-24 <= 2^-24 far / near.  s + u held just below s + 1 (the kernel's guard for
    u = 1 - 2^-24) is off by less than two roundings of s + u.  For the bounds tested here (powers of two) 1/near and
    1/far - 1/near are exact, which leaves at most six."""
    return 6 * U * far / near


def lindisp_f32(near, far, u) -> np.ndarray:
    """The kernel's arithmetic in numpy float32, same order, same guards."""
    u = np.asarray(u, F32)
    s_count = u.shape[-1]
    s = np.arange(s_count, dtype=F32)
    inv_near, dinv = F32(1.0 / float(near)), F32(1.0 / float(far) - 1.0 / float(near))
    v = s + u
    v = np.where(v >= s + F32(1), np.nextafter(s + F32(1), F32(0)), v).astype(F32)
    t = v / F32(s_count)
    z = F32(1) / (inv_near + dinv * t)
    return np.minimum(np.maximum(z, F32(near)), np.nextafter(F32(far), F32(near))).astype(F32)


# ---- NDC rays ----------------------------------------------------------------------------------------------------------
def _ndc(o, d, n, k, one, two):
    tn = -((n + o[..., 2]) / d[..., 2])
    px, py, pz = o[..., 0] + tn * d[..., 0], o[..., 1] + tn * d[..., 1], o[..., 2] + tn * d[..., 2]
    rx, ry, e = px / pz, py / pz, (two * n) / pz
    sx, sy = d[..., 0] / d[..., 2], d[..., 1] / d[..., 2]
    oo = np.stack([-(k * rx), -(k * ry), one + e, o[..., 3]], axis=-1)
    dd = np.stack([-(k * (sx - rx)), -(k * (sy - ry)), -e, d[..., 3]], axis=-1)
    return oo, dd, np.stack([px, py, pz], axis=-1)


def rays_to_ndc_f64(o, d, fov, n):
    """-> (o', d', p): the NDC rays and the origin shifted onto the near plane, float64, from the fp32 inputs and the fp32 k."""
    return _ndc(np.asarray(o, np.float64), np.asarray(d, np.float64), float(F32(n)), float(ndc_scale(fov)), 1.0, 2.0)


def rays_to_ndc_f32(o, d, fov, n):
    """The kernel's arithmetic in numpy float32 (same operations in the same order, nothing contracted)."""
    oo, dd, _ = _ndc(np.asarray(o, F32), np.asarray(d, F32), F32(n), ndc_scale(fov), F32(1), F32(2))
    return oo.astype(F32), dd.astype(F32)


def ndc_bars(o, d, fov, n):
    """Absolute bars (multiples of 2^-24 max(1, |value|)) per component of o' and d', from the operation count of each.

    First order in u = 2^-24, every fp32 operation within u of exact (relative).  With a = n + o_z, A = max |a| / n,
    sigma = max |d_x / d_z|, |d_y / d_z|, k = 1 / tan_half and O = max |o'_x|, |o'_y| over the rays at hand:
      tn = -a / d_z               add, divide:   2u
      q_c = tn d_c                multiply:      3u                      (|q_z| = |a|, |q_x| = |a| |d_x / d_z| <= n A sigma)
      p_c = o_c + q_c             add:           |dp_c| <= u (3 |q_c| + |p_c|);   p_z = -n, so dp_z / p_z <= u (3A + 1)
      r_x = p_x / p_z             divide:        |dr_x| <= u ((3A + 3) |r_x| + 3 A sigma)
      o'_x = -k r_x               multiply:      |do'_x| <= u ((3A + 4) |o'_x| + 3 k A sigma)
      e = 2n / p_z  (|e| = 2)     divide:        |de| <= 2u (3A + 2);  d'_z = -e
      o'_z = 1 + e  (|o'_z| = 1)  add:           |do'_z| <= u (6A + 5)
      s_x = d_x / d_z             divide:        u sigma
      g_x = s_x - r_x             subtract;  d'_x = -k g_x  multiply:
                                                 |dd'_x| <= u (2 |d'_x| + k sigma (1 + 3A) + (3A + 3) O)
    Each multiple gets + 1 for the second-order terms (u^2 times the squares of these multiples: far below one u).
    -> dict of multiples: "oxy", "oz", "dxy", "dz"."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    n, k = float(F32(n)), float(ndc_scale(fov))
    a_cond = float(np.abs(n + o[..., 2]).max() / n)
    sigma = float(np.abs(d[..., :2] / d[..., 2:3]).max())
    oo, _, _ = rays_to_ndc_f64(o, d, fov, n)
    o_max = float(np.abs(oo[..., :2]).max())
    return {"oxy": (3 * a_cond + 4) + 3 * k * a_cond * sigma + 1,
            "oz": 6 * a_cond + 5 + 1,
            "dxy": 2 + k * sigma * (1 + 3 * a_cond) + (3 * a_cond + 3) * o_max + 1,
            "dz": 6 * a_cond + 4 + 1}


def within(got, want, multiple) -> bool:
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all(np.abs(got - want) <= multiple * U * np.maximum(1.0, np.abs(want))))


# ---- poses -------------------------------------------------------------------------------------------------------------
def forward_facing_poses(count=3):
    """The ``count`` cameras of the golden LLFF rig (tests/golden/alexander50/poses_bounds.npy, recentred and scaled as the
    loader does, without decoding the images) whose viewing axis is closest to the world's -z: cameras look down -z in their
    own frame, and for these the world-space d_z of every pixel ray is far from 0.  -> (c2w (count,4,4) fp32, fov)."""
    from nerf_and_dietnerf_amd import datasets as D
    table = np.load(os.path.join(ROOT, "tests", "golden", "alexander50", D.POSES_BOUNDS_NPY), allow_pickle=False)
    llff = table[:, :15].reshape(-1, 3, 5)
    poses = np.concatenate([llff[:, :, 1:2], -llff[:, :, 0:1], llff[:, :, 2:]], axis=2)
    poses, _ = D.recenter_poses(poses)
    poses, _, _ = D.spherify_poses(poses, table[:, 15:].copy())
    _, width, focal = poses[0, :, 4]
    pick = np.argsort(-poses[:, 2, 2])[:count]               # the viewing axis is -R[:, 2]: most negative z first
    rig = np.zeros((count, 4, 4), np.float32)
    rig[:, :3, :] = poses[pick][:, :, :4]
    rig[:, 3, 3] = 1.0
    return rig, float(2.0 * np.arctan2(width / 2.0, focal))


def world_rays(oracle, c2w, fov, h, w):
    """(h*w,4) origins and directions of one camera, from the CPU oracle's raygen."""
    d = oracle.get_rays_directions(h, w, fov, c2w).reshape(-1, 4)
    return np.tile(np.asarray(c2w, F32)[:, 3], (h * w, 1)).astype(F32), np.ascontiguousarray(d)
