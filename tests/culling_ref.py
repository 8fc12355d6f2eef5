"""Test-side restatement of sample culling under an occupancy grid ("Sample culling";
include/nerf_mi355.h: nerf_ctx_set_sample_culling has the rule), in numpy with the device function's operations in its order,
vectorised over samples.  ``dtype=F32`` rounds every operation on its own, as the device does; ``dtype=F64`` is the same rule in
float64 on the same float32 inputs, the reference the float32 verdict is judged against.  Imported by
tests/test_culling_host.py and tests/test_gpu_culling.py; only culled_context, at the end, touches the library.

A grid is a bool array (R, R, R) indexed [ix, iy, iz].  For sample (ray, s):
  1. p_a = o_a + d_a z, multiply then add
  2. inside = lo_a <= p_a <= hi_a on all three axes (a NaN compares false: not inside)
  3. i_a = clamp(floor((p_a - lo_a) / cell_a), 0, R - 1), cell_a = (hi_a - lo_a) / R: the hi face belongs to cell R - 1, an
     interior cell face to the upper cell
  4. culled iff inside and the cell is empty; every other sample is kept (outside the box the grid knows nothing)"""
import numpy as np

import sampling_space_ref as R
from occupancy_ref import GOLDEN_BOX

F32, F64 = np.float32, np.float64


def sample_points(o, d, z, dtype=F32):
    """Step 1 -> (N, S, 3) in ``dtype``; for F32 these are the bits the network kernels form themselves."""
    T = dtype
    o, d = np.asarray(o, F32)[:, None, :3].astype(T), np.asarray(d, F32)[:, None, :3].astype(T)
    z = np.asarray(z, F32).astype(T)[:, :, None]
    with np.errstate(all="ignore"):
        return (o + (d * z).astype(T)).astype(T)


def sample_cells(o, d, z, lo, hi, r, dtype=F32):
    """Steps 1-3 -> (inside (N, S) bool, idx (N, S, 3) int64 in [0, R))."""
    T = dtype
    lo, hi = np.asarray(lo, F32).astype(T), np.asarray(hi, F32).astype(T)
    p = sample_points(o, d, z, T)
    with np.errstate(all="ignore"):
        inside = ((lo <= p) & (p <= hi)).all(axis=-1)
        cell = ((hi - lo) / T(r)).astype(T)
        f = np.floor(((p - lo).astype(T) / cell).astype(T))
        idx = np.where(f >= 0, np.where(f <= r - 1, f, r - 1), 0).astype(np.int64)      # NaN -> 0
    return inside, idx


def sample_keep(o, d, z, lo, hi, grid, dtype=F32):
    """The verdict (N, S) bool: True kept, False culled."""
    grid = np.asarray(grid, bool)
    inside, idx = sample_cells(o, d, z, lo, hi, grid.shape[0], dtype)
    return ~inside | grid[idx[..., 0], idx[..., 1], idx[..., 2]]


def zero_culled(raw, keep):
    """A copy of raw (N, S, C) -- or (N * S, C), or (N, S) -- with the rows of culled samples set to zero."""
    raw = np.array(raw, order="C", copy=True)
    k = np.asarray(keep, bool)
    raw.reshape(k.size, -1)[~k.ravel()] = 0           # a view of the fresh copy
    return raw


def scatter_rows(rows, keep, width=4):
    """Compact rows (M, width) of the kept samples, in ascending sample index -> (N, S, width) with zeros for the culled ones."""
    k = np.asarray(keep, bool)
    out = np.zeros(k.shape + (width,), F32)
    out[k] = np.asarray(rows, F32).reshape(-1, width)
    return out


# ---- hand cases: the box [-1, 1]^3 at R = 4 (cells of 0.5, every plane exact in float32) -----------------------------------------
HAND_LO, HAND_HI = np.array([-1.0, -1.0, -1.0], F32), np.array([1.0, 1.0, 1.0], F32)
HAND_O = np.array([[0.25, 0.25, 4.0, 1.0]], F32)
HAND_D = np.array([[0.0, 0.0, -1.0, 0.0]], F32)
# depth -> p_z = 4 - z: the hi face (1.0), the face between cells 2 and 3 (0.5), outside the box (1.5), NaN
HAND_Z = np.array([[3.0, 3.5, 2.5, np.nan]], F32)
HAND_CASES = [
    # (occupied cells, the verdicts of the four depths)
    ([(2, 2, 3)], [True, True, True, True]),          # the hi face belongs to cell 3, and so does the face between 2 and 3
    ([(2, 2, 2)], [False, False, True, True]),        # ... not to cell 2
    ([], [False, False, True, True]),                 # an empty grid still keeps what is outside the box, and a NaN
    ("full", [True, True, True, True]),
]


def hand_grids():
    """[(grid (4, 4, 4) bool, the four verdicts)]"""
    out = []
    for cells, want in HAND_CASES:
        g = np.ones((4, 4, 4), bool) if cells == "full" else np.zeros((4, 4, 4), bool)
        for c in ([] if cells == "full" else cells):
            g[c] = True
        out.append((g, want))
    return out


# ---- the golden scene of tests/test_gpu_culling.py, test_gpu_train_culling.py and test_gpu_ray_gradients.py  ---------------------
HALF_GRID = np.random.default_rng(16).random((16, 16, 16)) < 0.5      # a 16^3 grid, about half full


def camera_rays(oracle, golden_ckpt, n, spread=False):
    """n rays of the golden training camera (a 23 x 23 image), the last ten turned round so that they miss the box: the first
    n, or with ``spread`` n spread evenly over the image -- its first rows see only empty space, where the colour branch gets
    no gradient."""
    o, d = R.world_rays(oracle, golden_ckpt["c2w_train"], float(golden_ckpt["fov"]), 23, 23)
    idx = (np.arange(n) * len(o)) // n if spread else slice(n)
    o, d = np.ascontiguousarray(o[idx]), np.ascontiguousarray(d[idx])
    if n > 10:
        d[-10:, :3] *= -1.0
    return o, d


def train_scene(oracle, golden_ckpt, n, sc, sf, seed):
    """n spread camera rays with draws, targets and a d_rgb cotangent (drawn in this order), the shipped weights and bounds."""
    o, d = camera_rays(oracle, golden_ckpt, n, spread=True)
    rng = np.random.default_rng(seed)
    return dict(o=o, d=d, n=n, sc=sc, sf=sf, u_c=rng.random((n, sc), dtype=np.float32), u_f=rng.random((n, sf), dtype=np.float32),
                tgt=rng.random((n, 3), dtype=np.float32), d_rgb=(rng.standard_normal((n, 3)) * 0.1).astype(np.float32),
                near=float(golden_ckpt["near"]), far=float(golden_ckpt["far"]), bc=golden_ckpt["blob_coarse"],
                bf=golden_ckpt["blob_fine"])


def culled_context(p, grid, flag, box=GOLDEN_BOX, precision="fp32", **kw):
    """A context on the scene's weights and bounds under the box and the grid, with training-time sample culling set to flag."""
    import nerf_and_dietnerf_amd as N
    c = N.Context(near=p["near"], far=p["far"], precision=precision, **kw)
    c.load_weights(0, p["bc"])
    c.load_weights(1, p["bf"])
    c.set_scene_box(*box)
    if grid is not None:
        c.set_occupancy_grid(grid)
    c.set_train_sample_culling(flag)
    assert c.train_sample_culling is bool(flag)
    return c
