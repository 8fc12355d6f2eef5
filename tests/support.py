"""What the test modules share, defined once (``import support as S``).  Not a conftest and no fixtures; at import it needs
numpy and the standard library only -- torch, the package and the oracle are imported inside the functions that use them.
A new test file starts from this list:

  numbers         relerr, cos, f32 (an oracle call in float32), n_cus, kw (the geometry keywords of Context / glorot_blob)
  bits            bits, assert_same_bits (a pair of arrays), assert_same_bits_each (two sequences of arrays)
  golden problem  oracle_rays, golden_problem, golden_context: the shipped checkpoint on rays of the 8 x 8 sphere camera
  synthetic nets  NET, blob_context, glorot_context, rays_towards_origin, render_rays (raw nerf_render_rays, chosen outputs)
  ranks           build_stub_rccl, free_port, exchange_comm_id, assert_stand_in_loaded, run_ranks

Scene constants and builders live in the *_ref module they describe (GOLDEN_BOX, the NDC box and the occupancy scenes:
occupancy_ref; the half-full grid and the camera rays of the culling tests: culling_ref; the volume's box, media and rays:
volume_ref; the video bars: video_ref)."""
import os
import socket
import subprocess
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET = {"hidden_layer_dim": 256, "last_hidden_layer_dim": 128, "leaky_relu_alpha": 0.05, "n_pos_enc_dim_xyz": 5,
       "n_pos_enc_view_dir": 4, "n_angles_for_model": 2}
RENDER_OUTPUTS = ("rgb", "weights", "cumprod", "alpha", "rgb_samples", "z", "depth")      # the fields of NerfOutputs, in order


# ---- numbers ------------------------------------------------------------------------------------------------------------------
def relerr(a, b):
    """max |a - b| as a share of max |b|."""
    return float(np.abs(a - b).max() / np.abs(b).max())


def cos(a, b):
    """Cosine of two flat arrays, accumulated in float64 whatever they arrive as."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))


def f32(fn, *a, **kw):
    """The same oracle call in float32: the reference's own rounding, the yardstick of the block-wise bars
    (tests/grad_blocks.py)."""
    import torch
    return fn(*a, dtype=torch.float32, **kw)


def n_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def kw(lx, ld, na):
    return dict(n_pos_enc_xyz=lx, n_pos_enc_dir=ld, n_angles=na)


# ---- bit comparisons ----------------------------------------------------------------------------------------------------------
def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def assert_same_bits(a, b, label="", finite=False, dtype=None):
    """Equal shapes and no differing 32-bit word; reports the number of differing words and nanmax |a - b|.  ``finite``: a has
    no NaN or Inf either.  ``dtype``: a arrives as this dtype (before the float32 view is taken)."""
    if dtype is not None:
        assert np.asarray(a).dtype == dtype, (label, np.asarray(a).dtype)
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert a.shape == b.shape, (label, a.shape, b.shape)
    if finite:
        assert np.isfinite(a).all(), label
    diff = int(np.count_nonzero(bits(a) != bits(b)))
    assert diff == 0, (label, diff, float(np.nanmax(np.abs(a - b))))


def assert_same_bits_each(got, want):
    """Two sequences of arrays: the same length, and every pair the same bits."""
    assert len(got) == len(want), (len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        assert_same_bits(a, b, f"item {i}")


# ---- the golden checkpoint on rays of the sphere camera ---------------------------------------------------------------------------
def oracle_rays(oracle, n, seed=0, hw=8):
    """n rays of an hw x hw image of the camera at (-20, 30) on the unit sphere -> (origins, directions, the generator)."""
    rng = np.random.default_rng(seed)
    c2w = oracle.get_sphere_matrix(1.0, -20, 30, 0).astype(np.float32)
    d = oracle.get_rays_directions(hw, hw, 0.46, c2w).reshape(-1, 4)
    idx = rng.choice(d.shape[0], n, replace=n > d.shape[0])
    return np.tile(c2w[:, 3], (n, 1)).astype(np.float32), np.ascontiguousarray(d[idx]), rng


def golden_problem(oracle, golden_ckpt, n=48, sc=16, sf=24, seed=0):
    """Rays, explicit draws and targets (drawn in this order: u_c, u_f, tgt) with the shipped weights and bounds."""
    o, d, rng = oracle_rays(oracle, n, seed)
    return dict(o=o, d=d, u_c=rng.random((n, sc), dtype=np.float32), u_f=rng.random((n, sf), dtype=np.float32),
                tgt=rng.random((n, 3), dtype=np.float32), sc=sc, sf=sf, n=n, near=float(golden_ckpt["near"]),
                far=float(golden_ckpt["far"]), bc=golden_ckpt["blob_coarse"], bf=golden_ckpt["blob_fine"])


def golden_context(p, fine=True, **kw):
    """A context on the problem's bounds and weights; exact fp32 unless the caller names another precision."""
    import nerf_and_dietnerf_amd as N
    kw.setdefault("precision", "fp32")
    ctx = N.Context(near=p["near"], far=p["far"], **kw)
    ctx.load_weights(0, p["bc"])
    if fine:
        ctx.load_weights(1, p["bf"])
    return ctx


# ---- synthetic networks ---------------------------------------------------------------------------------------------------------
def blob_context(blob_pair, lx=5, ld=4, na=2, precision="f16x3", near=0.6, far=2.4):
    """A context of geometry (lx, ld, na) with the pair's blobs loaded; a None in the pair leaves that network unloaded."""
    import nerf_and_dietnerf_amd as N
    ctx = N.Context(near=near, far=far, precision=precision, **kw(lx, ld, na))
    for which, blob in enumerate(blob_pair):
        if blob is not None:
            ctx.load_weights(which, blob)
    return ctx


def glorot_context(precision, n_angles=2):
    """Glorot blobs 1 and 2 on the default bounds, the coarse network's sigma bias lifted to 0.5."""
    import nerf_and_dietnerf_amd as N
    c = N.Context(precision=precision, n_angles=n_angles)
    blob = N.glorot_blob(1, n_angles=n_angles)
    blob[-1] = 0.5
    c.load_weights(0, blob)
    c.load_weights(1, N.glorot_blob(2, n_angles=n_angles))
    return c


def rays_towards_origin(n, s, near, far, seed=3):
    """n rays towards the origin from z ~ 1.5, and n x s sorted depths in [near, far] -> (o, d, z)."""
    rng = np.random.default_rng(seed)
    o = np.zeros((n, 4), np.float32)
    o[:, :3] = rng.uniform(-0.3, 0.3, (n, 3))
    o[:, 2] += 1.5
    d = np.zeros((n, 4), np.float32)
    d[:, :3] = rng.uniform(-0.4, 0.4, (n, 3))
    d[:, 2] = -1.0
    z = np.sort(rng.uniform(near, far, (n, s)), axis=1).astype(np.float32)
    return o, d, z


def render_rays(ctx, which, o, d, z, outputs):
    """Raw nerf_render_rays on host arrays with the named outputs (of RENDER_OUTPUTS) requested and every other pointer NULL.
    Each output is prefilled with NaN -> the arrays, in the order asked for."""
    import ctypes as C

    from nerf_and_dietnerf_amd import _lib
    n, s = z.shape
    shapes = dict(rgb=(n, 3), weights=(n, s), cumprod=(n, s), alpha=(n, s), rgb_samples=(n, s, 3), z=(n, s), depth=(n,))
    arrays = [np.full(shapes[name], np.nan, np.float32) for name in outputs]
    outs = _lib.NerfOutputs(**{name: a.ctypes.data for name, a in zip(outputs, arrays)})
    o, d, z = (np.ascontiguousarray(x, np.float32) for x in (o, d, z))
    _lib.check(ctx.lib.nerf_render_rays(ctx.h, which, o.ctypes.data, d.ctypes.data, z.ctypes.data, n, s, C.byref(outs),
                                        _lib.NERF_MEM_HOST))
    return arrays


# ---- several ranks on one GPU ---------------------------------------------------------------------------------------------------
def build_stub_rccl(directory):
    """Compile the test-only RCCL stand-in tests/stub_rccl.c into ``directory`` -> its path."""
    out = os.path.join(str(directory), "libstub_rccl.so")
    subprocess.run(["gcc", "-O2", "-shared", "-fPIC", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "stub_rccl.c"),
                    "-o", out, "-L/opt/rocm/lib", "-lamdhip64", "-lrt"], check=True)
    return out


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def exchange_comm_id(N, rank, id_path):
    """rank 0 draws the communicator id, the others read it from a file (any channel will do: it is 128 bytes)."""
    if rank == 0:
        uid = N.Context.comm_unique_id()
        with open(id_path + ".tmp", "wb") as f:
            f.write(uid)
        os.replace(id_path + ".tmp", id_path)
        return uid
    t0 = time.time()
    while not os.path.exists(id_path):
        time.sleep(0.02)
        if time.time() - t0 > 120:
            raise TimeoutError("rank 0 never published the communicator id")
    with open(id_path, "rb") as f:
        return f.read()


def assert_stand_in_loaded():
    """The collective really went through tests/stub_rccl.c (NERF_RCCL_LIB), not through a librccl of the process."""
    with open("/proc/self/maps") as f:
        assert "libstub_rccl.so" in f.read()


def run_ranks(target, world, args, stub_lib=None, timeout=300):
    """Spawn target(rank, world, *args, queue) once per rank; each puts (rank, result), or (rank, exception), on the queue.
    NERF_RCCL_LIB names ``stub_lib`` only while the ranks start (they inherit it; this process keeps whatever it had loaded).
    -> the results in rank order; a rank's exception is raised here."""
    import torch.multiprocessing as mp
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    old = os.environ.get("NERF_RCCL_LIB")
    if stub_lib is not None:
        os.environ["NERF_RCCL_LIB"] = stub_lib
    try:
        procs = [mpc.Process(target=target, args=(r, world, *args, q)) for r in range(world)]
        for pr in procs:
            pr.start()
    finally:
        if old is None:
            os.environ.pop("NERF_RCCL_LIB", None)
        else:
            os.environ["NERF_RCCL_LIB"] = old
    res = [q.get(timeout=timeout) for _ in procs]
    for pr in procs:
        pr.join(timeout=60)
    for _, r in res:
        if isinstance(r, BaseException):
            raise r
    return [r for _, r in sorted(res, key=lambda t: t[0])]
