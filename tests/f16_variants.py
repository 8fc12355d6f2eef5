"""Shared definitions of the single-pass fp16 kernel variants (precision="f16") for tests/test_fp16_emulation_host.py
(CPU) and tests/test_gpu_f16_variants.py (GPU): the geometries each kernel serves, the weights and inputs both files use,
and the emulation of each kernel's arithmetic (oracle.mlp_forward_fp16 with the epilogue of that kernel).

Kernel of a network in the f16 mode (csrc/nerf_api.hip, mlp_launch):
  Lx <= 5, n_angles 2 / 1 -> mlp_f16_2t_kernel (mlp_f16_2t.hip)                 packed_epilogue=True
  Lx <= 5, n_angles 0     -> mlp_f16_xyz_kernel (mlp_f16x3.hip, FAST, XYZ)      packed_epilogue="c_in"
  Lx <= 5, n_angles 2 / 1 with NERF_F16_TILES=1 -> mlp_f16_kernel (mlp_f16x3.hip, FAST)             "c_in"
  Lx 6..10, any n_angles  -> the wide-PE build's mlp_f16_kernel / mlp_f16_xyz_kernel (mlp_f16x3_wide.hip)  "c_in"

Run as a script (``python tests/f16_variants.py OUT.npz``) it is the child process of the NERF_F16_TILES=1 test: that
variable is read once per process, so the one-tile kernel of the view-direction networks needs a fresh interpreter.
It writes model_predict's outputs for TILES1_GEOMETRIES at row counts given by the parent in F16_ROWS."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import nerf_oracle as O  # noqa: E402

from support import kw  # noqa: E402,F401  (re-exported: V.kw, B.kw)

# (Lx, Ld, n_angles); Ld is unused by the xyz-only network
TWO_TILE = [(3, 2, 2), (1, 1, 2), (5, 4, 1), (4, 3, 1), (2, 2, 1)]
ONE_TILE_XYZ = [(5, 4, 0), (1, 4, 0), (3, 2, 0)]
WIDE = [(10, 4, 2), (6, 4, 2), (7, 3, 1), (9, 1, 1), (10, 4, 0), (8, 2, 0)]
TILES1_GEOMETRIES = [(5, 4, 2), (3, 2, 2), (4, 3, 1)]     # the one-tile kernel of the view-direction networks

EPILOGUES = (True, "c_in", False)
GPU_BAR = 2e-3             # kernel vs its own emulation, relative to max(1, |emu|) (tests/test_gpu_parity.py's bar)
HOST_ROWS = 4173           # rows the cross-epilogue comparisons run on (a prefix of every GPU row set)


def epilogue_of(lx, na, tiles1=False):
    """packed_epilogue of the kernel that serves this network in the f16 mode."""
    return True if lx <= 5 and na != 0 and not tiles1 else "c_in"


def kernel_name(lx, na, tiles1=False):
    if lx > 5:
        return "wide one-tile" + (" xyz" if na == 0 else "")
    if na == 0:
        return "one-tile xyz"
    return "one-tile (TILES=1)" if tiles1 else "two-tile"


def blobs(lx, ld, na, seed=11):
    """Coarse and fine weights: Glorot kernels, small random biases (so that a misplaced or misrounded bias shows), and
    the sigma bias lifted to 1.5 (Glorot networks are almost transparent; tests/test_gpu_encodings.py does the same)."""
    out = []
    for s in (seed, seed + 1):
        blob = O.glorot_blob(s, **kw(lx, ld, na))
        layers = O.unpack_blob(blob, **kw(lx, ld, na))
        rng = np.random.default_rng(1000 + s)
        parts = []
        for i, (k, b) in enumerate(layers):
            b = rng.uniform(-0.1, 0.1, b.shape).astype(np.float32)
            if i == len(layers) - 1:
                b[:] = 1.5
            parts += [k.ravel(), b]
        out.append(np.concatenate(parts).astype(np.float32))
    return out[0], out[1]


def inputs(m, na, seed=5):
    """m points in [-1.5, 1.5]^3 and m view directions (n_angles + 1 components in [-1, 1], None for n_angles 0).
    Drawn from separate streams, so the inputs of m rows are the first m rows of any larger set."""
    xyz = np.random.default_rng(seed).uniform(-1.5, 1.5, (m, 3)).astype(np.float32)
    dirs = None if na == 0 else np.random.default_rng(seed + 1).uniform(-1, 1, (m, na + 1)).astype(np.float32)
    return xyz, dirs


def emulate(layers, xyz, dirs, lx, ld, epilogue, rnd=O.round_fp16, ladder=None):
    """Raw (M, 4) outputs of the network under packed_epilogue=epilogue; epilogue None = the fp32 oracle.
    ladder: encodings by the single-pass kernels' angle-doubling ladder (oracle.positional_encoding_ladder) instead of the
    oracle's sin / cos; default: for the fp16 epilogues.  At Lx = 10 the ladder flips the fp16 rounding of ~8% of the top
    octave's values, a difference the wide-PE kernels' own-emulation check would otherwise have to absorb."""
    if ladder is None:
        ladder = epilogue is not None
    if ladder:
        xe = O.positional_encoding_ladder(xyz, lx, True)
        de = None if dirs is None else O.positional_encoding_ladder(dirs, ld, False)
    else:
        xe = O.positional_encoding_for_xyz(xyz, lx)
        de = None if dirs is None else O.positional_encoding_for_views(dirs, ld)
    if epilogue is None:
        return O.mlp_forward(layers, xe, de)
    return O.mlp_forward_fp16(layers, xe, de, packed_epilogue=epilogue, rnd=rnd)


def rel_err(a, b):
    """max |a - b| relative to max(1, |b|)."""
    return float(np.abs(a - b).max()) / max(1.0, float(np.abs(b).max()))


def _child(path):
    import nerf_and_dietnerf_amd as N
    rows = [int(r) for r in os.environ["F16_ROWS"].split(",")]
    xyz_all, _ = inputs(max(rows), 2)
    res = {}
    for lx, ld, na in TILES1_GEOMETRIES:
        ctx = N.Context(near=0.6, far=2.4, precision="f16", **kw(lx, ld, na))
        for which, blob in enumerate(blobs(lx, ld, na)):
            ctx.load_weights(which, blob)
        _, dirs_all = inputs(max(rows), na)
        for which in (0, 1):
            for m in rows:
                res[f"{lx}_{ld}_{na}_{which}_{m}"] = ctx.model_predict(which, xyz_all[:m], dirs_all[:m])
        res[f"{lx}_{ld}_{na}_nonfinite"] = np.array(ctx.read_nonfinite())
        ctx.close()
    np.savez(path, **res)


if __name__ == "__main__":
    _child(sys.argv[1])
