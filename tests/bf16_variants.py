"""Shared definitions of the bf16x3 render mode (precision="bf16x3", NERF_PRECISION_BF16X3) for
tests/test_bf16x3_host.py (CPU) and tests/test_gpu_bf16x3.py (GPU): the geometries, the weights and inputs both files use,
and the emulation of the kernels' arithmetic (csrc/mlp_f16x3.hip built with NERF_BF16: mlp_bf16x3.hip, mlp_bf16x3_wide.hip).

The emulation calls the oracle's functions and substitutes the 256-wide contractions; it rounds where the kernels round:
  weights      hi = bf16(w) round-to-nearest-even, lo = bf16(w - hi)                 (the device re-pack)
  activations  hi = the top 16 bits of the fp32 value (truncation, no conversion), lo = bf16(x - hi)   (split_e / pack_lo)
  product      w_hi x_lo + w_lo x_hi + w_hi x_hi, accumulated in fp32 on top of the fp32 bias (C-in)
  heads        the 128 -> 3 rgb head in fp32 on the unsplit last hidden layer; sigma = a raw accumulator of an MFMA tile
What it does not model is the order of the fp32 additions inside the MFMA (numpy's matmul has its own)."""
import contextlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import nerf_oracle as O  # noqa: E402

from support import kw  # noqa: E402,F401  (re-exported: V.kw, B.kw)

F32 = np.float32

# (Lx, Ld, n_angles) of the parity cases: both view-direction forms, the xyz-only network, fewer octaves, the wide-PE build
GEOMETRIES = [(5, 4, 2), (5, 4, 1), (5, 4, 0), (3, 2, 2), (10, 4, 2), (7, 2, 0)]
RGB_BAR = 1e-4              # the project's bar for its fp32-class modes: final RGB against the fp32 oracle
RANGE_SCALE = 3e4           # range_blob: layer-1 activations of the shipped network pass 65504
RANGE_BOUNDS = (2.0, 6.0)   # ... on the test view out to depth 6 (the library's default frustum); see test_bf16x3_host.py
RAW_ROWS = 4173             # model_predict rows of the raw-output checks (ragged last tile)
RAW_BAR_FACTOR = 4.0        # kernel vs its own emulation: 4 x the emulation's error against the oracle (raw_figures)


def bf16_rne(a) -> np.ndarray:
    """Round fp32 to bf16 (nearest even, v_cvt_pk_bf16_f32) and hold the value as fp32."""
    x = np.ascontiguousarray(a, F32).view(np.uint32)
    r = ((x + np.uint32(0x7FFF) + ((x >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(F32)
    return np.where(np.isfinite(np.asarray(a, F32)), r, np.asarray(a, F32)).astype(F32)


def bf16_trunc(a) -> np.ndarray:
    """The top 16 bits of the fp32 value."""
    return (np.ascontiguousarray(a, F32).view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)


def split_w(w):
    hi = bf16_rne(w)
    return hi, bf16_rne(np.asarray(w, F32) - hi)


def split_act(a, trunc=True):
    a = np.asarray(a, F32)
    hi = bf16_trunc(a) if trunc else bf16_rne(a)
    return hi, bf16_rne(a - hi)


def contraction(a, w, passes=3, trunc=True):
    ah, al = split_act(a, trunc)
    wh, wl = split_w(w)
    out = al @ wh + ah @ wl + ah @ wh
    if passes == 4:
        out = out + al @ wl
    return out.astype(F32)


def make_forward(passes=3, trunc=True):
    """oracle.mlp_forward's signature with the contractions of the bf16 kernels (both networks' wiring: BODY_LAST, and
    BODY_HIDSIG / BODY_LAST0 for the xyz-only network)."""
    def c(a, w):
        return contraction(a, w, passes, trunc)

    def forward(layers, xyz_enc, dir_enc, alpha=0.05):
        act = O.leaky_relu
        h = act(c(xyz_enc, layers[0][0]) + layers[0][1], alpha)
        for k, b in layers[1:4]:
            h = act(c(h, k) + b, alpha)
        h = act(c(np.concatenate([xyz_enc, h], -1), layers[4][0]) + layers[4][1], alpha)
        for k, b in layers[5:8]:
            h = act(c(h, k) + b, alpha)
        if len(layers) == 12:
            h8 = act(c(h, layers[8][0]) + layers[8][1], alpha)
            h9 = act(c(h8, layers[9][0]) + layers[9][1], alpha)
            rgb = h9 @ layers[10][0] + layers[10][1]
            sigma = c(h, layers[11][0]) + layers[11][1]
            return np.concatenate([rgb, sigma], -1).astype(F32)
        hd = np.concatenate([h, dir_enc], -1)
        h8 = act(c(hd, layers[8][0]) + layers[8][1], alpha)
        rgb = h8 @ layers[9][0] + layers[9][1]
        sigma = c(hd, layers[10][0]) + layers[10][1]
        return np.concatenate([rgb, sigma], -1).astype(F32)
    return forward


@contextlib.contextmanager
def emulated(passes=3, trunc=True):
    """Inside: every oracle function that evaluates a network (model_predict, render, render_image) emulates bf16x3."""
    keep = O.mlp_forward
    O.mlp_forward = make_forward(passes, trunc)
    try:
        yield
    finally:
        O.mlp_forward = keep


def blobs(lx, ld, na, seed=11):
    """Coarse and fine weights: Glorot kernels, small random biases, sigma bias 1.5 (tests/f16_variants.py::blobs)."""
    out = []
    for s in (seed, seed + 1):
        layers = O.unpack_blob(O.glorot_blob(s, **kw(lx, ld, na)), **kw(lx, ld, na))
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
    """m points in [-1.5, 1.5]^3 and m view directions (n_angles + 1 components in [-1, 1], None for n_angles 0)."""
    xyz = np.random.default_rng(seed).uniform(-1.5, 1.5, (m, 3)).astype(np.float32)
    dirs = None if na == 0 else np.random.default_rng(seed + 1).uniform(-1, 1, (m, na + 1)).astype(np.float32)
    return xyz, dirs


def raw_figures(lx, ld, na):
    """For the coarse and the fine network of blobs(lx, ld, na) on inputs(RAW_ROWS, na): (layers, oracle raw, emulated raw,
    rel_err(emulated, oracle)).  4 x the error is the bar of the kernel against its own emulation: the factor covers the
    order of the fp32 additions inside the MFMA, which the emulation does not model."""
    xyz, dirs = inputs(RAW_ROWS, na)
    out = []
    for blob in blobs(lx, ld, na):
        layers = O.unpack_blob(blob, **kw(lx, ld, na))
        ref = O.model_predict(layers, xyz, dirs, lx, ld)
        with emulated():
            emu = O.model_predict(layers, xyz, dirs, lx, ld)
        out.append((layers, ref, emu, rel_err(emu, ref)))
    return out


def rays(n, seed):
    rng = np.random.default_rng(seed)
    o = np.concatenate([rng.uniform(-0.3, 0.3, (n, 3)), np.ones((n, 1))], 1).astype(np.float32)
    d = np.concatenate([rng.uniform(-1, 1, (n, 3)), np.zeros((n, 1))], 1).astype(np.float32)
    return o, d, rng


def rel_err(a, b):
    """max |a - b| relative to max(1, |b|)."""
    return float(np.abs(a - b).max()) / max(1.0, float(np.abs(b).max()))


def range_blob(blob, lx=5, scale=RANGE_SCALE):
    """The same function with activations beyond the fp16 range: layer 1's kernel and bias times `scale`, layer 2's kernel
    divided by it (LeakyReLU is positively homogeneous).  View-direction or xyz-only blob with `lx` xyz octaves."""
    out = np.array(blob, np.float32, copy=True)
    n0 = (3 + 6 * lx) * 256
    out[:n0 + 256] *= F32(scale)                       # layer 1: kernel (3 + 6 lx, 256), bias (256)
    out[n0 + 256:n0 + 256 + 256 * 256] /= F32(scale)   # layer 2: kernel (256, 256)
    return out


def widen_blob(blob, lx_to, lx_from=5, seed=0):
    """A view-direction blob of `lx_from` octaves as an `lx_to`-octave network (the range blob 'adapted to that
    geometry'): the octave rows it lacks are zero, so it is the same function."""
    small = O.unpack_blob(blob, **kw(lx_from, 4, 2))
    parts = []
    for l, (k, b) in enumerate(small):
        if l in (0, 4):
            rows = np.zeros((3 + 6 * lx_to + (256 if l == 4 else 0), k.shape[1]), np.float32)
            for c in range(3):
                src, dst = c * (1 + 2 * lx_from), c * (1 + 2 * lx_to)
                rows[dst:dst + 1 + 2 * lx_from] = k[src:src + 1 + 2 * lx_from]
            if l == 4:
                rows[3 + 6 * lx_to:] = k[3 + 6 * lx_from:]
            k = rows
        parts += [k.ravel(), b]
    return np.concatenate(parts).astype(np.float32)
