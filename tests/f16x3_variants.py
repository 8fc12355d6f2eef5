"""Shared definitions of the 3-pass fp16 render mode (precision="f16x3", NERF_PRECISION_F16X3) for
tests/test_f16x3_emulation_host.py (CPU) and tests/test_gpu_f16x3_emulation.py (GPU): the geometries, the weights and
inputs both files use, the emulation of the kernels' arithmetic (csrc/mlp_f16x3.hip without NERF_BF16, and its wide-PE
build mlp_f16x3_wide.hip), seeded defects of that arithmetic, and the downward twin of bf16_variants.range_blob.

The emulation calls the oracle's functions and substitutes the 256-wide contractions; it rounds where the kernels round
(lines of csrc/mlp_f16x3.hip unless another file is named):
  weights      hi = fp16(w) round-to-nearest-even, lo = fp16(w - hi) with w - hi in fp32: the device re-pack, repack_kernel
               in csrc/aux_kernels.hip ((E)w, (E)(w - (float)hi) with E = _Float16: v_cvt_f16_f32, IEEE RNE with subnormal
               halves below 2^-14, zero below 2^-25, inf from 65520).  The host test holds fp16_rne to numpy's conversion,
               which is the same IEEE rounding.
  activations  split_trunc (mlp_f16_frag.h:42-45): hi_f = the fp32 value with its 13 low mantissa bits cleared (11
  and both     significant bits), lo_f = y - hi_f in fp32 (exact).  Both then go through pack_h2 (mlp_f16_frag.h:27-30,
  encodings    v_cvt_pk_f16_f32, RNE): hi is exact while 2^-14 <= |y| < 65536, rounds to an fp16 subnormal (step 2^-24)
               below and is inf from 65536; lo (|lo| < 2^-10 |y|) is an fp16 subnormal once |y| < 2^-4 and is gone
               below |y| ~ 2^-15.  Layer outputs: store_pair, :202-205 (after act(), :151-156: max(v, alpha v) in fp32);
               encodings: split8, :430-434, of the fp32 values of :523-541 (xyz) and :549-561 (view directions).
  product      per k-step of 16 inputs w_hi x_lo, then w_lo x_hi, then w_hi x_hi (:317, :318, :320), accumulated in
               fp32 by v_mfma_f32_32x32x16_f16 on top of the fp32 bias, which is the accumulator's start value
               (load_bias, :158-164, :259, :365-368).  fp16 x fp16 is exact in fp32.
  heads        the 128 -> 3 rgb head in fp32 on the VALU on the UNSPLIT last hidden layer (xc[], :341-343, :396; the
               head :661-686); sigma = a raw accumulator (no activation) of an MFMA tile over [h7 | dir] with its bias as
               C-in (tile 4 of BODY_LAST / the tile of BODY_SIG, :409-413; xyz-only: the leading tile of BODY_HIDSIG
               over h7, :315).
  wiring       the skip layer reads [xyz_enc, h3] (BODY_SKIP, :299-301); layer 8 reads [h7, dir] (:303-304); the
               xyz-only network is 12 layers: ... h7 -> [sigma | 256-wide layer 8] (BODY_HIDSIG) -> 128-wide layer 9 in
               fp32 (BODY_LAST0) -> rgb head (:628-638).
  encodings    the 3-pass kernels (FAST = false) evaluate every octave by sin_shifted (:531, :557; nerf_device.h:12-27:
               Cody-Waite reduction and minimax polynomials, fp32-accurate) of theta = x (pi 2^k), the oracle's
               _pe_theta; the angle-doubling ladder is the single-pass kernels' (FAST, :528, :554).  So the matching
               oracle functions are positional_encoding_for_xyz / positional_encoding_for_views, the ones
               oracle.model_predict calls.
What it does not model is the order of the fp32 additions inside an MFMA and along the chain of k-steps: `accum` offers
three orders of the same split operands -- "f32" (three whole fp32 matrix products on top of the bias, numpy's own order;
the default, as in bf16_variants), "chain" (sequential k-steps of 16 in the kernel's fragment order, the three passes in
kernel order inside each) and "f64" (float64 accumulation, rounded to fp32 once per layer) -- and order_noise() measures
how far they are apart.

A k-step is 16 input SLOTS of the kernel's fragment layout, not 16 consecutive rows of the Keras kernel: ksteps() maps
each to the rows of the oracle's (in, out) kernel it holds (h_pe_row, h_hid_row, h_dir_row of the gather-table builder in
csrc/mlp_f16x3.hip; a network of fewer octaves sits in the (5 or 10, 4)-octave layout with zero rows, csrc/weight_tables.hip
blob_expand_index)."""
import collections
import contextlib
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import nerf_oracle as O  # noqa: E402

import bf16_variants as B  # noqa: E402
import f16_variants as V  # noqa: E402
import support as S  # noqa: E402

F32 = np.float32

GEOMETRIES = list(B.GEOMETRIES)     # (Lx, Ld, n_angles): ping-pong kernel, xyz-only kernel, both wide-PE builds
RAW_ROWS = V.HOST_ROWS              # 4173 model_predict rows (ragged last tile)
RAW_BAR_FACTOR = B.RAW_BAR_FACTOR   # kernel vs its own emulation: 4 x the emulation's error against the oracle
EMU_BAR = 5e-6                      # emulation vs oracle: ten times inside the 5e-5 bar of test_f16x3_model_predict
LEGACY_BAR = 5e-5                   # tests/test_gpu_parity.py::test_f16x3_model_predict, test_gpu_f16x3_seams.py
RGB_BAR = B.RGB_BAR                 # final RGB against the fp32 oracle
SHRINK_KS = (0, -4, -8, -12, -16)   # shrink_blob exponents of the low-magnitude table
PASSES = ("hl", "lh", "hh")         # kernel order: w_hi x_lo, w_lo x_hi, w_hi x_hi
PASS_NAMES = {"hl": "w_hi.x_lo", "lh": "w_lo.x_hi", "hh": "w_hi.x_hi"}

kw = S.kw
inputs = V.inputs
rel_err = V.rel_err
rays = B.rays


# ---- roundings ----
def fp16_rne(a) -> np.ndarray:
    """Round fp32 to fp16 (nearest even; subnormal halves below 2^-14, inf from 65520) and hold the value as fp32.
    In fp32 arithmetic: the fp16 grid around x has the step q = 2^(max(e, -14) - 10), e = x's exponent; x / q, rint (nearest
    even) and the product with q are exact.  (numpy's own conversion takes ten times as long on the subnormal results the
    lo halves are full of; the host test holds this function to it.)"""
    a = np.ascontiguousarray(a, F32)
    eb = a.view(np.uint32) & np.uint32(0x7F800000)                       # biased exponent, clamped to fp16's -14 .. 15
    np.clip(eb, np.uint32(113 << 23), np.uint32(142 << 23), out=eb)
    eb -= np.uint32(10 << 23)                                            # q = 2^(e - 10)
    r = a * (np.uint32(254 << 23) - eb).view(F32)                        # a / q
    np.rint(r, out=r)
    r *= eb.view(F32)
    if not (np.abs(r).max() <= F32(65504.0)):                            # overflow or NaN somewhere
        with np.errstate(invalid="ignore"):
            r = np.where(np.abs(r) > F32(65504.0), np.copysign(F32(np.inf), a), r).astype(F32)
    return r


def trunc11(a) -> np.ndarray:
    """split_trunc's hi_f: the fp32 value with its 13 low mantissa bits cleared."""
    return (np.ascontiguousarray(a, F32).view(np.uint32) & np.uint32(0xFFFFE000)).view(F32)


def flush_subnormal(a) -> np.ndarray:
    """fp16 values (held as fp32) with the fp16 subnormals set to zero."""
    a = np.asarray(a, F32)
    return np.where(np.abs(a) < F32(2.0 ** -14), F32(0), a).astype(F32)


_split_w_cache = {}


def split_w(w, rounding=True, flush=False):
    """(hi, lo) of a kernel; kept per array (the same layers are split hundreds of times by the defect runs)."""
    w = np.asarray(w, F32)
    if not rounding:
        return w, np.zeros_like(w)
    key = (id(w), flush)
    hit = _split_w_cache.get(key)
    if hit is not None and hit[0] is w:
        return hit[1], hit[2]
    hi = fp16_rne(w)
    with np.errstate(invalid="ignore"):
        lo = fp16_rne(w - hi)
    if flush:
        hi, lo = flush_subnormal(hi), flush_subnormal(lo)
    if not w.flags.writeable or w.base is not None:       # a view into a blob: its values are not going to change
        if len(_split_w_cache) > 512:
            _split_w_cache.clear()
        _split_w_cache[key] = (w, hi, lo)
    return hi, lo


def split_act(a, rounding=True, trunc=True, flush=False):
    a = np.asarray(a, F32)
    if not rounding:
        return a, np.zeros_like(a)
    hi_f = trunc11(a) if trunc else fp16_rne(a)
    with np.errstate(invalid="ignore"):
        lo_f = a - hi_f
    # 11 significant bits are exact in fp16 between 2^-14 and 65536: the conversion of hi matters outside only
    mag = hi_f.view(np.uint32) & np.uint32(0x7FFFFFFF)
    other = np.flatnonzero((mag - np.uint32(0x38800000) >= np.uint32(0x47800000 - 0x38800000)).ravel())
    hi = hi_f
    if other.size:
        hi = hi_f.copy()
        hi.ravel()[other] = fp16_rne(hi_f.ravel()[other])
    lo = fp16_rne(lo_f)
    return (flush_subnormal(hi), flush_subnormal(lo)) if flush else (hi, lo)


# ---- the kernels' k-steps in terms of the oracle's kernel rows ----
def _pe_steps(lx):
    """Rows of xyz_enc (3 + 6 lx: per component x, sin0, cos0, ...) held by each k-step of the PE block."""
    big = 5 if lx <= 5 else 10
    nsteps = (3 + 6 * big + 15) // 16
    steps = [[] for _ in range(nsteps)]
    for v in range(8 * nsteps):
        for h in (0, 1):
            if v < 3 * big:
                c, k = divmod(v, big)
                if k < lx:
                    steps[v // 8].append(c * (1 + 2 * lx) + 1 + 2 * k + h)
            elif big == 5:
                if v < 18 and h == 0:
                    steps[v // 8].append((v - 15) * (1 + 2 * lx))
            elif v == 30:
                steps[v // 8].append(2 * (1 + 2 * lx) if h else 0)
            elif v == 31 and h == 0:
                steps[v // 8].append(1 + 2 * lx)
    return [np.array(sorted(s), np.int64) for s in steps]


def _dir_steps(ld, na):
    """Rows of dir_enc (2 ld per component: sin0, cos0, ...) held by the two direction k-steps of layer 8."""
    steps = [[], []]
    for v in range(12):
        c, k = divmod(v, 4)
        if k >= ld or (na == 1 and c == 1):
            continue
        comp = c if na == 2 else (0 if c == 0 else 1)
        for h in (0, 1):
            steps[v // 8].append(comp * 2 * ld + 2 * k + h)
    return [np.array(sorted(s), np.int64) for s in steps]


_HID_STEPS = [np.arange(16 * n, 16 * n + 16) for n in range(16)]


def ksteps(layer, n_layers, lx, ld, na):
    """The k-steps of `layer` in kernel order: a list of row-index arrays into that layer's oracle kernel."""
    if layer == 0:
        return _pe_steps(lx)
    if layer == 4:
        return _pe_steps(lx) + [s + (3 + 6 * lx) for s in _HID_STEPS]
    if n_layers == 11 and layer in (8, 10):
        return _HID_STEPS + [s + 256 for s in _dir_steps(ld, na)]
    return _HID_STEPS


def contraction_layers(n_layers):
    """Layers that run on the matrix cores (the rgb head does not)."""
    return [l for l in range(n_layers) if l != (9 if n_layers == 11 else 10)]


def n_tiles(layer, n_layers):
    """32-wide output tiles of a layer (the sigma row is one tile)."""
    if layer == n_layers - 1:
        return 1
    return 4 if layer == (8 if n_layers == 11 else 9) else 8


# ---- defects ----
# One pass is not issued for the k-steps `ksteps` (indices into ksteps(); None = all) and the output columns `cols` (None =
# all) of `layer`.  A pass that is not issued adds nothing to the accumulator: the emulation zeroes that pass's weight
# operand on [rows of those k-steps] x [cols], which is the same thing.
Defect = collections.namedtuple("Defect", "layer pas ksteps cols")


def drop_layer(layer, pas):
    return Defect(layer, pas, None, None)


def drop_kstep(layer, pas, n):
    return Defect(layer, pas, (n,), None)


def drop_tile(layer, pas, u, n_layers=11):
    return Defect(layer, pas, None, range(0, 1) if layer == n_layers - 1 else range(32 * u, 32 * u + 32))


def whole_layer_defects(n_layers, passes=("hl", "lh")):
    return [drop_layer(l, p) for l in contraction_layers(n_layers) for p in passes]


def tile_defects(n_layers, passes=("hl", "lh")):
    """Every 32-wide output tile of every layer (the sigma tile included) without one of its lo passes."""
    return [drop_tile(l, p, u, n_layers) for l in contraction_layers(n_layers) for u in range(n_tiles(l, n_layers))
            for p in passes]


def kstep_defects(n_layers, lx, passes=("hl", "lh")):
    """One k-step per block of inputs: PE, hidden, the skip layer's PE and hidden steps, layer 8's and sigma's dir steps."""
    npe = len(_pe_steps(lx))
    picks = [(0, 0), (0, npe - 1), (2, 5), (4, 0), (4, npe + 3), (7, 15)]
    if n_layers == 11:
        picks += [(8, 3), (8, 16), (8, 17), (10, 9), (10, 16), (10, 17)]
    else:
        picks += [(8, 3), (9, 12), (11, 9)]
    return [drop_kstep(l, p, n) for l, n in picks for p in passes]


def describe(d):
    what = "layer" if d.ksteps is None and d.cols is None else ""
    if d.ksteps is not None:
        what += f"k-step {list(d.ksteps)}"
    if d.cols is not None:
        what += f"cols {d.cols.start}..{d.cols.stop - 1}"
    return f"L{d.layer} {PASS_NAMES[d.pas]} {what}"


# ---- the emulation ----
class Spec:
    """How to emulate.  plain: the oracle's own expression a @ w + b (wiring check).  rounding=False: the splits keep the
    fp32 value as hi and zero as lo (the contraction path without roundings).  trunc=False: the activation hi is RNE.
    flush: fp16-subnormal operands are zero.  accum: "f32" | "chain" | "f64" (module docstring).  defects: Defect list.
    n_angles / n_pos_enc_dir: the geometry, needed only for the direction k-steps ("chain", k-step defects on layer 8 / sigma)."""

    def __init__(self, plain=False, rounding=True, trunc=True, flush=False, accum="f32", defects=(), n_angles=None,
                 n_pos_enc_dir=None):
        assert accum in ("f32", "chain", "f64")
        self.plain, self.rounding, self.trunc, self.flush, self.accum = plain, rounding, trunc, flush, accum
        self.defects, self.n_angles, self.n_pos_enc_dir = tuple(defects), n_angles, n_pos_enc_dir

    def but(self, **changes):
        out = Spec(self.plain, self.rounding, self.trunc, self.flush, self.accum, self.defects, self.n_angles,
                   self.n_pos_enc_dir)
        for k, v in changes.items():
            assert hasattr(out, k), k
            setattr(out, k, tuple(v) if k == "defects" else v)
        return out


def _contraction(a, w, b, spec, layer, steps_of):
    """One dense layer before its activation: the three passes of the split operands on top of the bias."""
    if spec.plain:
        return a @ w + b
    ah, al = split_act(a, spec.rounding, spec.trunc, spec.flush)
    wh, wl = split_w(w, spec.rounding, spec.flush)
    acts = {"hl": al, "lh": ah, "hh": ah}
    wts = {"hl": wh, "lh": wl, "hh": wh}
    for d in spec.defects:
        if d.layer != layer:
            continue
        rows = np.arange(w.shape[0]) if d.ksteps is None else np.concatenate([steps_of()[n] for n in d.ksteps])
        cols = np.arange(w.shape[1]) if d.cols is None else np.asarray(d.cols)
        wp = wts[d.pas].copy()
        wp[np.ix_(rows, cols)] = 0
        wts[d.pas] = wp
    with np.errstate(invalid="ignore", over="ignore"):
        if spec.accum == "f64":
            acc = np.asarray(b, np.float64) + np.zeros((a.shape[0], w.shape[1]))
            for p in PASSES:
                acc = acc + acts[p].astype(np.float64) @ wts[p].astype(np.float64)
            return acc.astype(F32)
        if spec.accum == "chain":
            acc = np.asarray(b, F32) + np.zeros((a.shape[0], w.shape[1]), F32)
            for rows in steps_of():
                if len(rows):
                    for p in PASSES:
                        acc += acts[p][:, rows] @ wts[p][rows]
            return acc
        acc = np.asarray(b, F32) + acts["hl"] @ wts["hl"]
        acc += acts["lh"] @ wts["lh"]
        acc += acts["hh"] @ wts["hh"]
        return acc


def _geometry(n_layers, xyz_enc, dir_enc, spec):
    lx = (xyz_enc.shape[1] - 3) // 6
    if n_layers == 12 or dir_enc is None:
        return lx, 4, 0
    dim = dir_enc.shape[1]
    fits = [(ld, na) for na in (1, 2) for ld in (1, 2, 3, 4) if 2 * ld * (na + 1) == dim
            and spec.n_angles in (None, na) and spec.n_pos_enc_dir in (None, ld)]
    if len(fits) != 1:
        raise ValueError(f"{dim} direction inputs: pass n_angles / n_pos_enc_dir to tell the direction k-steps apart")
    return lx, fits[0][0], fits[0][1]


def forward(layers, xyz_enc, dir_enc, alpha=0.05, spec=None, resume=None):
    """oracle.mlp_forward under `spec`: (raw (M, 4), [h0 .. h7]).  resume: the [h0 .. h7] of another run on the same
    inputs whose layers before spec's first defect are reused (a defect changes nothing upstream of its layer)."""
    spec = spec or Spec()
    n = len(layers)
    act = O.leaky_relu

    def c(a, l):
        def steps_of():
            return ksteps(l, n, *_geometry(n, xyz_enc, dir_enc, spec))
        return _contraction(a, layers[l][0], layers[l][1], spec, l, steps_of)

    hs = []
    if resume is not None:
        first = min([d.layer for d in spec.defects] + [n])
        hs = list(resume[:min(first, 8)])
    for l in range(len(hs), 8):
        a = xyz_enc if l == 0 else np.concatenate([xyz_enc, hs[3]], -1) if l == 4 else hs[l - 1]
        hs.append(act(c(a, l), alpha))
    h = hs[7]
    if n == 12:
        h8 = act(c(h, 8), alpha)                              # BODY_HIDSIG's hidden tiles: split again for layer 9
        h9 = act(c(h8, 9), alpha)                             # BODY_LAST0: fp32, unsplit, for the VALU head
        rgb = h9 @ layers[10][0] + layers[10][1]
        sigma = c(h, 11)                                      # BODY_HIDSIG's leading tile: reads h7's fragments
    else:
        hd = np.concatenate([h, dir_enc], -1)
        h8 = act(c(hd, 8), alpha)                             # BODY_LAST: fp32, unsplit, for the VALU head
        rgb = h8 @ layers[9][0] + layers[9][1]
        sigma = c(hd, 10)                                     # tile 4 of BODY_LAST / BODY_SIG
    return np.concatenate([rgb, sigma], -1).astype(F32), hs


def make_forward(spec=None):
    def mlp_forward(layers, xyz_enc, dir_enc, alpha=0.05):
        return forward(layers, xyz_enc, dir_enc, alpha, spec)[0]
    return mlp_forward


@contextlib.contextmanager
def emulated(spec=None, **spec_kw):
    """Inside: every oracle function that evaluates a network (model_predict, render_rays, render, render_image) emulates
    f16x3 -- under Spec(**spec_kw), or `spec`."""
    keep = O.mlp_forward
    O.mlp_forward = make_forward(spec or Spec(**spec_kw))
    try:
        yield
    finally:
        O.mlp_forward = keep


def encode(xyz, dirs, lx, ld):
    return (O.positional_encoding_for_xyz(xyz, lx), None if dirs is None else O.positional_encoding_for_views(dirs, ld))


def predict(layers, xyz, dirs, lx, ld, spec=None, resume=None):
    """model_predict under `spec` in one chunk: (raw, [h0 .. h7])."""
    xe, de = encode(xyz, dirs, lx, ld)
    return forward(layers, xe, de, 0.05, spec, resume)


def order_noise(layers, xyz, dirs, lx, ld, na, accum="f64"):
    """rel_err between the emulation with fp32 accumulation (three whole matrix products) and with `accum` ("f64": float64
    accumulation rounded to fp32 per layer; "chain": the kernel's k-step order) -- two runs of the whole network from the
    same encodings and weights, so the figure includes what the difference of one layer does to the operands of the next."""
    a = predict(layers, xyz, dirs, lx, ld, Spec(n_angles=na, n_pos_enc_dir=ld))[0]
    b = predict(layers, xyz, dirs, lx, ld, Spec(accum=accum, n_angles=na, n_pos_enc_dir=ld))[0]
    return rel_err(b, a)


# ---- weights ----
def shrink_blob(blob, k, lx=5):
    """The same function with layer-1 activations 2^k times as large (k <= 0: smaller): layer 1's kernel and bias times
    2^k, layer 2's kernel divided by it (LeakyReLU is positively homogeneous, and a power of two commutes with every fp32
    rounding, so the oracle's output does not change by a bit).  bf16_variants.range_blob downward; view-direction or
    xyz-only blob with `lx` xyz octaves."""
    out = np.array(blob, np.float32, copy=True)
    n0 = (3 + 6 * lx) * 256
    out[:n0 + 256] *= F32(2.0 ** k)
    out[n0 + 256:n0 + 256 + 256 * 256] *= F32(2.0 ** -k)
    return out


def networks(family, lx, ld, na, golden_ckpt=None):
    """(coarse blob, fine blob) of a family: "biased" (f16_variants.blobs: Glorot kernels, random biases, sigma bias 1.5),
    "glorot" (oracle.glorot_blob(0 / 1): zero biases), "checkpoint" (the shipped epoch-95 weights, (5, 4, 2) only)."""
    if family == "biased":
        return V.blobs(lx, ld, na)
    if family == "glorot":
        return O.glorot_blob(0, **kw(lx, ld, na)), O.glorot_blob(1, **kw(lx, ld, na))
    assert family == "checkpoint" and (lx, ld, na) == (5, 4, 2)
    return golden_ckpt["blob_coarse"], golden_ckpt["blob_fine"]


Figures = collections.namedtuple("Figures", "layers ref emu hs fig bar")
_ckpt = None


def _checkpoint():
    global _ckpt
    if _ckpt is None:
        _ckpt = np.load(os.path.join(ROOT, "tests", "golden", "alexander50_epoch095.npz"))
    return _ckpt


@functools.lru_cache(maxsize=6)       # an entry holds both networks' hidden activations, ~70 MB
def raw_figures(family, lx, ld, na, shrink=0):
    """For the coarse and the fine network of networks(family, ...) (through shrink_blob(., shrink) if shrink != 0) on
    inputs(RAW_ROWS, na): Figures(layers, oracle raw, emulated raw, the emulation's [h0 .. h7], fig = rel_err(emulated,
    oracle), bar = RAW_BAR_FACTOR x fig).  The bar of a kernel against its own emulation comes from the reference alone:
    the factor covers the order of the fp32 additions inside the MFMA and along the chain, which the emulation does not
    model.  The last few calls are kept, so the tests of one geometry share one computation; the arrays are read-only."""
    xyz, dirs = inputs(RAW_ROWS, na)
    out = []
    for blob in networks(family, lx, ld, na, _checkpoint() if family == "checkpoint" else None):
        if shrink:
            blob = shrink_blob(blob, shrink, lx)
        layers = O.unpack_blob(blob, **kw(lx, ld, na))
        ref = O.model_predict(layers, xyz, dirs, lx, ld)
        emu, hs = predict(layers, xyz, dirs, lx, ld, Spec(n_angles=na, n_pos_enc_dir=ld))
        fig = rel_err(emu, ref)
        for arr in [ref, emu] + hs:
            arr.setflags(write=False)
        out.append(Figures(layers, ref, emu, hs, fig, RAW_BAR_FACTOR * fig))
    return tuple(out)


def variant(figures, lx, ld, na, rows=None, **spec_kw):
    """The emulation of raw_figures' network under another Spec (a defect list, flush, trunc, accum) on the same inputs, or
    on their first `rows` rows (compare with figures.emu[:rows])."""
    xyz, dirs = inputs(rows or RAW_ROWS, na)
    spec = Spec(n_angles=na, n_pos_enc_dir=ld, **spec_kw)
    resume = [h[:rows] for h in figures.hs] if spec.defects and set(spec_kw) <= {"defects"} else None
    return predict(figures.layers, xyz, dirs, lx, ld, spec, resume)[0]


def checkpoint_rays(golden_ckpt, side=8):
    """The side x side rays of the shipped checkpoint's test view: (origins (n, 4), directions (n, 4))."""
    c2w = np.asarray(golden_ckpt["c2w_test"], np.float32)
    d = np.ascontiguousarray(O.get_rays_directions(side, side, float(golden_ckpt["fov"]), c2w).reshape(-1, 4), np.float32)
    o = np.ascontiguousarray(np.tile(c2w[:, 3], (side * side, 1)), np.float32)
    return o, d


def render_draws(n=64, sc=64, sf=128, seed=17):
    rng = np.random.default_rng(seed)
    return rng.random((n, sc), dtype=np.float32), rng.random((n, sf), dtype=np.float32)


# ---- what the GPU test asserts of a kernel's raw outputs (also evaluated on the CPU with stand-ins for the kernel) ----
DEFECT_ROWS = 521     # rows of the host test's defect runs: an eighth of RAW_ROWS (see distance())


def distance(raw, fg, rows=None):
    """rel_err(raw, fg.emu) when `raw` holds only the first `rows` rows: max |raw - emu[:rows]| over max(1, |emu|) of ALL
    rows.  It is at most the rel_err the same variant has on all RAW_ROWS rows (a maximum over fewer rows, the same
    denominator), so "at least x bars on the subset" implies "at least x bars on the full set"."""
    return float(np.abs(raw - fg.emu[:rows]).max()) / max(1.0, float(np.abs(fg.emu).max()))


@functools.lru_cache(maxsize=6)
def identification_set(family, lx, ld, na, shrink=0, rows=None):
    """Per network of raw_figures(...): [(label, raw outputs of a WRONG emulation, its distance() from the correct one)] --
    every whole-layer dropped lo pass, fp16-subnormal operands flushed, and the activation hi rounded instead of
    truncated; on all rows, or on the first `rows`."""
    out = []
    for fg in raw_figures(family, lx, ld, na, shrink):
        runs = [(describe(d), variant(fg, lx, ld, na, rows, defects=[d])) for d in whole_layer_defects(len(fg.layers))]
        runs.append(("subnormals flushed", variant(fg, lx, ld, na, rows, flush=True)))
        runs.append(("hi by RNE", variant(fg, lx, ld, na, rows, trunc=False)))
        out.append([(label, raw, distance(raw, fg, rows)) for label, raw in runs])
    return tuple(out)


def check_kernel(raw, fg, wrong=(), label="", out=print):
    """The assertions on one network's model_predict output `raw`: within fg.bar of its emulation, finite, and strictly
    closer to it than to each wrong emulation of `wrong` (identification_set rows; the RNE-hi row only where it is more
    than the bar away from the correct emulation, printed as skipped otherwise).  Returns (kernel vs emulation, kernel vs
    oracle)."""
    e_emu, e_ref = rel_err(raw, fg.emu), rel_err(raw, fg.ref)
    out(f"[f16x3 {label}] emulation vs oracle {fg.fig:.3e} -> bar {fg.bar:.3e}; kernel vs emulation {e_emu:.3e}, kernel "
        f"vs oracle {e_ref:.3e}")
    assert np.isfinite(raw).all(), label
    assert e_emu <= fg.bar, (label, e_emu, fg.bar)
    for name, other, apart in wrong:
        if name == "hi by RNE" and apart <= fg.bar:
            out(f"[f16x3 {label}] hi by RNE is {apart:.3e} from the emulation, inside the bar: comparison skipped")
            continue
        e_other = rel_err(raw, other)
        assert e_emu < e_other, (label, name, e_emu, e_other)
    return e_emu, e_ref


# ---- the RGB floor of the shipped checkpoint ----
RGB_FLOOR_K = -9      # rgb_floor()[0], asserted by tests/test_f16x3_emulation_host.py::test_low_magnitude_table


@functools.lru_cache(maxsize=None)
def _floor_scene():
    ck = _checkpoint()
    o, d = checkpoint_rays(ck)
    uc, uf = render_draws()
    near, far = float(ck["near"]), float(ck["far"])
    ref = O.render(O.unpack_blob(ck["blob_coarse"]), O.unpack_blob(ck["blob_fine"]), o, d, near, far, uc, uf)[0]
    return ck, o, d, uc, uf, near, far, ref


@functools.lru_cache(maxsize=None)
def rgb_at(k):
    """Both shipped networks through shrink_blob(., k): oracle.render of the 8 x 8 test view (64 rays, 64 + 128 samples,
    explicit draws) under emulated(), and the plain oracle's RGB of the unshrunk networks (shrinking does not change a bit
    of it).  Returns (emulated RGB, oracle RGB)."""
    ck, o, d, uc, uf, near, far, ref = _floor_scene()
    c, f = (O.unpack_blob(shrink_blob(ck[n], k)) for n in ("blob_coarse", "blob_fine"))
    with emulated():
        return O.render(c, f, o, d, near, far, uc, uf)[0], ref


def rgb_floor(k_min=-16):
    """(the first k = 0, -1, ... whose emulated RGB is more than RGB_BAR from the oracle's (None: none down to k_min),
    {k: max-abs RGB error} of the k tried)."""
    errs = {}
    for k in range(0, k_min - 1, -1):
        emu, ref = rgb_at(k)
        errs[k] = float(np.abs(emu - ref).max())
        if errs[k] > RGB_BAR:
            return k, errs
    return None, errs
