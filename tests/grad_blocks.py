"""Block-wise comparison of a network's gradient blob -- TEST INFRASTRUCTURE ONLY.

`max|g - ref| / max|ref|` over a whole blob only constrains the loudest of its 22-24 tensors: the sigma head's kernel is
~1e-4 of the blob's max, its bias and view-direction rows ~1e-5, most biases ~1e-2.  The trainer builds these through
separate code paths (the batched weight-gradient GEMMs, head_wgrad, the sigma head riding in layer 8's GEMM, the row-mapped
reduction of layer 4's [xyz | hidden] kernel, the bias rows of every partial), so each is compared against ITS OWN max here.

    blocks(lx, ld, n_angles)          -> [(name, index_array)] into the Keras-order blob
    block_errors(g, ref, blocks)      -> per block: max error / block max, relative L2, share of the blob max
    assert_blocks(g, ref, blocks, bar) -> raises naming the worst block; returns the per-block figures

Block names: "k<i>" / "b<i>" for layer i's kernel / bias (top level: these partition the blob), and "k<i>[xyz]",
"k<i>[hidden]", "k<i>[dir]" for the row groups of a kernel whose input is a concatenation.
"""
from collections import namedtuple

import numpy as np

from oracle import nerf_oracle as O

FLOOR = 1e-7              # a block whose reference max is below FLOOR x the blob's max is compared absolutely
MAX_FLOOR_BLOCKS = 2      # ... and a comparison may hold at most this many of them

BlockError = namedtuple("BlockError", "name max_rel rel_l2 share abs_err floor")


def blocks(lx=5, ld=4, n_angles=2):
    """Ordered (name, index_array) list: every kernel and bias, each followed by its row groups where the trainer treats them
    separately.  Layout and widths come from oracle.unpack_blob's shapes: the xyz width is layer 0's input, the hidden width
    layer 1's, and a kernel with more input rows than that is a concatenation ([xyz | hidden] where the surplus equals the
    xyz width -- layer 4 --, [hidden | dir] otherwise -- layer 8 and the sigma head of the view-direction networks)."""
    kw = dict(n_pos_enc_xyz=lx, n_pos_enc_dir=ld, n_angles=n_angles)
    layers = O.unpack_blob(np.zeros(O.blob_size(**kw), np.float32), **kw)
    dim_xyz, hidden = layers[0][0].shape[0], layers[1][0].shape[0]
    out, off = [], 0
    for i, (k, b) in enumerate(layers):
        rows, cols = k.shape
        out.append((f"k{i}", np.arange(off, off + rows * cols)))
        if i > 0 and rows > hidden:
            first = ("xyz", dim_xyz) if i == 4 else ("hidden", hidden)
            second = "hidden" if i == 4 else "dir"
            assert i != 4 or rows == dim_xyz + hidden, (i, rows)
            cut = off + first[1] * cols
            out.append((f"k{i}[{first[0]}]", np.arange(off, cut)))
            out.append((f"k{i}[{second}]", np.arange(cut, off + rows * cols)))
        off += rows * cols
        out.append((f"b{i}", np.arange(off, off + cols)))
        off += cols
    assert off == O.blob_size(**kw)
    return out


def top_level(blks):
    """The kernels and biases themselves (they partition the blob), without the row groups."""
    return [(n, ix) for n, ix in blks if "[" not in n]


def block_errors(g, ref, blks):
    """Per block: max|g - ref| / max|ref| over the block, ||g - ref|| / ||ref||, max|ref| over the block / max|ref| over the blob,
    max|g - ref|, and whether the block lies under the absolute-comparison floor (its relative figures are then inf or nan
    where the reference is zero)."""
    g, ref = np.asarray(g, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    assert g.shape == ref.shape, (g.shape, ref.shape)
    blob_max = float(np.abs(ref).max())
    out = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for name, ix in blks:
            d, r = g[ix] - ref[ix], ref[ix]
            rmax, dmax = float(np.abs(r).max()), float(np.abs(d).max())
            out.append(BlockError(name, float(np.float64(dmax) / rmax), float(np.linalg.norm(d) / np.linalg.norm(r)),
                                  float(np.float64(rmax) / blob_max), dmax, bool(rmax < FLOOR * blob_max)))
    return out


def worst(errs, metric="max"):
    """(name, figure) of the block with the largest relative error among those compared relatively."""
    key = (lambda e: e.max_rel) if metric == "max" else (lambda e: e.rel_l2)
    rel = [e for e in errs if not e.floor and np.isfinite(key(e))]
    if not rel:
        return None, 0.0
    w = max(rel, key=key)
    return w.name, key(w)


def _bar_of(bar, name):
    return float(bar[name]) if isinstance(bar, dict) else float(bar)


def assert_blocks(g, ref, blks, bar, metric="max", label="", blob_relative=None, exact_zero=False):
    """Every block of `g` within `bar` of `ref`, relative to the block's OWN max (metric "max") or its own L2 norm ("l2").
    bar: one number, or {block name: number}.
    A block whose reference is identically zero must be exactly zero in `g`.
    A block whose reference max is below FLOOR x the blob's max is compared absolutely, at bar x FLOOR x blob max; more than
    MAX_FLOOR_BLOCKS of them is an error of the test's inputs (the reference does not exercise those tensors).
    blob_relative: {block name: bar of the blob's max} for blocks whose path is documented to reach only that (they are
    still reported).  exact_zero: the reference gradient is zero on purpose; every block of `g` must be exactly zero.
    Raises AssertionError naming the worst block, its error and its share of the blob max; returns the BlockErrors."""
    g, ref = np.asarray(g, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    if exact_zero:
        assert not ref.any(), f"{label}: exact_zero asked for a reference gradient that is not zero"
        bad = [(n, float(np.abs(g[ix]).max())) for n, ix in blks if g[ix].any()]
        assert not bad, f"{label}: blocks that must be exactly zero are not: " + ", ".join(f"{n} (max {v:.3e})" for n, v in bad)
        return []
    # a block whose reference is identically zero (a dead ReLU, a head the loss does not reach) must be exactly zero: stricter
    # than the absolute comparison, so it does not count against the cap
    dead = [(n, ix) for n, ix in blks if not ref[ix].any()]
    bad = [(n, float(np.abs(g[ix]).max())) for n, ix in dead if g[ix].any()]
    assert not bad, f"{label}: blocks whose reference is identically zero are not: " + ", ".join(f"{n} (max {v:.3e})" for n, v in bad)
    dead_names = {n for n, _ in dead}
    errs = block_errors(g, ref, [(n, ix) for n, ix in blks if n not in dead_names])
    blob_max = float(np.abs(ref).max())
    floor = [e for e in errs if e.floor]
    if len(floor) > MAX_FLOOR_BLOCKS:
        raise ValueError(f"{label}: {len(floor)} blocks lie under {FLOOR:g} of the blob max ({', '.join(e.name for e in floor)}): "
                         f"the inputs do not exercise them -- change the inputs, not the cap of {MAX_FLOOR_BLOCKS}")
    blob_relative = blob_relative or {}
    failed = []                                           # (excess factor, message)
    for e in errs:
        b = _bar_of(bar, e.name)
        if e.name in blob_relative:
            fig, lim, how = e.abs_err / blob_max, blob_relative[e.name], "of the blob max"
        elif e.floor:
            fig, lim, how = e.abs_err, b * FLOOR * blob_max, "absolute (block under the floor)"
        elif metric == "l2":
            fig, lim, how = e.rel_l2, b, "relative L2 of the block"
        else:
            fig, lim, how = e.max_rel, b, "of the block's own max"
        if not fig <= lim:                                # (nan fails)
            failed.append((fig / lim if lim > 0 else np.inf,
                           f"{e.name}: error {fig:.3e} {how} > bar {lim:.3e}; the block is {e.share:.2e} of the blob max"))
    if failed:
        failed.sort(key=lambda t: -t[0] if np.isfinite(t[0]) else -np.inf)
        raise AssertionError(f"{label}: worst block {failed[0][1]}" +
                             ("" if len(failed) == 1 else "; also " + "; ".join(m for _, m in failed[1:])))
    return errs


def scaled_bars(yard, ref, blks, factor, metric="max", least=0.0):
    """Per-block bars from a reference-side yardstick: factor x the error of `yard` against `ref` in each block (the same
    metric), never below `least`.  A block under the floor is compared absolutely: it gets the yardstick's figure over the
    whole blob."""
    yard, ref = np.asarray(yard, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    whole = block_errors(yard, ref, [("blob", np.arange(ref.size))])[0]
    out = {}
    for e in block_errors(yard, ref, blks):
        fig = (whole if e.floor else e)[1 if metric == "max" else 2]
        out[e.name] = max(least, factor * fig)
    return out


def summary(errs, metric="max"):
    """One short string for a test's printed line: the worst block and its figure."""
    n, v = worst(errs, metric)
    if n is None:
        return "no block compared relatively"
    share = next(e.share for e in errs if e.name == n)
    return f"worst block {n} {v:.2e} ({'max' if metric == 'max' else 'rel-L2'}; block is {share:.1e} of the blob max)"


# ---- the bars of the gradient tests, each from the reference side (testing) ------------------------------------
FP32_BAR = 2e-4           # float32 policy, smooth (alpha = 1) network: of the block's own max
FP32_SUPPORT = 0.35       # ... where plain float32 autograd itself resolves the block to 0.35 of the bar (7e-5; it reaches
#                           6.9e-5 on the default problem).  A block it does not resolve that far is a sum over the sample rows
#                           that cancels to a small net value: every fp32 summand is rounded at 6e-8 of ITS size, so the error
#                           relative to the block's net max grows with sum|terms| / |sum terms| whatever the summation order --
#                           the float32 oracle shares no code with the kernels and measures exactly that conditioning.  Such a
#                           block keeps the blob-relative assert (its figure is still reported).
MASK_FACTOR = 16.0        # alpha = 0.05: x the float32 oracle's largest per-block relative L2 (a handful of LeakyReLU mask
#                           flips where it has one or two; a flip in one layer moves every layer's gradient, so the yardstick
#                           is the oracle's worst block, and a wrong mask in a block is an O(1) error)
MIXED_FACTOR, MIXED_LEAST = 4.0, 2e-2     # mixed_float16: x (the emulation in float32 vs itself in float64), never below 2e-2


def check_fp32_smooth(g, ref64, ref32, blks, blob_bar, label="", named=(), bar=FP32_BAR):
    """float32 policy at alpha = 1: FP32_BAR of each block's own max for the blocks the float32 oracle `ref32` resolves;
    `blob_bar` of the blob max (the test's own blob bar) for the others, and for the blocks the test names in `named` (with
    the derivation in its docstring).  bar: FP32_BAR unless the test documents why its inputs carry a larger fp32 error into
    every block (then its own blob bar).  -> a line for the test to print."""
    own = block_errors(ref32, ref64, blks)
    blob_rel = {e.name: blob_bar for e in own if not e.floor and np.isfinite(e.max_rel) and e.max_rel > FP32_SUPPORT * bar}
    assert set(named) <= {n for n, _ in blks}, named
    blob_rel.update({n: blob_bar for n in named})
    errs = block_errors(g, ref64, blks)
    kept = [e for e in errs if e.name in blob_rel]
    line = label + ": " + summary([e for e in errs if e.name not in blob_rel and np.isfinite(e.max_rel)]) + f", bar {bar:g}"
    if kept:
        line += "; at the blob-relative bar (float32 autograd itself > 0.35 of the bar there, or named by the test): " + \
                ", ".join(f"{e.name} {e.max_rel:.1e}" for e in kept)
    print("\n    " + line, end="")
    assert_blocks(g, ref64, blks, bar, "max", label, blob_relative=blob_rel)
    return line


def check_fp32_masks(g, ref64, ref32, blks, label="", named=(), blob_bar=5e-2):
    """float32 policy at alpha = 0.05: relative L2 of each block against MASK_FACTOR x the float32 oracle's largest.
    named: the blocks of the layers at and below ONE LeakyReLU mask flip that the test documents (float32 autograd has none
    on its problem, so its figure is no yardstick for them): they keep `blob_bar` of the blob max, the bar the blob-wide
    assert holds them to, and are reported."""
    own = [e.rel_l2 for e in block_errors(ref32, ref64, blks) if not e.floor and np.isfinite(e.rel_l2)]
    # never below FP32_BAR: the masks only add to the error of the smooth network's arithmetic, which the alpha = 1 bar allows
    # (where float32 autograd has no flip at all its figure, ~1e-6, is below the fp32-class products' own 1e-5..1e-4)
    bar = max(FP32_BAR, MASK_FACTOR * max(own))
    assert set(named) <= {n for n, _ in blks}, named
    errs = [e for e in block_errors(g, ref64, blks) if np.isfinite(e.rel_l2)]
    line = f"{label}: {summary([e for e in errs if e.name not in named], 'l2')}, bar {bar:.1e} (16 x the float32 oracle's {max(own):.1e}, at least 2e-4)"
    if named:
        line += "; at the blob-relative bar (one documented mask flip): " + \
                ", ".join(f"{e.name} {e.rel_l2:.1e}" for e in errs if e.name in named)
    print("\n    " + line, end="")
    assert_blocks(g, ref64, blks, bar, "l2", label, blob_relative={n: blob_bar for n in named})
    return line


def layers_up_to(blks, last):
    """Names of every block (row groups included) of layers 0..last: what one mask flip in layer `last` can move."""
    return tuple(n for n, _ in blks if int(n[1:].split("[")[0]) <= last)


def check_mixed(g, emu64, emu32, blks, label=""):
    """mixed_float16 at alpha = 1 against the fp16-emulating oracle `emu64`: per block, MIXED_FACTOR x the distance of the same
    emulation run in float32 (the same rounding points after a different accumulation), never below MIXED_LEAST."""
    bars = scaled_bars(emu32, emu64, blks, MIXED_FACTOR, "max", MIXED_LEAST)
    errs = [e for e in block_errors(g, emu64, blks) if np.isfinite(e.max_rel)]
    w, v = worst(errs)
    line = f"{label}: {summary(errs)}, bar {bars[w]:.1e}" + (" (4 x the emulation's own)" if bars[w] > MIXED_LEAST else "")
    over = [e for e in errs if e.max_rel > MIXED_LEAST]
    if over:
        line += "; above 2e-2: " + ", ".join(f"{e.name} {e.max_rel:.1e} (bar {bars[e.name]:.1e})" for e in over)
    print("\n    " + line, end="")
    assert_blocks(g, emu64, blks, bars, "max", label)
    return line


def check_equal(g, ref, blks, bar, label=""):
    """Two GPU results that must agree (a split batch, two ranks, two call paths): `bar` of each block's own max; bar 0 = bit
    equality, reported by block."""
    if bar == 0:
        bad = [n for n, ix in blks if not np.array_equal(np.asarray(g).ravel()[ix], np.asarray(ref).ravel()[ix])]
        assert not bad, f"{label}: blocks differ: {', '.join(bad)}"
        return
    assert_blocks(g, ref, blks, bar, "max", label)
