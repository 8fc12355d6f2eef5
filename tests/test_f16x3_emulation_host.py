"""The 3-pass fp16 render mode (precision="f16x3") against a CPU emulation of its own arithmetic -- the host side, no
device needed.  tests/f16x3_variants.py holds the emulation, the seeded defects and the shared inputs;
tests/test_gpu_f16x3_emulation.py holds the kernels to it.

What is established here, from the references alone:
  * the roundings of the emulation are the kernels' (fp16 RNE with subnormals, the device re-pack's conversion), and with the
    roundings off the emulation is the fp32 network, through the k-step map of the kernels' fragment layout as well;
  * the bar of a kernel against its emulation, RAW_BAR_FACTOR (4) x the emulation's error against the fp32 oracle, per
    geometry and network; that error is at most 5e-6, ten times inside the 5e-5 the suite held f16x3 to so far;
  * at that bar a lost pass shows: every whole-layer dropped lo pass is >= 3 bars from the emulation, every single 32-wide
    tile > 1 bar, flushed fp16 subnormals >= 3 bars (Glorot families; the shipped checkpoint's late layers are less
    sensitive and are printed only, as tests/test_fp16_emulation_host.py notes for the single-pass mode);
  * the assertions of the GPU test, evaluated with a defect emulation standing in for the kernel, fail;
  * the LOWER limit of the mode: the lo half of an activation is an fp16 subnormal below 2^-4 and hi itself below 2^-14,
    so a network whose activations are small degrades without any non-finite value to watch for -- the table of
    test_low_magnitude_table, quoted in DESIGN.md section 4.1."""
import numpy as np
import pytest

import bf16_variants as B
import f16x3_variants as X

FAMILIES = ("biased", "glorot")


def _say(capsys, text):
    with capsys.disabled():
        print("\n" + text, end="")


# ---- 1. roundings ----
def test_fp16_roundings_agree_on_subnormal_and_halfway_cases():
    """fp16_rne (the emulation) and numpy's conversion (IEEE RNE, what v_cvt_f16_f32 of the device re-pack computes) give
    the same bits on every fp16 value, every midpoint between two neighbours, the fp32 neighbours of both, and random
    values over 2^-30 .. 2^17."""
    halfs = np.arange(0x0000, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float64)     # every finite half >= 0
    mid = (halfs[:-1] + halfs[1:]) / 2                                                        # exact in fp32
    base = np.concatenate([halfs, mid, [65520.0, 65536.0, 2.0 ** -25, 2.0 ** -26, 1e9]]).astype(np.float32)
    near = np.concatenate([base, np.nextafter(base, np.float32(np.inf)), np.nextafter(base, np.float32(-np.inf))])
    rng = np.random.default_rng(0)
    rand = (rng.standard_normal(200000) * 2.0 ** rng.integers(-30, 18, 200000)).astype(np.float32)
    x = np.concatenate([near, -near, rand, [np.inf, -np.inf]]).astype(np.float32)
    with np.errstate(over="ignore"):
        want = x.astype(np.float16)
    np.testing.assert_array_equal(X.fp16_rne(x).view(np.uint32), want.astype(np.float32).view(np.uint32))
    assert np.isnan(X.fp16_rne(np.array([np.nan], np.float32))).all()
    # the lo half of a weight: w - hi is exact in fp32, and the re-pack's conversion of it is the emulation's
    w = (rng.standard_normal(100000) * 2.0 ** rng.integers(-22, 3, 100000)).astype(np.float32)
    hi, lo = X.split_w(w)
    np.testing.assert_array_equal(w.astype(np.float16).astype(np.float32), hi)
    np.testing.assert_array_equal((w - hi).astype(np.float16).astype(np.float32), lo)
    assert np.count_nonzero((np.abs(lo) < 2.0 ** -14) & (lo != 0)) > 1000          # subnormal lo halves were among them
    big = np.abs(w) >= 2.0 ** -3
    assert np.all(np.abs((hi + lo) - w)[big] <= np.abs(w[big]) * 2.0 ** -21)


def test_activation_split():
    x = np.array([1.0, 1.0 + 2.0 ** -10, 1.0 + 2.0 ** -11 + 2.0 ** -12, -3.1415927, 65503.0, 65519.0, 65535.0, 65536.0,
                  7e4, 2.0 ** -5 * 1.2345, 2.0 ** -14 * 1.2345, 2.0 ** -20 * 1.2345, 2.0 ** -26], np.float32)
    hi, lo = X.split_act(x)
    assert hi[2] == 1.0 and lo[2] == np.float32(2.0 ** -11 + 2.0 ** -12)           # truncated, not rounded
    assert X.split_act(x, trunc=False)[0][2] == np.float32(1.0 + 2.0 ** -10)       # ... which RNE would take up
    assert np.isfinite(hi[:7]).all() and hi[6] == 65504.0 and np.isinf(hi[7:9]).all()      # 11 bits below 65536 are <= 65504
    ok = slice(0, 7)
    assert np.all(np.abs((hi + lo) - x)[ok] <= np.abs(x[ok]) * 2.0 ** -21)
    assert np.all(np.abs(hi[:7]) <= np.abs(x[:7]))
    # below 2^-4 lo is on the subnormal grid (multiples of 2^-24); below 2^-14 hi is too; 2^-26 is gone altogether
    assert lo[9] != 0 and lo[9] % np.float32(2.0 ** -24) == 0 and abs(hi[9] + lo[9] - x[9]) > 0
    assert hi[11] % np.float32(2.0 ** -24) == 0 and lo[11] == 0 and hi[12] == 0 and lo[12] == 0
    fh, fl = X.split_act(x, flush=True)
    assert fl[9] == 0 and fh[9] == hi[9] and fh[10] == hi[10] and fh[11] == 0


# ---- 2. rounding off: the fp32 network ----
@pytest.mark.parametrize("na", [2, 1, 0])
@pytest.mark.parametrize("lx,ld", [(1, 1), (5, 4), (10, 2)])
def test_without_roundings_the_emulation_is_the_fp32_network(oracle, lx, ld, na):
    """plain (the oracle's own a @ w + b in the emulation's wiring): the same bits as oracle.mlp_forward.  rounding=False
    (hi = the fp32 value, lo = 0, through the three-pass contraction): within 1e-6, in numpy's order and along the chain of
    the kernel's k-steps -- which also shows that ksteps() holds every input row of every layer exactly once."""
    kw = X.kw(lx, ld, na)
    xyz, dirs = X.inputs(257, na)
    xe, de = X.encode(xyz, dirs, lx, ld)
    for blob in X.networks("biased", lx, ld, na):
        layers = oracle.unpack_blob(blob, **kw)
        ref = oracle.mlp_forward(layers, xe, de)
        np.testing.assert_array_equal(X.forward(layers, xe, de, spec=X.Spec(plain=True))[0], ref)
        for accum in ("f32", "chain", "f64"):
            got = X.forward(layers, xe, de, spec=X.Spec(rounding=False, accum=accum, n_angles=na, n_pos_enc_dir=ld))[0]
            assert X.rel_err(got, ref) <= 1e-6, (accum, X.rel_err(got, ref))
        for l in X.contraction_layers(len(layers)):
            rows = np.sort(np.concatenate(X.ksteps(l, len(layers), lx, ld, na)))
            np.testing.assert_array_equal(rows, np.arange(layers[l][0].shape[0]), err_msg=f"layer {l}")
            assert all(len(s) <= 16 for s in X.ksteps(l, len(layers), lx, ld, na))
    with X.emulated(plain=True):
        np.testing.assert_array_equal(oracle.model_predict(layers, xyz, dirs, lx, ld), ref)
    np.testing.assert_array_equal(oracle.model_predict(layers, xyz, dirs, lx, ld), ref)      # and the patch is gone


def test_shrink_blob_layout(oracle):
    """shrink_blob scales exactly layer 1's kernel and bias and layer 2's kernel, for both network forms."""
    for lx, ld, na in [(5, 4, 2), (3, 2, 2), (7, 2, 0)]:
        kw = X.kw(lx, ld, na)
        blob = X.networks("biased", lx, ld, na)[0]
        a, b = oracle.unpack_blob(blob, **kw), oracle.unpack_blob(X.shrink_blob(blob, -8, lx), **kw)
        for l, ((k0, b0), (k1, b1)) in enumerate(zip(a, b)):
            sk, sb = {0: (2.0 ** -8, 2.0 ** -8), 1: (2.0 ** 8, 1.0)}.get(l, (1.0, 1.0))
            np.testing.assert_array_equal(k1, k0 * np.float32(sk), err_msg=f"kernel {l}")
            np.testing.assert_array_equal(b1, b0 * np.float32(sb), err_msg=f"bias {l}")


# ---- 3. figures, bars, discrimination ----
def _defect_ratios(fg, lx, ld, na, defects):
    """Distance of each defect from the emulation in bars, on the first DEFECT_ROWS rows (a lower bound of the distance on
    all rows: f16x3_variants.distance)."""
    m = X.DEFECT_ROWS
    return [(X.describe(d), X.distance(X.variant(fg, lx, ld, na, m, defects=[d]), fg, m) / fg.bar) for d in defects]


def _figures(capsys, family, lx, ld, na, assert_discrimination):
    xyz, dirs = X.inputs(X.RAW_ROWS, na)
    for which, fg in enumerate(X.raw_figures(family, lx, ld, na)):
        tag = f"[f16x3 {family} ({lx},{ld},{na}) net {which}]"
        n = len(fg.layers)
        noise64 = X.rel_err(X.variant(fg, lx, ld, na, accum="f64"), fg.emu)
        chain = X.rel_err(X.variant(fg, lx, ld, na, accum="chain"), fg.emu)
        _say(capsys, f"{tag} emulation vs oracle {fg.fig:.3e} -> bar {fg.bar:.3e}; summation order: fp32 vs float64 "
                     f"{noise64:.3e}, fp32 vs k-step chain {chain:.3e}")
        assert np.isfinite(fg.emu).all()
        assert fg.fig <= X.EMU_BAR, (tag, fg.fig)
        whole = [(name, apart / fg.bar) for name, _, apart in X.identification_set(family, lx, ld, na, 0, X.DEFECT_ROWS)[which]]
        flush, rne = whole[-2][1], whole[-1][1]
        whole = whole[:-2]
        tiles = _defect_ratios(fg, lx, ld, na, X.tile_defects(n))
        steps = _defect_ratios(fg, lx, ld, na, X.kstep_defects(n, lx))
        lo_w, lo_t, lo_s = (min(r, key=lambda t: t[1]) for r in (whole, tiles, steps))
        _say(capsys, f"{tag} distance from the emulation in bars: whole-layer dropped pass min {lo_w[1]:.1f} ({lo_w[0]}), "
                     f"single tile min {lo_t[1]:.1f} ({lo_t[0]}), single k-step min {lo_s[1]:.2f} ({lo_s[0]}), subnormals "
                     f"flushed {flush:.1f}, hi by RNE {rne:.2f}")
        if assert_discrimination:
            assert lo_w[1] >= 3.0, (tag, lo_w)
            assert lo_t[1] > 1.0, (tag, lo_t)
            assert flush >= 3.0, (tag, flush)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("lx,ld,na", X.GEOMETRIES)
def test_figures_and_discrimination(capsys, family, lx, ld, na):
    """Per geometry and Glorot family, both networks, 4173 rows: the emulation is within 5e-6 of the oracle (measured 2.1e-7 ..
    6.8e-7); every whole-layer dropped lo pass is >= 3 bars from the emulation, every single-tile one > 1 bar, flushed
    subnormals >= 3 bars.  The defect runs (some 200 per network) use the first 521 rows: their distance there is a lower
    bound of their distance on all 4173 (f16x3_variants.distance), so each assertion implies the one on the full set.  Single k-steps (one per block of inputs, the direction steps of layer 8 and of sigma among
    them) and the RNE-hi variant are printed: a single k-step of 16 inputs out of 256 can sit inside the bar."""
    _figures(capsys, family, lx, ld, na, True)


def test_figures_of_the_shipped_checkpoint(capsys):
    """The same quantities for the shipped epoch-95 networks; only the emulation's own error is asserted."""
    _figures(capsys, "checkpoint", 5, 4, 2, False)


def test_a_dropped_pass_fails_the_gpu_assertions(capsys):
    """check_kernel is what tests/test_gpu_f16x3_emulation.py asserts of a kernel's output.  Stand-ins for the kernel: the
    emulation in another summation order (the k-step chain) passes; the emulation without w_hi.x_lo in layer 2, without
    w_lo.x_hi in layer 6, without one pass of the sigma tile, or with flushed subnormals fails."""
    lx, ld, na = 5, 4, 2
    for family in FAMILIES:
        for which, fg in enumerate(X.raw_figures(family, lx, ld, na)):
            wrong = X.identification_set(family, lx, ld, na)[which]
            label = f"{family} net {which}, stand-in"
            X.check_kernel(X.variant(fg, lx, ld, na, accum="chain"), fg, wrong, label + " k-step chain", lambda s: _say(capsys, s))
            for bad in ([X.drop_layer(2, "hl")], [X.drop_layer(6, "lh")], [X.drop_layer(10, "hl")]):
                with pytest.raises(AssertionError):
                    X.check_kernel(X.variant(fg, lx, ld, na, defects=bad), fg, wrong, label, lambda s: None)
                with pytest.raises(AssertionError):      # the bar alone catches it, without the identification
                    X.check_kernel(X.variant(fg, lx, ld, na, defects=bad), fg, (), label, lambda s: None)
            with pytest.raises(AssertionError):
                X.check_kernel(X.variant(fg, lx, ld, na, flush=True), fg, wrong, label, lambda s: None)


# ---- 4. the lower limit ----
def test_low_magnitude_table(oracle, golden_ckpt, capsys):
    """shrink_blob(., k): layer-1 activations 2^k times as large, the same function.  The oracle's output does not change
    by a bit; the bf16x3 emulation's error does not move (fp32's exponent range); the f16x3 emulation's error does not
    improve as k falls and at k = -12 is outside 5e-5 on the shipped networks -- with every value finite, so nothing
    trips the non-finite watch.  Measured (rel_err against the oracle, 4173 rows):
         k    Glorot-biased   checkpoint coarse   checkpoint fine      bf16x3: 3.8e-6 / 8.9e-6 / 1.3e-5 at every k
         0      2.3e-7            2.1e-7              1.7e-6
        -4      3.7e-7            3.7e-6              1.1e-5
        -8      2.6e-6            2.8e-5              2.3e-4
       -12      5.3e-5            1.2e-3              2.5e-3
       -16      8.6e-4            1.3e-2              4.5e-2
    And the RGB floor: with both shipped networks shrunk, the emulated render (64 rays of the test view, 64 + 128 samples)
    leaves 1e-4 of the oracle's RGB at k = -9 (6.3e-5 at -8, 1.9e-4 at -9)."""
    xyz, dirs = X.inputs(X.RAW_ROWS, 2)
    nets = [("Glorot-biased", "biased", 0), ("checkpoint coarse", "checkpoint", 0), ("checkpoint fine", "checkpoint", 1)]
    table = {}
    for name, family, which in nets:
        ref0 = X.raw_figures(family, 5, 4, 2)[which].ref
        for k in X.SHRINK_KS:
            fg = X.raw_figures(family, 5, 4, 2, k)[which]
            np.testing.assert_array_equal(fg.ref, ref0, err_msg=f"{name}, k = {k}: the oracle's output moved")
            assert np.isfinite(fg.emu).all(), (name, k)
            with B.emulated():
                bf = X.rel_err(oracle.model_predict(fg.layers, xyz, dirs, 5, 4), fg.ref)
            table[name, k] = (fg.fig, bf)
    _say(capsys, "[low magnitude] f16x3 / bf16x3 emulation vs oracle:   k   " + "   ".join(f"{n[0]:>21s}" for n in nets))
    for k in X.SHRINK_KS:
        _say(capsys, f"[low magnitude] {k:51d}   " + "   ".join(f"{table[n[0], k][0]:9.2e} / {table[n[0], k][1]:9.2e}" for n in nets))
    for name, family, _ in nets:
        figs = [table[name, k][0] for k in X.SHRINK_KS]
        assert all(b >= a for a, b in zip(figs[:-1], figs[1:])), (name, figs)
        assert all(table[name, k][1] == table[name, 0][1] for k in X.SHRINK_KS), (name, [table[name, k][1] for k in X.SHRINK_KS])
        assert table[name, 0][0] <= X.EMU_BAR
        if family == "checkpoint":
            assert table[name, -12][0] > X.LEGACY_BAR, (name, table[name, -12])
    k_floor, errs = X.rgb_floor()
    _say(capsys, "[low magnitude] emulated render of the shipped checkpoint vs oracle, max-abs RGB: "
                 + ", ".join(f"k={k}: {e:.2e}" for k, e in errs.items()) + f" -> leaves {X.RGB_BAR:g} at k = {k_floor}")
    assert all(np.isfinite(a).all() for k in errs for a in X.rgb_at(k))
    assert errs[0] <= 1e-5
    assert k_floor == X.RGB_FLOOR_K, k_floor
    # the shrunk oracle itself renders the same bits (what lets rgb_at compare with the unshrunk oracle)
    ck, o, d, uc, uf, near, far, ref = X._floor_scene()
    c, f = (oracle.unpack_blob(X.shrink_blob(golden_ckpt[n], k_floor)) for n in ("blob_coarse", "blob_fine"))
    np.testing.assert_array_equal(oracle.render(c, f, o, d, near, far, uc, uf)[0], ref)
