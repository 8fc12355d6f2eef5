"""The 3-pass fp16 render kernels on the device (precision="f16x3"; csrc/mlp_f16x3.hip, mlp_f16x3_wide.hip) against the
CPU emulation of their own arithmetic (tests/f16x3_variants.py; its CPU side: tests/test_f16x3_emulation_host.py).

The suite held this mode to 5e-5 of the exact-fp32 mode (tests/test_gpu_parity.py::test_f16x3_model_predict,
tests/test_gpu_f16x3_seams.py); a kernel that loses one of its two lo passes in a whole layer stays inside that.  Here the
bar is RAW_BAR_FACTOR (4) x the emulation's own error against the fp32 oracle on the same rows, relative to
max(1, |ref|): 8e-7 .. 3e-6 on the Glorot networks.  It is computed from the references when the test runs, never from a
kernel's output; the factor covers the order of the fp32 additions inside the MFMA and along the chain of k-steps, which
the emulation does not model (the host test prints how far two orders of the emulation are apart: 3e-7 .. 7e-7).

model_predict on 4173 rows (ragged last tile), both networks of a context, over bf16_variants.GEOMETRIES: the ping-pong
kernel (Lx <= 5, n_angles 2 / 1), the copy-back xyz-only kernel, both wide-PE builds.  On the Glorot families the kernel
must also be strictly closer to its emulation than to every emulation with a whole layer's lo pass dropped, to the one
with fp16-subnormal operands flushed to zero, and to the one whose activation hi is rounded instead of truncated (where
that one is more than a bar away from the correct emulation; it is not at ordinary magnitudes, and says so).

Measured when the tests were written (one MI355X; kernel vs emulation, as a fraction of the bar): 0.15 .. 0.88 over the 26
networks -- two to four units in the last place of the fp32 outputs; the largest are (5,4,0) biased coarse 1.02e-6 of
1.16e-6 and (5,4,1) biased fine 6.9e-7 of 8.4e-7.  DESIGN.md section 4.1b lists every case."""
import numpy as np
import pytest

import bf16_variants as B
import f16x3_variants as X
import support as S

pytestmark = pytest.mark.gpu

NEAR, FAR = 0.6, 2.4


def _say(capsys):
    def out(text):
        with capsys.disabled():
            print("\n" + text, end="")
    return out


# ---- 1. kernel vs emulation, identification ----
CASES = [(f, *g) for g in X.GEOMETRIES for f in ("biased", "glorot")] + [("checkpoint", 5, 4, 2)]


@pytest.mark.parametrize("family,lx,ld,na", CASES)
def test_kernel_follows_its_emulation(golden_ckpt, capsys, family, lx, ld, na):
    """check_kernel (tests/f16x3_variants.py) on both networks: within the bar of the emulation, finite, and -- Glorot
    families -- identified against every whole-layer defect, the flushed-subnormal and the RNE-hi emulation;
    read_nonfinite() == 0."""
    ctx = S.blob_context(X.networks(family, lx, ld, na, golden_ckpt), lx, ld, na)
    try:
        xyz, dirs = X.inputs(X.RAW_ROWS, na)
        figures = X.raw_figures(family, lx, ld, na)
        wrong = X.identification_set(family, lx, ld, na) if family != "checkpoint" else ((), ())
        for which, fg in enumerate(figures):
            raw = ctx.model_predict(which, xyz, dirs)
            X.check_kernel(raw, fg, wrong[which], f"{family} ({lx},{ld},{na}) net {which}", _say(capsys))
        assert ctx.read_nonfinite() == 0
    finally:
        ctx.close()


# ---- 2. the sigma-only kernel ----
def test_sigma_only_kernel_follows_the_emulated_sigma(oracle, capsys):
    """1391 rays x 3 samples = 4173 rows (ragged last tile, the ray changes inside a wave) through the sigma-only kernel of
    the biased Glorot network; reference: the emulated raw outputs composited by oracle.ray_marching.

    Why (FAR - NEAR) x bar bounds the weights (the argument of tests/test_gpu_f16x3_seams.py, item (b)):
    w_s = alpha_s T_s with alpha_s = 1 - exp(-relu(sigma_s) delta_s) and T_s = exp(-sum_{k < s} relu(sigma_k) delta_k), so
    w_s = exp(-A_s) - exp(-A_(s+1)) with A_s = sum_{k < s} relu(sigma_k) delta_k; exp(-.) and relu are 1-Lipschitz, hence
    |d w_s| <= max(|d A_s|, |d A_(s+1)|) <= sum_{k <= s} delta_k |d sigma_k| <= (z_(s+1) - z_0) max |d sigma|
    <= (FAR - NEAR) max |d sigma| for every sample but a ray's last (delta = 1e9 there: a step function of sigma's sign).
    And max |d sigma| between a kernel and its emulation is what test_kernel_follows_its_emulation bounds: bar x
    max(1, |ref|), with the bar -- 4 x the emulation's error against the oracle -- taken on these very rows."""
    lx, ld, na = 5, 4, 2
    blobs = X.networks("biased", lx, ld, na)
    layers = oracle.unpack_blob(blobs[0], **X.kw(lx, ld, na))
    n, s = 1391, 3
    o, d, z = S.rays_towards_origin(n, s, NEAR, FAR)
    pts = oracle.sample_along_rays(o, d, z)[..., :3].reshape(-1, 3)
    view = oracle.get_view_directions(s, d, na)
    ref_raw = oracle.model_predict(layers, pts, view, lx, ld)
    with X.emulated():
        emu_raw = oracle.model_predict(layers, pts, view, lx, ld)
    w_emu = oracle.ray_marching(emu_raw.reshape(n, s, 4), z)[1]
    fig = X.rel_err(emu_raw, ref_raw)
    bound = (FAR - NEAR) * X.RAW_BAR_FACTOR * fig * max(1.0, float(np.abs(ref_raw).max()))
    ctx = S.blob_context(blobs, lx, ld, na)
    try:
        w, = S.render_rays(ctx, 0, o, d, z, ("weights",))                 # {weights} alone: mlp_f16x3_sig_kernel
        err = float(np.abs(w[:, :-1] - w_emu[:, :-1]).max())
        _say(capsys)(f"[f16x3 sigma-only, {n} rays x {s}] emulation vs oracle (raw) {fig:.3e} -> weights bound {bound:.3e}; "
                     f"kernel vs emulated weights (all but the last sample) {err:.3e}; largest weight {w[:, :-1].max():.3f}")
        assert np.isfinite(w).all() and w[:, :-1].max() > 1e-2
        assert err <= bound, (err, bound)
        assert ctx.read_nonfinite() == 0
    finally:
        ctx.close()


# ---- 3. low magnitude ----
@pytest.mark.parametrize("k", [-4, -8, -12])
def test_low_magnitude_kernels_follow_their_emulations(oracle, golden_ckpt, capsys, k):
    """The shipped networks through shrink_blob(., k) (layer-1 activations 2^k times as large, the same function): the
    f16x3 kernel follows ITS emulation -- degraded as that is, tests/test_f16x3_emulation_host.py::test_low_magnitude_table
    -- within the bar computed for that blob, counts no non-finite row, and is closer to it than to the emulation with
    flushed fp16 subnormals (at k = -8 the two are more than 1e-2 apart: the MFMA operands and v_cvt_pk_f16_f32 keep
    subnormals, or this fails).  The bf16x3 kernel on the same blobs meets its own bar."""
    xyz, dirs = X.inputs(X.RAW_ROWS, 2)
    figures = X.raw_figures("checkpoint", 5, 4, 2, k)
    ctx = S.blob_context([X.shrink_blob(golden_ckpt[n], k) for n in ("blob_coarse", "blob_fine")])
    try:
        for which, fg in enumerate(figures):
            flushed = X.variant(fg, 5, 4, 2, flush=True)
            wrong = [("subnormals flushed", flushed, X.distance(flushed, fg))]
            raw = ctx.model_predict(which, xyz, dirs)
            e_emu, _ = X.check_kernel(raw, fg, wrong, f"checkpoint x 2^{k} net {which}", _say(capsys))
            _say(capsys)(f"[f16x3 checkpoint x 2^{k} net {which}] flushed-subnormal emulation: {wrong[0][2]:.3e} from the "
                         f"emulation, {X.rel_err(raw, flushed):.3e} from the kernel")
        assert ctx.read_nonfinite() == 0
        ctx.set_precision("bf16x3")
        for which, fg in enumerate(figures):
            with B.emulated():
                emu = oracle.model_predict(fg.layers, xyz, dirs, 5, 4)
            bar = B.RAW_BAR_FACTOR * X.rel_err(emu, fg.ref)
            raw = ctx.model_predict(which, xyz, dirs)
            e_emu, e_ref = X.rel_err(raw, emu), X.rel_err(raw, fg.ref)
            _say(capsys)(f"[bf16x3 checkpoint x 2^{k} net {which}] bar {bar:.3e}; kernel vs emulation {e_emu:.3e}, kernel vs "
                         f"oracle {e_ref:.3e}")
            assert np.isfinite(raw).all() and e_emu <= bar, (which, e_emu, bar)
        assert ctx.read_nonfinite() == 0
    finally:
        ctx.close()


def test_render_at_the_rgb_floor(golden_ckpt, capsys):
    """Both shipped networks through shrink_blob(., RGB_FLOOR_K) -- the first k at which the EMULATED f16x3 render leaves
    1e-4 of the oracle's RGB (tests/test_f16x3_emulation_host.py finds it) -- rendered on the 64 rays of the 8 x 8 test view,
    64 + 128 samples, explicit draws: f16x3 is within 1e-5 of its emulated RGB (so it is outside 1e-4 of the oracle, silently),
    bf16x3 within 1e-4 of the oracle."""
    k = X.RGB_FLOOR_K
    emu, ref = X.rgb_at(k)
    o, d = X.checkpoint_rays(golden_ckpt)
    uc, uf = X.render_draws()
    ctx = S.blob_context([X.shrink_blob(golden_ckpt[n], k) for n in ("blob_coarse", "blob_fine")],
                   near=float(golden_ckpt["near"]), far=float(golden_ckpt["far"]))
    try:
        got = ctx.render(o, d, 64, 128, uc, uf)[0]
        n16 = ctx.read_nonfinite()
        ctx.set_precision("bf16x3")
        got_bf = ctx.render(o, d, 64, 128, uc, uf)[0]
        e_emu, e_ref = float(np.abs(got - emu).max()), float(np.abs(got - ref).max())
        e_bf = float(np.abs(got_bf - ref).max())
        _say(capsys)(f"[render, checkpoint x 2^{k}] emulated f16x3 vs oracle {np.abs(emu - ref).max():.3e}; f16x3 kernel vs its "
                     f"emulation {e_emu:.3e}, vs oracle {e_ref:.3e} (non-finite rows {n16}); bf16x3 kernel vs oracle {e_bf:.3e}")
        assert np.isfinite(got).all() and n16 == 0
        assert e_emu <= 1e-5, e_emu
        assert np.isfinite(got_bf).all() and e_bf <= X.RGB_BAR, e_bf
        assert ctx.read_nonfinite() == 0
    finally:
        ctx.close()
