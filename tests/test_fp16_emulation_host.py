"""CPU checks of oracle.mlp_forward_fp16, the emulation every single-pass fp16 kernel is held to
(tests/test_gpu_f16_variants.py; the kernel of each network is listed in tests/f16_variants.py):
  * with its rounding switched off it is the fp32 network (wiring apart from rounding), for every epilogue;
  * its xyz-only "c_in" branch equals oracle/train_oracle.py::_mlp16, an independent torch statement of that arithmetic;
  * at the GPU test's inputs the three epilogues and fp32 are told apart, and single-row weight defects move the
    output by several times the GPU bar (so that bar catches them)."""
import numpy as np
import pytest
import torch

import f16_variants as V

IDENT = lambda a: a          # noqa: E731  (rounding off)
ALL = V.TWO_TILE + V.ONE_TILE_XYZ + V.WIDE + [(5, 4, 2)]


@pytest.mark.parametrize("na", [2, 1, 0])
@pytest.mark.parametrize("lx", [1, 5, 10])
def test_wiring_without_rounding_is_the_fp32_network(oracle, lx, na):
    ld = 2 if na == 1 else 4
    layers = oracle.unpack_blob(V.blobs(lx, ld, na)[0], **V.kw(lx, ld, na))
    xyz, dirs = V.inputs(500, na)
    ref = V.emulate(layers, xyz, dirs, lx, ld, None)
    xe = oracle.positional_encoding_for_xyz(xyz, lx)
    assert np.array_equal(ref, oracle.mlp_forward_xyz_only(layers, xe) if na == 0
                          else oracle.mlp_forward(layers, xe, oracle.positional_encoding_for_views(dirs, ld)))
    for ep in V.EPILOGUES:
        got = V.emulate(layers, xyz, dirs, lx, ld, ep, rnd=IDENT, ladder=False)
        assert got.shape == (500, 4) and got.dtype == np.float32
        err = float(np.abs(got - ref).max() / np.abs(ref).max())
        assert err <= 1e-6, (ep, err)
        # and with rounding on it is an fp16-class answer, not the fp32 one
        assert float(np.abs(V.emulate(layers, xyz, dirs, lx, ld, ep, ladder=False) - ref).max() / np.abs(ref).max()) > 1e-5, ep


@pytest.mark.parametrize("lx", [5, 1, 10])
def test_xyz_only_c_in_equals_train_oracle(oracle, lx):
    """The numpy xyz-only emulation of mlp_f16_xyz_kernel vs train_oracle._mlp16's 24-tensor branch (float64 torch, fp16
    rounding at the same places) -- the same cross-check tests/test_train_oracle.py makes for the view-direction network."""
    from oracle import train_oracle as T
    blob = V.blobs(lx, 4, 0)[0]
    xyz, _ = V.inputs(300, 0)
    xe = oracle.positional_encoding_for_xyz(xyz, lx)
    want = oracle.mlp_forward_fp16(oracle.unpack_blob(blob, **V.kw(lx, 4, 0)), xe, None, 0.05, packed_epilogue="c_in")
    params = T.blob_to_params(blob, **V.kw(lx, 4, 0))
    assert len(params) == 24
    got = T._mlp16(params, torch.tensor(xe, dtype=torch.float64), None, 0.05, 32768.0).detach().numpy()
    assert np.abs(got - want).max() <= 2e-4 * np.abs(want).max()


def _top_xyz_octave(layers, lx, ld, na):
    """Zero the weight rows of the top xyz octave (sin and cos of 2^(lx-1) pi x, all three components) in layer 0."""
    out = [(k.copy(), b.copy()) for k, b in layers]
    for c in range(3):
        out[0][0][c * (1 + 2 * lx) + 1 + 2 * (lx - 1):c * (1 + 2 * lx) + 1 + 2 * lx] = 0
    return out


def _top_dir_octave(layers, lx, ld, na):
    """Zero the weight rows of the top direction octave in layer 8 (rows 256.. are the direction encoding)."""
    out = [(k.copy(), b.copy()) for k, b in layers]
    for c in range(na + 1):
        out[8][0][256 + c * 2 * ld + 2 * (ld - 1):256 + c * 2 * ld + 2 * ld] = 0
    return out


def _no_sigma_bias(layers, lx, ld, na):
    out = [(k.copy(), b.copy()) for k, b in layers]
    out[-1][1][:] = 0
    return out


@pytest.mark.parametrize("lx,ld,na", ALL)
def test_epilogues_are_told_apart_and_single_row_defects_exceed_the_bar(oracle, lx, ld, na, capsys):
    """At the GPU test's inputs (its first HOST_ROWS rows, both networks): (a) each pair of epilogues, and each epilogue
    and fp32, differ by far more than float noise (the GPU test asserts the kernel is closer to its own emulation than to
    any of the others); (b) each single-row defect moves the kernel's emulation by >= 3x the GPU bar."""
    xyz, dirs = V.inputs(V.HOST_ROWS, na)
    own = V.epilogue_of(lx, na)
    for which, blob in enumerate(V.blobs(lx, ld, na)):
        layers = oracle.unpack_blob(blob, **V.kw(lx, ld, na))
        emu = {ep: V.emulate(layers, xyz, dirs, lx, ld, ep) for ep in V.EPILOGUES + (None,)}
        keys = list(emu)
        gaps = {(a, b): V.rel_err(emu[a], emu[b]) for i, a in enumerate(keys) for b in keys[i + 1:]}
        perturb = [_top_xyz_octave, _no_sigma_bias] + ([_top_dir_octave] if na else [])
        sens = {f.__name__.strip("_"): V.rel_err(V.emulate(f(layers, lx, ld, na), xyz, dirs, lx, ld, own), emu[own])
                for f in perturb}
        with capsys.disabled():
            print(f"\n[f16 emulation ({lx},{ld},{na}) net {which}, {V.kernel_name(lx, na)}] gaps "
                  + " ".join(f"{a}/{b} {g:.2e}" for (a, b), g in gaps.items())
                  + " | sensitivity " + " ".join(f"{k} {s:.2e}" for k, s in sens.items()), end="")
        for pair, g in gaps.items():
            assert g >= 5e-5, (pair, g)          # fp32 summation-order noise here is ~3e-7 (the wiring test)
        for name, s in sens.items():
            assert s >= 3 * V.GPU_BAR, (name, s)


def test_shipped_checkpoint_defects_exceed_the_bar(oracle, golden_ckpt):
    """The shipped (5, 4, 2) networks at the GPU test's inputs: dropping the top xyz octave exceeds 3x the bar (measured
    0.38 / 1.08).  The other two defects are no test of the bar on these trained weights: their sigma biases are ~1e-3
    and their top direction octave moves the output by 7e-3 / 3e-3 -- the synthetic weights above cover those rows."""
    xyz, dirs = V.inputs(V.HOST_ROWS, 2)
    for key in ("blob_coarse", "blob_fine"):
        layers = oracle.unpack_blob(golden_ckpt[key])
        emu = V.emulate(layers, xyz, dirs, 5, 4, True)
        s = V.rel_err(V.emulate(_top_xyz_octave(layers, 5, 4, 2), xyz, dirs, 5, 4, True), emu)
        assert s >= 3 * V.GPU_BAR, (key, s)
