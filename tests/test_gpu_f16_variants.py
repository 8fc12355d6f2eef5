"""Every single-pass fp16 kernel (precision="f16") against an emulation of ITS arithmetic (oracle.mlp_forward_fp16 with
the epilogue of that kernel; the dispatch table is in tests/f16_variants.py), at the default network's bar (2e-3 of
max(1, |emu|), tests/test_gpu_parity.py::test_fp16_single_pass_mode) instead of the fp32 oracle's fp16-class bars
(3e-2 RGB / 5e-2 raw).  tests/test_fp16_emulation_host.py shows on the CPU that single-row weight defects (top xyz octave,
top direction octave, sigma bias) move these outputs by >= 3x this bar, and that the three epilogues and fp32 differ.

Row counts straddle the tiles (128 rows per workgroup tile in the one-tile kernels, 256 in the two-tile one) and include
two counts at which every workgroup of the persistent grid (grid = min(tiles, CUs)) loops at least twice."""
import os
import subprocess
import sys

import numpy as np
import pytest

import f16_variants as V
import support as S

pytestmark = pytest.mark.gpu

ROWS = [1, 31, 127, 128, 129, 255, 256, 257, 333, 1000, V.HOST_ROWS]


def _rows():
    import torch
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count     # the library's hipDeviceProp_t.multiProcessorCount
    return ROWS + [2 * n_cus * 128 + 77, 2 * n_cus * 256 + 77]


def _check(predict, layers, lx, ld, na, epilogue, rows, label):
    """predict(m) -> (m, 4) raw outputs for the first m rows of V.inputs.  Asserts the bar at every row count, and that on
    the first HOST_ROWS rows the kernel is clearly closer to its own emulation than to the other two epilogues and fp32.

    The ordering is judged on the MEAN |error|, not the max: the max over 16692 outputs is set by one fp16 rounding flip
    (fp32 summation order) that propagates, and it is about the same whichever emulation it is measured against -- on
    the MI355X err_own was up to 13% above err_False at (6, 4, 2) while its mean was 3x below.  Measured mean ratios
    own / nearest other: 0.08 .. 0.36 over every variant; the assertion asks for <= 0.5."""
    xyz, dirs = V.inputs(max(rows), na)
    emu = V.emulate(layers, xyz, dirs, lx, ld, epilogue)
    worst, got_h = 0.0, None
    for m in rows:
        got = predict(m)
        assert got.shape == (m, 4) and np.isfinite(got).all(), (label, m)
        err = V.rel_err(got, emu[:m])
        assert err <= V.GPU_BAR, (label, m, err)
        worst = max(worst, err)
        if m == V.HOST_ROWS:
            got_h = got
    h = V.HOST_ROWS
    others = {"fp32" if ep is None else str(ep): V.emulate(layers, xyz[:h], None if dirs is None else dirs[:h], lx, ld, ep)
              for ep in V.EPILOGUES + (None,) if ep != epilogue}
    mean = lambda ref: float(np.abs(got_h - ref).mean())          # noqa: E731
    own, own_mean = V.rel_err(got_h, emu[:h]), mean(emu[:h])
    line = (f"[{label}] err_own {own:.2e} (worst over rows {worst:.2e}) | "
            + " ".join(f"err_{k} {V.rel_err(got_h, o):.2e}" for k, o in others.items())
            + f" | mean-abs own {own_mean:.2e} " + " ".join(f"{k} {mean(o):.2e}" for k, o in others.items()))
    for k, o in others.items():
        assert own_mean <= 0.5 * mean(o), (label, k, line)
    return line


@pytest.mark.parametrize("lx,ld,na", V.TWO_TILE + V.ONE_TILE_XYZ + V.WIDE)
def test_model_predict_matches_its_kernels_emulation(oracle, lx, ld, na, capsys):
    rows = _rows()
    blob_pair = V.blobs(lx, ld, na)
    ctx = S.blob_context(blob_pair, lx, ld, na, "f16")
    xyz, dirs = V.inputs(max(rows), na)
    ep = V.epilogue_of(lx, na)
    try:
        for which, blob in enumerate(blob_pair):
            layers = oracle.unpack_blob(blob, **V.kw(lx, ld, na))
            line = _check(lambda m: ctx.model_predict(which, xyz[:m], None if dirs is None else dirs[:m]),
                          layers, lx, ld, na, ep, rows, f"({lx},{ld},{na}) net {which} {V.kernel_name(lx, na)}")
            with capsys.disabled():
                print("\n" + line, end="")
        assert ctx.read_nonfinite() == 0
    finally:
        ctx.close()


def test_shipped_checkpoint_matches_two_tile_emulation(oracle, golden_ckpt, capsys):
    rows = _rows()
    blob_pair = (golden_ckpt["blob_coarse"], golden_ckpt["blob_fine"])
    ctx = S.blob_context(blob_pair, 5, 4, 2, "f16")
    xyz, dirs = V.inputs(max(rows), 2)
    try:
        for which, blob in enumerate(blob_pair):
            line = _check(lambda m: ctx.model_predict(which, xyz[:m], dirs[:m]), oracle.unpack_blob(blob), 5, 4, 2,
                          True, rows, f"shipped checkpoint net {which} two-tile")
            with capsys.disabled():
                print("\n" + line, end="")
        assert ctx.read_nonfinite() == 0
    finally:
        ctx.close()


def test_one_tile_kernel_under_nerf_f16_tiles_1(oracle, tmp_path, capsys):
    """NERF_F16_TILES=1 (read once per process) routes the view-direction networks to mlp_f16_kernel, whose arithmetic is
    the "c_in" epilogue's: a fresh child process (tests/f16_variants.py) writes its outputs, this one compares."""
    rows = _rows()
    out = tmp_path / "tiles1.npz"
    env = dict(os.environ, NERF_F16_TILES="1", F16_ROWS=",".join(str(m) for m in rows))
    helper = os.path.join(os.path.dirname(os.path.abspath(__file__)), "f16_variants.py")
    res = subprocess.run([sys.executable, helper, str(out)], env=env, timeout=600, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    got = np.load(out)
    for lx, ld, na in V.TILES1_GEOMETRIES:
        assert int(got[f"{lx}_{ld}_{na}_nonfinite"]) == 0
        for which, blob in enumerate(V.blobs(lx, ld, na)):
            layers = oracle.unpack_blob(blob, **V.kw(lx, ld, na))
            line = _check(lambda m: got[f"{lx}_{ld}_{na}_{which}_{m}"], layers, lx, ld, na, "c_in", rows,
                          f"({lx},{ld},{na}) net {which} {V.kernel_name(lx, na, tiles1=True)}")
            with capsys.disabled():
                print("\n" + line, end="")


@pytest.mark.parametrize("lx,ld,na", [(3, 2, 2), (3, 2, 0), (7, 3, 1), (10, 4, 0)])
def test_render_matches_emulating_oracle(oracle, lx, ld, na, monkeypatch, capsys):
    """render() of one geometry per kernel (two-tile, one-tile xyz, wide, wide xyz) against oracle.render whose network
    forward is that kernel's emulation, at ragged (rays, coarse, fine) shapes; config 5's RGB bar."""
    near, far = 0.6, 2.4
    blob_pair = V.blobs(lx, ld, na)
    ctx = S.blob_context(blob_pair, lx, ld, na, "f16")
    coarse, fine = (oracle.unpack_blob(b, **V.kw(lx, ld, na)) for b in blob_pair)
    ep = V.epilogue_of(lx, na)
    emu = lambda layers, xe, de, alpha=0.05: oracle.mlp_forward_fp16(layers, xe, de, alpha, packed_epilogue=ep)  # noqa: E731
    errs = []
    try:
        for n, sc, sf in ((1, 2, 1), (17, 33, 0), (96, 7, 100), (2, 64, 256)):
            rng = np.random.default_rng(n + sc + sf)
            o = np.concatenate([rng.uniform(-0.3, 0.3, (n, 3)), np.ones((n, 1))], 1).astype(np.float32)
            d = np.concatenate([rng.uniform(-1, 1, (n, 3)), np.zeros((n, 1))], 1).astype(np.float32)
            uc, uf = rng.random((n, sc), dtype=np.float32), rng.random((n, sf), dtype=np.float32)
            got = ctx.render(o, d, sc, sf, uc, uf if sf else None)
            with monkeypatch.context() as mp:
                mp.setattr(oracle, "mlp_forward", emu)
                ref = oracle.render(coarse, fine if sf else None, o, d, near, far, uc, uf, **V.kw(lx, ld, na))
            assert got[0].shape == (n, 3)
            e = float(np.abs(got[0] - ref[0]).max())
            errs.append(e)
            assert e <= 1e-3, ((n, sc, sf), e)
        assert ctx.read_nonfinite() == 0
    finally:
        ctx.close()
    with capsys.disabled():
        print(f"\n[render ({lx},{ld},{na}) {V.kernel_name(lx, na)}] max-abs RGB vs emulating oracle "
              + " ".join(f"{e:.2e}" for e in errs), end="")


@pytest.mark.parametrize("lx,ld,na", V.WIDE)
def test_wide_build_f16x3_row_sweep(oracle, lx, ld, na, capsys):
    """The wide-PE build's 3-pass f16x3 kernels over the same row counts, against the fp32 oracle at the 5e-5 raw bar of
    tests/test_gpu_encodings.py (which checks model_predict at 400 rows only)."""
    rows = _rows()
    blob_pair = V.blobs(lx, ld, na)
    ctx = S.blob_context(blob_pair, lx, ld, na, "f16x3")
    xyz, dirs = V.inputs(max(rows), na)
    worst = 0.0
    try:
        for which, blob in enumerate(blob_pair):
            ref = V.emulate(oracle.unpack_blob(blob, **V.kw(lx, ld, na)), xyz, dirs, lx, ld, None)
            for m in rows:
                got = ctx.model_predict(which, xyz[:m], None if dirs is None else dirs[:m])
                assert got.shape == (m, 4)
                err = V.rel_err(got, ref[:m])
                assert err <= 5e-5, (which, m, err)
                worst = max(worst, err)
        assert ctx.read_nonfinite() == 0
    finally:
        ctx.close()
    with capsys.disabled():
        print(f"\n[f16x3 wide ({lx},{ld},{na})] worst raw error vs fp32 oracle over rows {worst:.2e}", end="")
