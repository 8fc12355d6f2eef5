"""tests/grad_blocks.py has teeth (CPU, the autograd oracle alone): gradients tampered with in ways the blob-wide
max|g - ref| / max|ref| and the cosine accept are rejected block by block, with the block named; the float32 oracle passes
the block-wise bars against the float64 oracle; blocks() partitions the blob for every network family."""
import numpy as np
import pytest
import torch

import grad_blocks as GB
import support as S
from oracle import nerf_oracle as O
from oracle import train_oracle as T

FP32_BLOB_BAR, MIXED_BLOB_BAR = 2e-4, 2e-2          # the blob-wide bars of tests/test_gpu_train.py at alpha = 1


@pytest.fixture(scope="module")
def default_problem(golden_ckpt):
    """test_gradients_coarse_and_fine's problem: 48 rays x (16 + 24) samples, the shipped checkpoint."""
    p = S.golden_problem(O, golden_ckpt)
    return (p["bc"], p["bf"], p["o"], p["d"], p["tgt"], p["near"], p["far"], p["u_c"], p["u_f"])


@pytest.fixture(scope="module")
def grads(default_problem):
    """float64 and float32 oracle gradients at alpha = 1 and 0.05 (sampler term on), computed once."""
    out = {}
    for alpha in (1.0, 0.05):
        for dt in (torch.float64, torch.float32):
            out[(alpha, dt)] = T.train_gradients(*default_problem, alpha=alpha, dtype=dt)
    return out


def _block(blks, name):
    return dict(blks)[name]


def _rejected(g, ref, blks, bar):
    with pytest.raises(AssertionError) as exc:
        GB.assert_blocks(g, ref, blks, bar, label="tampered")
    return str(exc.value)


def test_tampered_gradients_pass_the_blob_metric_and_fail_block_by_block(grads):
    blks = GB.blocks(5, 4, 2)
    ref = grads[(1.0, torch.float64)]["grad_fine"]
    # 1: the fine sigma head's bias and view-direction rows are zero
    g = ref.copy()
    g[_block(blks, "b10")] = 0.0
    g[_block(blks, "k10[dir]")] = 0.0
    assert S.relerr(g, ref) <= FP32_BLOB_BAR and S.cos(g, ref) > 0.9999999          # today's fp32 bar accepts it
    assert S.relerr(g, ref) <= MIXED_BLOB_BAR                                      # ... and so does the mixed one
    msg = _rejected(g, ref, blks, GB.FP32_BAR)
    assert "worst block b10:" in msg or "worst block k10[dir]:" in msg
    assert "b10:" in msg and "k10[dir]:" in msg and "of the blob max" in msg
    # 2: b8 has the wrong sign
    g = ref.copy()
    g[_block(blks, "b8")] *= -1.0
    assert S.relerr(g, ref) <= MIXED_BLOB_BAR and S.cos(g, ref) > 0.9999            # the mixed bar accepts it
    msg = _rejected(g, ref, blks, GB.MIXED_LEAST)
    assert "worst block b8:" in msg and "k8" not in msg
    # 1 + 2 together, as a mixed_float16 result might carry them
    g[_block(blks, "b10")] = 0.0
    g[_block(blks, "k10[dir]")] = 0.0
    assert S.relerr(g, ref) <= MIXED_BLOB_BAR and S.cos(g, ref) > 0.9999
    msg = _rejected(g, ref, blks, GB.MIXED_LEAST)
    assert all(n in msg for n in ("b8:", "b10:", "k10[dir]:"))
    # 3: layer 4's [xyz | hidden] row groups written in the other order
    g = ref.copy()
    xyz, hid = _block(blks, "k4[xyz]"), _block(blks, "k4[hidden]")
    g[_block(blks, "k4")] = np.concatenate([ref[hid], ref[xyz]])
    msg = _rejected(g, ref, blks, GB.FP32_BAR)
    assert "worst block k4" in msg and "k4[xyz]:" in msg and "k4[hidden]:" in msg
    assert "k3:" not in msg and "k5:" not in msg and "b4:" not in msg
    # the untouched gradient passes
    assert len(GB.assert_blocks(ref.copy(), ref, blks, GB.FP32_BAR)) == len(blks)


def test_float32_oracle_passes_block_by_block(grads, capsys):
    """The reference resolves every block: float32 autograd against float64 autograd at the bars the GPU tests use."""
    blks = GB.blocks(5, 4, 2)
    for net in ("grad_coarse", "grad_fine"):
        r64, r32 = grads[(1.0, torch.float64)][net], grads[(1.0, torch.float32)][net]
        errs = GB.assert_blocks(r32, r64, blks, GB.FP32_BAR, label=f"float32 oracle, alpha 1, {net}")
        assert not any(e.floor for e in errs)                          # no block of the default problem is under the floor
        assert max(e.max_rel for e in errs) <= GB.FP32_SUPPORT * GB.FP32_BAR      # ... and the reference supports the bar
        assert min(e.share for e in errs) > 50 * GB.FLOOR
        # alpha = 0.05 (LeakyReLU masks): relative L2 of every block, the sampler-free part (the fine network)
        r64, r32 = grads[(0.05, torch.float64)][net], grads[(0.05, torch.float32)][net]
        errs = GB.block_errors(r32, r64, blks)
        assert not any(e.floor for e in errs)
        assert max(e.rel_l2 for e in errs) <= 1e-3                     # measured 3.5e-4 (coarse, through the sampler) / 3.4e-4
        with capsys.disabled():
            print(f"\n[float32 vs float64 oracle, alpha 0.05, {net}] {GB.summary(errs, 'l2')}", end="")


def test_the_floor_and_its_cap(grads):
    blks = GB.blocks(5, 4, 2)
    ref = grads[(1.0, torch.float64)]["grad_fine"].copy()
    big = np.abs(ref).max()
    # a block far under the floor is compared absolutely, at bar x FLOOR x blob max
    ref[_block(blks, "b10")] = 1e-9 * big
    g = ref.copy()
    g[_block(blks, "b10")] += 0.5 * GB.FP32_BAR * GB.FLOOR * big
    errs = GB.assert_blocks(g, ref, blks, GB.FP32_BAR)
    assert [e.name for e in errs if e.floor] == ["b10"]
    g[_block(blks, "b10")] += GB.FP32_BAR * GB.FLOOR * big
    assert "b10:" in _rejected(g, ref, blks, GB.FP32_BAR) and "absolute" in _rejected(g, ref, blks, GB.FP32_BAR)
    # more than two such blocks: the inputs are at fault, and the helper says so
    for n in ("b8", "b9"):
        ref[_block(blks, n)] *= 1e-12
    with pytest.raises(ValueError, match="change the inputs"):
        GB.assert_blocks(ref.copy(), ref, blks, GB.FP32_BAR)
    # an identically zero reference block must be exactly zero
    ref = grads[(1.0, torch.float64)]["grad_fine"].copy()
    ref[_block(blks, "b9")] = 0.0
    g = ref.copy()
    GB.assert_blocks(g, ref, blks, GB.FP32_BAR)
    g[_block(blks, "b9")[1]] = 1e-30
    assert "b9" in _rejected(g, ref, blks, GB.FP32_BAR)
    # a zero reference on purpose
    z = np.zeros_like(ref)
    assert GB.assert_blocks(z, z, blks, 0.0, exact_zero=True) == []
    g = z.copy()
    g[_block(blks, "k2")[5]] = 1e-38
    with pytest.raises(AssertionError, match="k2"):
        GB.assert_blocks(g, z, blks, 0.0, exact_zero=True)


@pytest.mark.parametrize("lx,ld,na", [(5, 4, 2), (2, 3, 1), (3, 4, 0), (10, 4, 2), (10, 4, 0), (1, 1, 2), (7, 2, 1)])
def test_blocks_partition_the_blob(lx, ld, na):
    kw = dict(n_pos_enc_xyz=lx, n_pos_enc_dir=ld, n_angles=na)
    blks = GB.blocks(lx, ld, na)
    top = GB.top_level(blks)
    shapes = O.layer_shapes(**kw)
    assert [n for n, _ in top] == [f"{t}{i}" for i in range(len(shapes)) for t in "kb"]
    np.testing.assert_array_equal(np.concatenate([ix for _, ix in top]), np.arange(O.blob_size(**kw)))
    # the row groups partition their kernel, in the order the kernel stores them
    d = dict(blks)
    groups = {"k4": ("k4[xyz]", "k4[hidden]")}
    if na:
        groups.update({"k8": ("k8[hidden]", "k8[dir]"), "k10": ("k10[hidden]", "k10[dir]")})
    assert sorted(n for n in d if "[" in n) == sorted(n for g in groups.values() for n in g)
    for k, (a, b) in groups.items():
        np.testing.assert_array_equal(np.concatenate([d[a], d[b]]), d[k])
    dim_xyz, dim_dir = 3 + 6 * lx, 2 * ld * (na + 1)
    assert d["k4[xyz]"].size == dim_xyz * 256 and d["k4[hidden]"].size == 256 * 256
    if na:
        assert d["k8[dir]"].size == dim_dir * 128 and d["k10[dir]"].size == dim_dir and d["k10[hidden]"].size == 256
    # the indices address what unpack_blob returns
    blob = np.arange(O.blob_size(**kw), dtype=np.float32)
    for i, (k, b) in enumerate(O.unpack_blob(blob, **kw)):
        np.testing.assert_array_equal(blob[d[f"k{i}"]], k.ravel())
        np.testing.assert_array_equal(blob[d[f"b{i}"]], b)
    np.testing.assert_array_equal(blob[d["k4[xyz]"]], O.unpack_blob(blob, **kw)[4][0][:dim_xyz].ravel())
