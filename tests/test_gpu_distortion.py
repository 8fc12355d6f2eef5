"""The distortion loss on the device (include/nerf_mi355.h, "distortion loss"): the bare operator nerf_distortion_loss against
the float64 pairwise definition, and the regulariser inside nerf_train_gradients / nerf_train_step against float64 autograd of
the training graph with the two extra terms (tests/distortion_ref.py), with the helpers and the bars tests/test_gpu_train.py
uses for the plain step."""
import ctypes as C
import functools

import numpy as np
import pytest

import distortion_ref as D
import grad_blocks as GB
from occupancy_ref import GOLDEN_BOX
import support as S

pytestmark = pytest.mark.gpu

BLOCKS = GB.blocks(5, 4, 2)
NEAR, FAR = 2.0, 6.0                       # the operator tests' bounds
SIZES = [1, 2, 63, 64, 65, 129, 1024]      # the chunk seams, the single-sample ray, the longest coarse pass
N_RAYS = 5                                 # a partly filled block of four rays


# ---- shared references (computed once) --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _operator_case(s):
    """Inputs at S = s, the float64 definition on them, and the bar of each output: 4 x the error of the float32 numpy
    restatement against float64 on the same inputs (the factor allows for another summation order in the scans)."""
    w, z = D.operator_inputs(N_RAYS, s, NEAR, FAR, seed=s)
    assert not D.has_ties(z, NEAR, FAR) and not w[1].any() and (s < 63 or (w[[0, 2, 3, 4]] == 0).any())
    ref = D.pairwise_grads(w, z, NEAR, FAR)
    r32 = D.restated(w, z, NEAR, FAR, np.float32)
    own = [float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(r32, ref)]
    for a in ref + r32 + (w, z):
        a.setflags(write=False)
    return w, z, ref, own


_REFS = {}


def _ref(p, key, dtype="float64", **kw):
    """distortion_ref.train_gradients on problem `p`, kept under `key` for the tests that share it."""
    import torch
    full = (key, dtype) + tuple(sorted((k, str(v)) for k, v in kw.items()))
    if full not in _REFS:
        _REFS[full] = D.train_gradients(p["bc"], p["bf"], p["o"], p["d"], p["tgt"], p["near"], p["far"], p["u_c"], p["u_f"],
                                        dtype=getattr(torch, dtype), **kw)
    return _REFS[full]


def _grads(ctx, p):
    return ctx.train_gradients(p["o"], p["d"], p["tgt"], p["sc"], p["sf"], p["u_c"], p["u_f"])


def _raw_call(ctx, w, z, want=(True, True, True)):
    """nerf_distortion_loss on host arrays with any of the three output pointers NULL."""
    from nerf_and_dietnerf_amd import _lib
    n, s = w.shape
    outs = [np.full(shape, np.nan, np.float32) if on else None for on, shape in zip(want, ((n,), (n, s), (n, s)))]
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)                       # noqa: E731
    rc = ctx.lib.nerf_distortion_loss(ctx.h, ptr(w), ptr(z), n, s, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), _lib.NERF_MEM_HOST)
    return rc, outs


@pytest.fixture(scope="module")
def op_ctx():
    import nerf_and_dietnerf_amd as N
    ctx = N.Context(near=NEAR, far=FAR)
    yield ctx
    ctx.close()


# ---- 1. the operator against the float64 definition ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("s", SIZES)
def test_operator_against_the_float64_definition(op_ctx, s, mem, capsys):
    """N = 5 rays x S samples, weights alpha * cumprod with exact zeros and one all-zero ray, sorted depths without ties.  Per
    output the bar is 4 x the error the float32 numpy restatement has against float64 on the same inputs; for orientation, that
    error is about 6e-7 on dL/dw (values up to 2) and 5e-8 on L_ray and dL/dz."""
    import torch
    w, z, ref, own = _operator_case(s)
    if mem == "device":
        got = op_ctx.distortion_loss(torch.tensor(w).cuda(), torch.tensor(z).cuda())
        assert all(g.is_cuda for g in got)
        got = [g.cpu().numpy() for g in got]
    else:
        got = [np.array(g) for g in op_ctx.distortion_loss(w, z)]
    errs = [float(np.abs(g.astype(np.float64) - r).max()) for g, r in zip(got, ref)]
    with capsys.disabled():
        print(f"\n    [distortion operator, {N_RAYS} x {s}, {mem}] error vs float64 (bar = 4 x the float32 restatement's): " +
              ", ".join(f"{n} {e:.2e} (bar {4 * o:.2e})" for n, e, o in zip(("L_ray", "dL/dw", "dL/dz"), errs, own)), end="")
    assert [g.shape for g in got] == [(N_RAYS,), (N_RAYS, s), (N_RAYS, s)]
    assert all(np.isfinite(g).all() for g in got)
    assert not got[0][1] and not got[1][1].any() and not got[2][1].any()          # the all-zero ray
    for name, e, o in zip(("L_ray", "dL/dw", "dL/dz"), errs, own):
        assert e <= 4 * o, (name, s, mem, e, 4 * o)
    if mem == "host":        # each output pointer NULL in turn: the others do not change
        for k in range(3):
            want = tuple(i != k for i in range(3))
            rc, outs = _raw_call(op_ctx, w, z, want)
            assert rc == 0 and outs[k] is None
            S.assert_same_bits_each([o for o in outs if o is not None], [g for i, g in enumerate(got) if i != k])
        rc, _ = _raw_call(op_ctx, w, z, (False, False, False))
        assert rc == 0


# ---- 2. determinism ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [129, 1024])
def test_operator_gives_the_same_bits_on_every_run(op_ctx, s):
    import torch
    w, z, _, _ = _operator_case(s)
    wd, zd = torch.tensor(w).cuda(), torch.tensor(z).cuda()
    first = [g.cpu().numpy() for g in op_ctx.distortion_loss(wd, zd)]
    again = [g.cpu().numpy() for g in op_ctx.distortion_loss(wd, zd)]
    host = [np.array(g) for g in op_ctx.distortion_loss(w, z)]
    S.assert_same_bits_each(again, first)
    S.assert_same_bits_each(host, first)
    # ... and for another batching of the rays: a ray's results do not depend on its neighbours in the block
    alone = [g.cpu().numpy() for g in op_ctx.distortion_loss(wd[3:4].contiguous(), zd[3:4].contiguous())]
    S.assert_same_bits_each(alone, [f[3:4] for f in first])


# ---- 3. the regulariser alone, through the network -----------------------------------------------------------------------------------
@pytest.mark.parametrize("lam,sampler_gradient", [((1.0, 1.0), False), ((1.0, 1.0), True), ((0.0, 1.0), True)])
def test_regulariser_alone_through_the_network(oracle, golden_ckpt, lam, sampler_gradient, capsys):
    """MSE weights (0, 0) and distortion weights (1, 1): every gradient that arrives came through the new path -- dL/dw into
    the compositing backward of both passes and, under sampler_gradient, dL/dz of the fine depths into the sampler and on into
    the coarse network.  The shipped checkpoint at alpha = 1, 48 x (16 + 24), against float64 autograd at the bars of
    tests/test_gpu_train.py::test_gradients_coarse_and_fine (2e-4 of each block's own max; 2e-4 of the blob max where float32
    autograd itself does not resolve a block).  The colour branch gets no gradient from this loss: its blocks are exactly zero.
    With the sampler term the coarse blob must hold the dL/dz part, and the reference WITHOUT it must fail the same bar.  At
    weights (1, 1) it cannot: on this problem the whole sampler term is 2e-6 of the coarse blob (float64 autograd: the blob's
    max is 3.1e-5 from the coarse pass's own dL/dw against 7.4e-11 through the sampler), so leaving dL/dz out moves the blob by
    5e-6 of its max, far below any fp32 bar.  The third case, weights (0, 1), takes the coarse pass's own term away: the
    coarse blob is then the sampler term alone, the reference without dL/dz is off by 2.2 x the blob's max, and it is that
    case which shows the term is there."""
    p = S.golden_problem(oracle, golden_ckpt)
    kw = dict(loss_w=(0.0, 0.0), lam=lam, sampler_grad=sampler_gradient, alpha=1.0)
    r, r32 = _ref(p, "default", **kw), _ref(p, "default", "float32", **kw)
    ctx = S.golden_context(p, leaky_relu_alpha=1.0)
    ctx.train_begin(5e-4, sampler_gradient=sampler_gradient)
    ctx.train_set_loss_weights(0.0, 0.0)
    ctx.train_set_distortion_weights(*lam)
    m, gc, gf = _grads(ctx, p)
    sums, steps = ctx.train_read_distortion_sums()
    ctx.close()
    assert np.isfinite(gc).all() and np.isfinite(gf).all() and gc.any() and gf.any()
    assert m["loss"] == 0.0 and steps == 1 and (lam[0] > 0 or sums["distortion_coarse"] == 0.0)
    tag = f"[distortion alone, weights {lam}, 48 x (16+24), alpha 1, sampler term {'on' if sampler_gradient else 'off'}]"
    with capsys.disabled():
        print(f"\n    {tag} L coarse {sums['distortion_coarse']:.6f} (ref {r['dist_coarse']:.6f}), fine "
              f"{sums['distortion_fine']:.6f} (ref {r['dist_fine']:.6f}); blob error coarse {S.relerr(gc, r['grad_coarse']):.2e}, "
              f"fine {S.relerr(gf, r['grad_fine']):.2e} of max|g|", end="")
        GB.check_fp32_smooth(gc, r["grad_coarse"], r32["grad_coarse"], BLOCKS, 2e-4, tag + " coarse")
        GB.check_fp32_smooth(gf, r["grad_fine"], r32["grad_fine"], BLOCKS, 2e-4, tag + " fine")
    assert S.relerr(gc, r["grad_coarse"]) <= 2e-4 and S.relerr(gf, r["grad_fine"]) <= 2e-4
    if sampler_gradient:
        no_dz = _ref(p, "default", **kw, dz_term=False)
        np.testing.assert_array_equal(no_dz["grad_fine"], r["grad_fine"])      # (the fine network does not see that term)
        with capsys.disabled():
            print(f"; the reference without dL/dz differs by {S.relerr(no_dz['grad_coarse'], r['grad_coarse']):.2e} of the "
                  f"coarse blob's max", end="")
            if lam[0] == 0.0:
                with pytest.raises(AssertionError):
                    GB.check_fp32_smooth(gc, no_dz["grad_coarse"], r32["grad_coarse"], BLOCKS, 2e-4, tag + " coarse, NO dL/dz")


# ---- 4. MSE and regulariser together ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,sampler_gradient,blob_bar", [((48, 16, 24), True, 2e-4), ((48, 16, 24), False, 2e-4),
                                                              ((37, 65, 7), True, 5e-4)])
def test_mse_and_regulariser_together(oracle, golden_ckpt, shape, sampler_gradient, blob_bar, capsys):
    """Loss weights (1, 1), distortion weights (0.01, 0.01): the step a training run takes.  The ragged shape (37 rays: a
    partly filled block; 65 coarse samples: one past a chunk seam; 7 fine ones) takes the blob bar of
    tests/test_gpu_train.py::test_gradients_at_ragged_shapes, 5e-4."""
    n, sc, sf = shape
    p = S.golden_problem(oracle, golden_ckpt, n=n, sc=sc, sf=sf, seed=0 if n == 48 else 11)
    kw = dict(loss_w=(1.0, 1.0), lam=(0.01, 0.01), sampler_grad=sampler_gradient, alpha=1.0)
    key = "default" if n == 48 else "ragged"
    r, r32 = _ref(p, key, **kw), _ref(p, key, "float32", **kw)
    ctx = S.golden_context(p, leaky_relu_alpha=1.0)
    ctx.train_begin(5e-4, sampler_gradient=sampler_gradient)
    ctx.train_set_distortion_weights(0.01, 0.01)
    m, gc, gf = _grads(ctx, p)
    ctx.close()
    tag = f"[MSE + 0.01 distortion, {n} x ({sc}+{sf}), alpha 1, sampler term {'on' if sampler_gradient else 'off'}]"
    with capsys.disabled():
        print(f"\n    {tag} blob error coarse {S.relerr(gc, r['grad_coarse']):.2e}, fine {S.relerr(gf, r['grad_fine']):.2e} of "
              f"max|g|", end="")
        GB.check_fp32_smooth(gc, r["grad_coarse"], r32["grad_coarse"], BLOCKS, blob_bar, tag + " coarse")
        GB.check_fp32_smooth(gf, r["grad_fine"], r32["grad_fine"], BLOCKS, blob_bar, tag + " fine")
    assert abs(m["loss"] - r["loss"]) <= 2e-6 * r["loss"]                         # the metric stays the weighted MSE sum
    assert abs(m["psnr_coarse"] - r["psnr_coarse"]) <= 1e-4 and abs(m["psnr_fine"] - r["psnr_fine"]) <= 1e-4
    assert S.relerr(gc, r["grad_coarse"]) <= blob_bar and S.relerr(gf, r["grad_fine"]) <= blob_bar


# ---- 5. mixed_float16 -------------------------------------------------------------------------------------------------------------
def test_mixed_float16_policy(oracle, golden_ckpt, capsys):
    """The gradients the kernel emits carry the loss scale, read from the optimizer state on the device.  MSE weights (0, 0)
    and distortion weights (1, 1), so that every gradient is the new path's (beside the MSE terms, whose gradients are 1e3 x
    larger on this problem, a regulariser without its loss scale would hide under the fp16-class bars) -- against the autograd
    oracle that rounds where the kernels round, block by block (grad_blocks.check_mixed); the unscaled gradients at two
    initial loss scales agree as in tests/test_gpu_train.py::test_mixed_float16_policy_gradients_and_loss_scaling."""
    p = S.golden_problem(oracle, golden_ckpt)
    grads = {}
    for scale in (32768.0, 4096.0):
        kw = dict(loss_w=(0.0, 0.0), lam=(1.0, 1.0), sampler_grad=True, alpha=1.0, fp16_loss_scale=scale)
        r16, e32 = _ref(p, "default", **kw), _ref(p, "default", "float32", **kw)
        ctx = S.golden_context(p, leaky_relu_alpha=1.0)
        ctx.train_begin(5e-4, mixed_float16=True, initial_loss_scale=scale)
        ctx.train_set_loss_weights(0.0, 0.0)
        ctx.train_set_distortion_weights(1.0, 1.0)
        m, gc, gf = _grads(ctx, p)
        sums, _ = ctx.train_read_distortion_sums()
        assert ctx.train_loss_scale()[0] == scale
        ctx.close()
        grads[scale] = (gc, gf)
        assert np.isfinite(gc).all() and np.isfinite(gf).all() and m["loss"] == 0.0
        with capsys.disabled():
            print(f"\n    [mixed_float16, distortion alone, scale {scale:g}] L coarse {sums['distortion_coarse']:.6f} (emulation "
                  f"{r16['dist_coarse']:.6f}), fine {sums['distortion_fine']:.6f} ({r16['dist_fine']:.6f})", end="")
            GB.check_mixed(gc, r16["grad_coarse"], e32["grad_coarse"], BLOCKS, f"[mixed_float16, distortion alone, scale {scale:g}] coarse")
            GB.check_mixed(gf, r16["grad_fine"], e32["grad_fine"], BLOCKS, f"[mixed_float16, distortion alone, scale {scale:g}] fine")
        assert abs(sums["distortion_fine"] - r16["dist_fine"]) <= 1e-3 * r16["dist_fine"]
    np.testing.assert_allclose(grads[32768.0][1], grads[4096.0][1], rtol=0, atol=2e-2 * np.abs(grads[4096.0][1]).max())
    a, b = grads[32768.0][0].astype(np.float64), grads[4096.0][0].astype(np.float64)
    assert float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b))) > 0.999


# ---- 6. off means off -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["float32", "mixed_float16"])
def test_off_means_off(oracle, golden_ckpt, policy):
    p = S.golden_problem(oracle, golden_ckpt)
    d_rgb = (np.random.default_rng(3).standard_normal((48, 3)) * 0.1).astype(np.float32)
    mixed = policy == "mixed_float16"
    never = S.golden_context(p)
    never.train_begin(5e-4, mixed_float16=mixed)
    m0, gc0, gf0 = _grads(never, p)
    render0 = never.train_render_gradients(p["o"], p["d"], d_rgb, p["sc"], p["sf"], p["u_c"], p["u_f"])
    assert never.train_read_distortion_sums() == ({"distortion_coarse": 0.0, "distortion_fine": 0.0}, 0)
    never.close()
    ctx = S.golden_context(p)
    ctx.train_begin(5e-4, mixed_float16=mixed)
    ctx.train_set_distortion_weights(0.5, 0.25)
    m1, gc1, gf1 = _grads(ctx, p)
    # with the regulariser the metrics are those without it, bit for bit; the gradients are not
    assert m1 == m0 and not np.array_equal(gc1, gc0) and not np.array_equal(gf1, gf0)
    # the backward passes through render() ignore it
    render1 = ctx.train_render_gradients(p["o"], p["d"], d_rgb, p["sc"], p["sf"], p["u_c"], p["u_f"])
    S.assert_same_bits_each(render1, render0)
    # switched off again: the step of a context that never heard of it
    ctx.train_set_distortion_weights(0.0, 0.0)
    m2, gc2, gf2 = _grads(ctx, p)
    assert m2 == m0
    S.assert_same_bits_each([gc2, gf2], [gc0, gf0])
    assert ctx.train_read_distortion_sums()[1] == 1
    # a restarted trainer starts without it
    ctx.train_set_distortion_weights(0.5, 0.25)
    ctx.train_begin(5e-4, mixed_float16=mixed)
    m3, gc3, gf3 = _grads(ctx, p)
    assert m3 == m0
    S.assert_same_bits_each([gc3, gf3], [gc0, gf0])
    ctx.close()


# ---- 7. culling -------------------------------------------------------------------------------------------------------------------
def test_full_grid_culling_is_the_flag_off(oracle, golden_ckpt):
    """A culled sample has weight zero and the compositing runs on all samples: the trainer's sample culling needs no special
    case.  Under a full grid, where every sample is kept, the gradients with the regulariser are the flag-off ones bit for bit."""
    p = S.golden_problem(oracle, golden_ckpt)
    res = []
    for flag in (False, True):
        ctx = S.golden_context(p)
        ctx.set_scene_box(*GOLDEN_BOX)
        ctx.set_occupancy_grid(np.ones((16, 16, 16), bool))
        ctx.set_train_sample_culling(flag)
        ctx.train_begin(5e-4)
        ctx.train_set_distortion_weights(0.5, 0.25)
        m, gc, gf = _grads(ctx, p)
        samples, kept = ctx.read_culling()
        assert (samples, kept) == ((48 * 40, 48 * 40) if flag else (0, 0))
        res.append((m, [gc, gf], ctx.train_read_distortion_sums()))
        ctx.close()
    assert res[0][0] == res[1][0] and res[0][2] == res[1][2] and res[0][1][0].any() and res[0][1][1].any()
    S.assert_same_bits_each(res[1][1], res[0][1])


# ---- 8. the running sums ------------------------------------------------------------------------------------------------------------
def test_running_sums(oracle, golden_ckpt, capsys):
    """Three nerf_train_gradients calls on three batches: the sums are the reference's three L values added up, the bar test
    1's bar for L_ray (4 x the float32 restatement's error, the largest over test 1's sizes) times the pass's S; a read clears
    them; a pass whose weight is 0 adds nothing."""
    probs = [S.golden_problem(oracle, golden_ckpt, n=12, seed=s) for s in (0, 1, 2)]
    refs = [_ref(q, f"sums{i}", alpha=1.0) for i, q in enumerate(probs)]
    want = {"distortion_coarse": sum(r["dist_coarse"] for r in refs), "distortion_fine": sum(r["dist_fine"] for r in refs)}
    bar_ray = 4 * max(_operator_case(s)[3][0] for s in SIZES)
    bars = {"distortion_coarse": bar_ray * 16, "distortion_fine": bar_ray * 24}
    ctx = S.golden_context(probs[0], leaky_relu_alpha=1.0)
    ctx.train_begin(5e-4)
    ctx.train_set_distortion_weights(0.01, 0.01)
    for q in probs:
        _grads(ctx, q)
    sums, steps = ctx.train_read_distortion_sums()
    with capsys.disabled():
        print("\n    [distortion sums over three batches] " + ", ".join(
            f"{k} {sums[k]:.8f} (ref {want[k]:.8f}, error {abs(sums[k] - want[k]):.2e}, bar {bars[k]:.2e})" for k in sums), end="")
    assert steps == 3
    assert ctx.train_read_distortion_sums() == ({"distortion_coarse": 0.0, "distortion_fine": 0.0}, 0)
    ctx.train_set_distortion_weights(0.0, 0.01)
    _grads(ctx, probs[0])
    ctx.train_step(probs[0]["o"], probs[0]["d"], probs[0]["tgt"], 16, 24, probs[0]["u_c"], probs[0]["u_f"])
    one, steps1 = ctx.train_read_distortion_sums()
    assert steps1 == 2 and one["distortion_coarse"] == 0.0 and one["distortion_fine"] > 0.0
    ctx.train_set_distortion_weights(0.01, 0.0)
    _grads(ctx, probs[0])
    one, steps1 = ctx.train_read_distortion_sums()
    assert steps1 == 1 and one["distortion_fine"] == 0.0 and one["distortion_coarse"] > 0.0
    ctx.close()
    for k in sums:
        assert abs(sums[k] - want[k]) <= bars[k], (k, sums[k], want[k], bars[k])


# ---- 9. behaviour -----------------------------------------------------------------------------------------------------------------
BEHAVIOUR_STEPS, BEHAVIOUR_WEIGHTS = 20, (0.0, 1.0)


def test_the_regulariser_lowers_the_fine_distortion(oracle, golden_ckpt, capsys):
    """From the shipped checkpoint, BEHAVIOUR_STEPS Adam steps on one fixed batch with fixed draws, once without and once with
    the regulariser; then the fine pass's L of the weights each run ended with, read through the running sums of one
    nerf_train_gradients call under the same weights.  It ends lower with the regulariser.
    K = 20 and weights (0, 1) were chosen once, on the GPU, and were the first pair tried: L ended at 0.167408 without and at
    0.019766 with the regulariser."""
    p = S.golden_problem(oracle, golden_ckpt)
    ends = []
    for on in (False, True):
        ctx = S.golden_context(p)
        ctx.train_begin(5e-4)
        if on:
            ctx.train_set_distortion_weights(*BEHAVIOUR_WEIGHTS)
        for _ in range(BEHAVIOUR_STEPS):
            ctx.train_step(p["o"], p["d"], p["tgt"], p["sc"], p["sf"], p["u_c"], p["u_f"], want_metrics=False)
        ctx.train_read_distortion_sums()
        ctx.train_set_distortion_weights(*BEHAVIOUR_WEIGHTS)
        _grads(ctx, p)
        sums, steps = ctx.train_read_distortion_sums()
        assert steps == 1
        ends.append(sums["distortion_fine"])
        ctx.close()
    with capsys.disabled():
        print(f"\n    [behaviour] fine-pass L after {BEHAVIOUR_STEPS} steps: {ends[0]:.6f} without, {ends[1]:.6f} with the "
              f"regulariser at weights {BEHAVIOUR_WEIGHTS}", end="")
    assert np.isfinite(ends).all() and ends[1] < ends[0]


# ---- 10. errors -------------------------------------------------------------------------------------------------------------------
def test_errors_name_the_argument(oracle, golden_ckpt, op_ctx):
    from nerf_and_dietnerf_amd import _lib
    p = S.golden_problem(oracle, golden_ckpt)
    ctx = S.golden_context(p)
    for call in (lambda: ctx.train_set_distortion_weights(0.1, 0.1), ctx.train_read_distortion_sums):
        with pytest.raises(RuntimeError, match="nerf_train_begin"):
            call()
    ctx.train_begin(5e-4)
    for bad, name in (((-0.1, 0.0), "coarse"), ((float("nan"), 0.0), "coarse"), ((0.0, -1.0), "fine"),
                      ((0.0, float("nan")), "fine"), ((0.0, float("inf")), "fine")):
        with pytest.raises(RuntimeError, match=name):
            ctx.train_set_distortion_weights(*bad)
    ctx.train_set_distortion_weights(0.0, 0.0)
    ctx.close()
    w, z, _, _ = _operator_case(2)
    null = lambda *a: op_ctx.lib.nerf_distortion_loss(op_ctx.h, *a, None, None, None, _lib.NERF_MEM_HOST)   # noqa: E731
    pw, pz = w.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p)
    for args, name in (((None, pz, 5, 2), "weights"), ((pw, None, 5, 2), "z is NULL"), ((pw, pz, 5, 0), "S"),
                       ((pw, pz, 5, -3), "S"), ((pw, pz, -1, 2), "N")):
        assert null(*args) != 0
        assert name in _lib.last_error(), (name, _lib.last_error())
    assert null(pw, pz, 0, 2) == 0                       # no rays: nothing to do
    # the operator measures t between the context's bounds
    import nerf_and_dietnerf_amd as N
    flat = N.Context(near=1.0, far=1.0)
    with pytest.raises(RuntimeError, match="far_boundary > near_boundary"):
        flat.distortion_loss(w, z)
    flat.close()
