"""Training under sample culling on the device (include/nerf_mi355.h: nerf_ctx_set_train_sample_culling has the rule): the
gradients of every training entry point under the switch against the torch restatement of the culled graph
(tests/train_culling_ref.py), with the helpers and the bars tests/test_gpu_train.py uses for the un-culled step -- the arithmetic
is the same, only fewer rows run -- and bit for bit against the switch being off where the rule says so (no grid, a full grid,
the slot path against the one-call path).  Weights and rays are the golden checkpoint's; every grid is 16^3 over GOLDEN_BOX.

The restatement takes its verdicts in float64 on its own depths, the device in float32 on its own: the inputs are chosen (draw
seeds, below) so that no sample point of the restatement lies within MARGIN cell edge lengths of a cell face or a box face, and
every test asserts that before it compares."""
import numpy as np
import pytest

import culling_ref as K
import grad_blocks as GB
import occupancy_ref as G
import support as S
import train_culling_ref as TC

pytestmark = pytest.mark.gpu

FULL_GRID = np.ones((16, 16, 16), bool)
EMPTY_GRID = np.zeros((16, 16, 16), bool)
MARGIN = 1e-4
BLOCKS = GB.blocks(5, 4, 2)
# Draw seeds for which the margin condition holds in every restatement run of the test (found on the CPU with
# tests/occupancy_ref.py::z_values standing in for the device's depths) and for which float32 autograd, standing in for the
# device, passes the block-wise helpers.  The render-gradient scene took one more step.  Its bars are alpha = 1 bars, and at
# alpha = 1 the golden weights are a linear map that saturates the sigmoid on some of these rays: of the four seeds the CPU
# search gave (12, 25, 78, 138) each fails one of the inherited bars by a small factor under one policy -- the fp32 forward
# (rgb 5.4e-5 against the bar of 5e-5 at 78), the fp16 forward against its emulation (1.4e-2 against 2e-3 at 138), or blocks
# whose sums over the rows cancel to a small share of the blob max and which the device resolves to 2e-4..1e-3 of their own
# max (12, 25).  The same figures show on the same rays under a FULL grid, where every sample is kept (seed 25: k8 6.1e-4,
# seed 78: coarse 1.1e-3, float32 autograd itself at 4.5e-4 / 9.4e-4), so they are the inputs' conditioning, not the
# compaction.  Each policy therefore runs the seed on which the un-culled arithmetic class meets its own bars.
SEED_STEP, SEED_RENDER, SEED_OTHER = 4, {"float32": 138, "mixed_float16": 12}, 42


def check_conditions(p, r, grid, lo_share=0.2, hi_share=0.9, label=""):
    """What a comparison against the restatement `r` rests on: kept shares, a ragged last tile, the margin to every face."""
    shares = [float(k.mean()) for k in r["keeps"]]
    margins = [TC.face_margin(p["o"], p["d"], z, *G.GOLDEN_BOX, grid.shape[0]) for z in r["depths"]]
    print(f"\n{label} kept {[int(k.sum()) for k in r['keeps']]} of {[k.size for k in r['keeps']]} samples, margins "
          f"{[f'{m:.2e}' for m in margins]} cell edges", end="")
    assert all(lo_share <= s <= hi_share for s in shares), shares
    assert min(margins) >= MARGIN, margins
    return [int(k.sum()) for k in r["keeps"]]


# ---- 1. off is off -------------------------------------------------------------------------------------------------------------
def test_the_flag_without_a_grid_is_off(oracle, golden_ckpt):
    p = K.train_scene(oracle, golden_ckpt, 130, 8, 16, 2)
    c = K.culled_context(p, None, False)
    c.train_begin(5e-4)
    c.read_culling()
    res = []
    for flag in (False, True):
        c.set_train_sample_culling(flag)
        m, gc, gf = c.train_gradients(p["o"], p["d"], p["tgt"], 8, 16, p["u_c"], p["u_f"])
        rgb, rc, rf = c.train_render_gradients(p["o"], p["d"], p["d_rgb"], 8, 16, p["u_c"], p["u_f"])
        res.append((m, [gc, gf, rgb, rc, rf]))
        assert c.read_culling() == (0, 0)
    assert res[0][0] == res[1][0] and np.isfinite(res[0][1][0]).all() and res[0][1][0].any()
    S.assert_same_bits_each(res[1][1], res[0][1])
    # the flag outlives a grid that comes and goes, and a restarted trainer
    c.set_occupancy_grid(K.HALF_GRID)
    c.set_occupancy_grid(None)
    c.train_begin(5e-4)
    assert c.train_sample_culling
    m, gc, gf = c.train_gradients(p["o"], p["d"], p["tgt"], 8, 16, p["u_c"], p["u_f"])
    S.assert_same_bits_each([gc, gf], res[0][1][:2])
    assert m == res[0][0] and c.read_culling() == (0, 0)
    c.close()


# ---- 2. a full grid is the flag off ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trainer", ["float32", "mixed_float16", "reference"])
def test_a_full_grid_is_the_flag_off(oracle, golden_ckpt, trainer, monkeypatch):
    """Every sample kept: point mode on the gathered rows against ray mode, the gathered dL/d(raw) against the full one, the
    compact positional-encoding backward against the plain one -- bit for bit, on the fused trainer under both policies and on
    the fp32 reference trainer."""
    if trainer == "reference":
        monkeypatch.setenv("NERF_TRAIN_FORWARD", "gemm")
    n, sc, sf = 130, 8, 16
    p = K.train_scene(oracle, golden_ckpt, n, sc, sf, 6)
    res = []
    for flag in (False, True):
        c = K.culled_context(p, FULL_GRID, flag)
        c.train_begin(5e-4, mixed_float16=trainer == "mixed_float16")
        m, gc, gf = c.train_gradients(p["o"], p["d"], p["tgt"], sc, sf, p["u_c"], p["u_f"])
        assert c.read_culling() == ((n * (sc + sf),) * 2 if flag else (0, 0))
        rgb, rc, rf = c.train_render_gradients(p["o"], p["d"], p["d_rgb"], sc, sf, p["u_c"], p["u_f"])
        assert c.read_culling() == ((n * (2 * sc + sf),) * 2 if flag else (0, 0))
        res.append((m, [gc, gf, rgb, rc, rf]))
        c.close()
    assert res[0][0] == res[1][0] and np.isfinite(res[0][1][1]).all()
    assert all(g.any() for g in res[0][1])
    for name, a, b in zip(("coarse", "fine"), res[1][1][:2], res[0][1][:2]):
        GB.check_equal(a, b, BLOCKS, 0, f"full grid, {trainer}, {name}")            # (names the block that differs)
    S.assert_same_bits_each(res[1][1], res[0][1])


# ---- 3. a partial grid against the restatement -----------------------------------------------------------------------------------
def _step_against_restatement(c, p, grid, alpha, sampler, blocks, tag, capsys, flip=None, **net):
    """tests/test_gpu_train.py::test_gradients_coarse_and_fine with the culled step and the culled restatement.  A wide-PE
    network (n_pos_enc_xyz > 5) inherits the bars of ITS un-culled step, tests/test_gpu_encodings.py::
    test_training_gradients_float32_policy: the top octave multiplies the fp32 sample position by 2^9 pi, whose rounding moves
    the angle by ~1e-4 rad (alpha 1: 5e-3 of max|g|, cosine 0.9999, loss 1e-5)."""
    wide = net.get("n_pos_enc_xyz", 5) > 5
    z = c.get_z_values_for_rays(p["o"], p["d"], p["sc"], uniform_values=p["u_c"])
    args = (p["bc"], p["bf"], p["o"], p["d"], p["tgt"], z, p["u_f"], TC.grid_keep(*G.GOLDEN_BOX, grid))
    r = TC.train_gradients(*args, sampler_grad=sampler, alpha=alpha, **net)
    with capsys.disabled():
        kept = check_conditions(p, r, grid, label=tag)
    c.read_culling()
    m, gc, gf = c.train_gradients(p["o"], p["d"], p["tgt"], p["sc"], p["sf"], p["u_c"], p["u_f"])
    assert c.read_culling() == (p["n"] * (p["sc"] + p["sf"]), sum(kept))
    assert abs(m["loss"] - r["loss"]) <= (1e-5 if wide else 2e-6) * r["loss"]
    assert abs(m["psnr_coarse"] - r["psnr_coarse"]) <= 1e-4 and abs(m["psnr_fine"] - r["psnr_fine"]) <= 1e-4
    assert np.isfinite(gc).all() and np.isfinite(gf).all()
    tol, cos_min = ((5e-3 if wide else 2e-4), (0.9999 if wide else 0.9999999)) if alpha == 1.0 else (5e-2, 0.999)
    with capsys.disabled():
        print(f"\n{tag} vs float64: coarse {S.relerr(gc, r['grad_coarse']):.2e}, fine {S.relerr(gf, r['grad_fine']):.2e} of max|g|, "
              f"cosine {S.cos(gc, r['grad_coarse']):.8f}, {S.cos(gf, r['grad_fine']):.8f}", end="")
    assert S.relerr(gc, r["grad_coarse"]) <= tol and S.cos(gc, r["grad_coarse"]) > cos_min
    assert S.relerr(gf, r["grad_fine"]) <= tol and S.cos(gf, r["grad_fine"]) > cos_min
    r32 = S.f32(TC.train_gradients, *args, sampler_grad=sampler, alpha=alpha, **net)
    assert [k.sum() for k in r32["keeps"]] == [k.sum() for k in r["keeps"]]
    with capsys.disabled():
        if alpha == 1.0:
            GB.check_fp32_smooth(gc, r["grad_coarse"], r32["grad_coarse"], blocks, tol, tag + " coarse")
            GB.check_fp32_smooth(gf, r["grad_fine"], r32["grad_fine"], blocks, tol, tag + " fine")
        else:
            if not sampler:
                GB.check_fp32_masks(gc, r["grad_coarse"], r32["grad_coarse"], blocks, tag + " coarse")
            GB.check_fp32_masks(gf, r["grad_fine"], r32["grad_fine"], blocks, tag + " fine",
                                named=() if flip is None else GB.layers_up_to(blocks, flip))
    return kept, gc, gf


@pytest.mark.parametrize("alpha", [1.0, 0.05])
@pytest.mark.parametrize("sampler_gradient", [False, True])
def test_gradients_under_a_half_full_grid(oracle, golden_ckpt, sampler_gradient, alpha, capsys):
    p = K.train_scene(oracle, golden_ckpt, 48, 16, 24, SEED_STEP)
    c = K.culled_context(p, K.HALF_GRID, True, leaky_relu_alpha=alpha)
    c.train_begin(5e-4, sampler_gradient=sampler_gradient)
    tag = f"[culled 48 x (16+24), alpha {alpha:g}, sampler term {'on' if sampler_gradient else 'off'}]"
    kept, gc, gf = _step_against_restatement(c, p, K.HALF_GRID, alpha, sampler_gradient, BLOCKS, tag, capsys)
    assert any(k % 128 for k in kept)                                      # a last tile of the network kernels that is not full
    # culling did act: the un-culled step on the same depths has other gradients
    c.set_train_sample_culling(False)
    _, gc0, gf0 = c.train_gradients(p["o"], p["d"], p["tgt"], p["sc"], p["sf"], p["u_c"], p["u_f"])
    assert S.relerr(gf, gf0) > 1e-2
    c.close()


def test_mixed_float16_gradients_under_a_half_full_grid(oracle, golden_ckpt, capsys):
    """tests/test_gpu_train.py::test_mixed_float16_policy_gradients_and_loss_scaling's gradient bars, culled: against the
    restatement that rounds where the kernels round (fp16_loss_scale), block by block with check_mixed at alpha = 1.  (That test's
    distance to FLOAT64 is the arithmetic class on its own inputs and is not repeated here: the emulation pins the kernels.)"""
    p = K.train_scene(oracle, golden_ckpt, 48, 16, 24, SEED_STEP)
    scale = 32768.0
    for alpha, sg in ((1.0, True), (0.05, True), (0.05, False), (1.0, False)):
        c = K.culled_context(p, K.HALF_GRID, True, leaky_relu_alpha=alpha)
        c.train_begin(5e-4, mixed_float16=True, sampler_gradient=sg, initial_loss_scale=scale)
        z = c.get_z_values_for_rays(p["o"], p["d"], p["sc"], uniform_values=p["u_c"])
        args = (p["bc"], p["bf"], p["o"], p["d"], p["tgt"], z, p["u_f"], TC.grid_keep(*G.GOLDEN_BOX, K.HALF_GRID))
        r16 = TC.train_gradients(*args, sampler_grad=sg, alpha=alpha, fp16_loss_scale=scale)
        tag = f"[culled, mixed_float16, alpha {alpha:g}, sampler term {'on' if sg else 'off'}]"
        with capsys.disabled():
            kept = check_conditions(p, r16, K.HALF_GRID, label=tag)
        c.read_culling()
        m, gc, gf = c.train_gradients(p["o"], p["d"], p["tgt"], p["sc"], p["sf"], p["u_c"], p["u_f"])
        assert c.read_culling() == (48 * 40, sum(kept))
        c.close()
        assert np.isfinite(gc).all() and np.isfinite(gf).all()
        qc, qf = S.relerr(gc, r16["grad_coarse"]), S.relerr(gf, r16["grad_fine"])
        with capsys.disabled():
            print(f"\n{tag} vs the fp16-emulating restatement: coarse {qc:.2e}, fine {qf:.2e}; cosine "
                  f"{S.cos(gc, r16['grad_coarse']):.6f}, {S.cos(gf, r16['grad_fine']):.6f}", end="")
        if (alpha, sg) == (1.0, True):
            assert qc <= 2e-2 and qf <= 2e-3
            assert abs(m["loss"] - r16["loss"]) <= 2e-5 * r16["loss"]
        else:
            assert abs(m["loss"] - r16["loss"]) <= 1e-4 * r16["loss"]
            assert qc <= 2e-2 and qf <= 3e-2 and S.cos(gc, r16["grad_coarse"]) > 0.9999 and S.cos(gf, r16["grad_fine"]) > 0.9999
        if alpha == 1.0:                   # (the block-wise mixed bar is an alpha = 1 bar: no mask flips)
            e32 = S.f32(TC.train_gradients, *args, sampler_grad=sg, alpha=alpha, fp16_loss_scale=scale)
            with capsys.disabled():
                GB.check_mixed(gc, r16["grad_coarse"], e32["grad_coarse"], BLOCKS, tag + " coarse")
                GB.check_mixed(gf, r16["grad_fine"], e32["grad_fine"], BLOCKS, tag + " fine")


# ---- 4. render gradients and slots ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["float32", "mixed_float16"])
@pytest.mark.parametrize("sampler_gradient", [True, False])
def test_render_gradients_and_slots_under_a_half_full_grid(oracle, golden_ckpt, sampler_gradient, policy, capsys):
    """nerf_train_render_gradients under the flag against the render-gradient restatement (the fine pass masked on the merged
    depths) with the bars of test_backward_through_render (float32 policy) / test_backward_through_render_mixed_policy; then
    the slot path: forward and backward in two calls equal the one call bit for bit, also when the flag is switched off and the
    grid replaced in between -- the slot keeps its compaction record."""
    n, sc, sf = 130, 8, 16
    mixed = policy == "mixed_float16"
    scale = 32768.0 if mixed else None
    p = K.train_scene(oracle, golden_ckpt, n, sc, sf, SEED_RENDER[policy])
    c = K.culled_context(p, K.HALF_GRID, True, leaky_relu_alpha=1.0)
    c.train_begin(5e-4, sampler_gradient=sampler_gradient, mixed_float16=mixed, initial_loss_scale=scale or 0.0)
    z = c.get_z_values_for_rays(p["o"], p["d"], sc, uniform_values=p["u_c"])
    args = (p["bc"], p["bf"], p["o"], p["d"], p["d_rgb"], z, p["u_f"], TC.grid_keep(*G.GOLDEN_BOX, K.HALF_GRID))
    r = TC.render_gradients(*args, sampler_grad=sampler_gradient, alpha=1.0, fp16_loss_scale=scale)
    tag = f"[culled render(), {policy}, 130 x (8+16), sampler term {'on' if sampler_gradient else 'off'}]"
    with capsys.disabled():
        kept = check_conditions(p, r, K.HALF_GRID, label=tag)
    assert r["keeps"][1].shape == (n, sc + sf)
    c.read_culling()
    rgb, gc, gf = c.train_render_gradients(p["o"], p["d"], p["d_rgb"], sc, sf, p["u_c"], p["u_f"])
    assert c.read_culling() == (n * (2 * sc + sf), sum(kept))
    assert np.isfinite(gc).all() and np.isfinite(gf).all()
    r32 = S.f32(TC.render_gradients, *args, sampler_grad=sampler_gradient, alpha=1.0, fp16_loss_scale=scale)
    ef, cf = S.relerr(gf, r["grad_fine"]), S.cos(gf, r["grad_fine"])
    line = f"\n{tag} fine vs the restatement {ef:.2e} of max|g|, cosine {cf:.7f}"
    if mixed:
        assert np.abs(rgb - r["rgb"]).max() <= 2e-3
        assert ef <= 5e-3 and cf > 0.9999
        check = lambda g, net: GB.check_mixed(g, r["grad_" + net], r32["grad_" + net], BLOCKS, f"{tag} {net}")     # noqa: E731
        bar_c, cos_c = 3e-2, 0.999
    else:
        assert np.abs(rgb - r["rgb"]).max() <= 5e-5
        assert ef <= 2e-4 and cf > 0.9999999
        check = lambda g, net: GB.check_fp32_smooth(g, r["grad_" + net], r32["grad_" + net], BLOCKS, 2e-4, f"{tag} {net}")   # noqa: E731
        bar_c, cos_c = 2e-4, 0.9999999
    with capsys.disabled():
        check(gf, "fine")
    if sampler_gradient:
        ec, cc = S.relerr(gc, r["grad_coarse"]), S.cos(gc, r["grad_coarse"])
        line += f"; coarse (through the sampler only) {ec:.2e}, cosine {cc:.7f}"
        assert ec <= bar_c and cc > cos_c
        with capsys.disabled():
            check(gc, "coarse")
    else:
        assert not gc.any() and not r["grad_coarse"].any()
    with capsys.disabled():
        print(line, end="")
    # the slot path, bit for bit
    np.testing.assert_array_equal(c.train_render_forward(2, p["o"], p["d"], sc, sf, p["u_c"], p["u_f"]), rgb)
    sc_, sf_ = c.train_render_backward(2, p["d_rgb"])
    GB.check_equal(sc_, gc, BLOCKS, 0, "slot path, coarse")
    GB.check_equal(sf_, gf, BLOCKS, 0, "slot path, fine")
    # ... and with the flag off and another grid by the time of the backward pass
    np.testing.assert_array_equal(c.train_render_forward(0, p["o"], p["d"], sc, sf, p["u_c"], p["u_f"]), rgb)
    c.set_train_sample_culling(False)
    c.set_occupancy_grid(~K.HALF_GRID)
    c.read_culling()
    tc_, tf_ = c.train_render_backward(0, p["d_rgb"])
    assert c.read_culling() == (0, 0)                                    # the backward half compacts nothing anew
    GB.check_equal(tc_, gc, BLOCKS, 0, "slot path after the switch, coarse")
    GB.check_equal(tf_, gf, BLOCKS, 0, "slot path after the switch, fine")
    S.assert_same_bits_each([sc_, sf_, tc_, tf_], [gc, gf, gc, gf])
    c.close()


def test_a_culled_render_between_forward_and_backward_leaves_the_slot_alone(oracle, golden_ckpt):
    """The render path and the trainer run the same compaction routine, each into a record of its own: a culled render under
    another grid between a slot's forward and its backward pass overwrites the context's record and the shared scratch, and the
    slot's backward pass still equals the one call bit for bit."""
    n, sc, sf = 130, 8, 16
    p = K.train_scene(oracle, golden_ckpt, n, sc, sf, SEED_RENDER["float32"])
    c = K.culled_context(p, K.HALF_GRID, True)
    c.train_begin(5e-4)
    rgb, gc, gf = c.train_render_gradients(p["o"], p["d"], p["d_rgb"], sc, sf, p["u_c"], p["u_f"])
    c.read_culling()
    np.testing.assert_array_equal(c.train_render_forward(0, p["o"], p["d"], sc, sf, p["u_c"], p["u_f"]), rgb)
    samples, kept = c.read_culling()
    assert samples == n * (2 * sc + sf) and 0 < kept < samples            # the slot does hold a record
    c.set_sample_culling(True)
    c.set_occupancy_grid(~K.HALF_GRID)
    assert np.isfinite(c.render(p["o"], p["d"], sc, sf, p["u_c"], p["u_f"])[0]).all()
    samples, kept_render = c.read_culling()
    assert 0 < kept_render < samples and kept_render != kept              # the render did compact, to other rows
    sc_, sf_ = c.train_render_backward(0, p["d_rgb"])
    assert c.read_culling() == (0, 0)
    assert gc.any() and gf.any()
    S.assert_same_bits_each([sc_, sf_], [gc, gf])
    c.close()


def test_stage_events_belong_to_render_passes_only(oracle, golden_ckpt):
    """With timing on, a culled render pass records its six stage events and a culled training pass records none."""
    n, sc, sf = 130, 8, 16
    p = K.train_scene(oracle, golden_ckpt, n, sc, sf, 2)
    c = K.culled_context(p, K.HALF_GRID, True)
    c.set_sample_culling(True)
    c.train_begin(5e-4)
    c.enable_timing(True)
    c.read_culling_timing()
    c.read_culling()
    c.render(p["o"], p["d"], sc, sf, p["u_c"], p["u_f"])
    samples, kept = c.read_culling()
    assert 0 < kept < samples
    assert c.read_culling_timing()[1] == 2                                # the coarse pass and the fine pass
    c.train_gradients(p["o"], p["d"], p["tgt"], sc, sf, p["u_c"], p["u_f"], want_blobs=False)
    samples, kept = c.read_culling()
    assert samples == n * (sc + sf) and 0 < kept < samples                # two culled training passes ...
    assert c.read_culling_timing()[1] == 0                                # ... and no stage event
    c.close()


# ---- 5. nothing kept ---------------------------------------------------------------------------------------------------------
def _rays_inside(oracle, golden_ckpt, c, n, sc):
    """As tests/test_gpu_culling.py::test_nothing_kept: the rays that hit the box.  The trainer draws its own depths; uniform in
    disparity at draws of 0.5 they lie strictly inside the box interval (linear depths put a ray's last sample at or behind
    the far end of its interval, outside the box, where it is kept)."""
    o, d = K.camera_rays(oracle, golden_ckpt, n, spread=True)
    _, narrowed = c.ray_box_bounds(o, d)
    hit = narrowed == 1
    assert hit[:-10].sum() >= 30 and not hit[-10:].any()
    return o[hit], d[hit], o[-10:], d[-10:]


@pytest.mark.parametrize("policy", ["float32", "mixed_float16"])
def test_nothing_kept(oracle, golden_ckpt, policy):
    """An all-zero grid and rays whose depths all lie inside the box: no network kernel runs, the render is black, both gradients
    are exact zeros, and the optimizer step is an applied one.  With ten rays that miss the box the gradients are back."""
    n, sc, sf = 130, 8, 16
    p = K.train_scene(oracle, golden_ckpt, n, sc, sf, 3)
    c = K.culled_context(p, EMPTY_GRID, True)
    c.set_sampling("lindisp")
    oi, di, om, dm = _rays_inside(oracle, golden_ckpt, c, n, sc)
    ni = len(oi)
    u_c, u_f, tgt = np.full((ni, sc), 0.5, np.float32), p["u_f"][:ni], p["tgt"][:ni]
    zi = c.get_z_values_for_rays(oi, di, sc, uniform_values=u_c)
    inside, _ = K.sample_cells(oi, di, zi, *G.GOLDEN_BOX, 16, K.F32)
    assert inside.all() and not K.sample_keep(oi, di, zi, *G.GOLDEN_BOX, EMPTY_GRID, K.F32).any()
    c.train_begin(5e-4, mixed_float16=policy == "mixed_float16")
    c.read_culling()
    m, gc, gf = c.train_gradients(oi, di, tgt, sc, sf, u_c, u_f)
    assert c.read_culling() == (ni * (sc + sf), 0)
    black = float(np.mean(tgt.astype(np.float64) ** 2))
    assert np.isfinite(m["loss"]) and abs(m["loss"] - 2 * black) <= 1e-6 * black
    assert not gc.any() and not gf.any()
    rgb, rc, rf = c.train_render_gradients(oi, di, p["d_rgb"][:ni], sc, sf, u_c, u_f)
    assert c.read_culling() == (ni * (2 * sc + sf), 0)
    assert not rgb.any() and not rc.any() and not rf.any()
    w0 = c.get_weights(0)
    m = c.train_step(oi, di, tgt, sc, sf, u_c, u_f)
    assert abs(m["loss"] - 2 * black) <= 1e-6 * black
    scale, applied, skipped = c.train_loss_scale()
    assert (applied, skipped) == (1, 0)
    np.testing.assert_array_equal(c.get_weights(0), w0)                   # Adam on an exact zero gradient
    assert c.read_culling() == (ni * (sc + sf), 0)
    # the same with the ten rays that miss the box: they keep every sample
    o2, d2 = np.concatenate([oi, om]), np.concatenate([di, dm])
    u2c, u2f = np.concatenate([u_c, p["u_c"][:10]]), np.concatenate([u_f, p["u_f"][:10]])
    m, gc, gf = c.train_gradients(o2, d2, p["tgt"][:ni + 10], sc, sf, u2c, u2f)
    assert c.read_culling() == ((ni + 10) * (sc + sf), 10 * (sc + sf))
    assert np.isfinite(m["loss"]) and np.isfinite(gc).all() and np.isfinite(gf).all() and gc.any() and gf.any()
    # ... and that gradient is the ten rays' own: culling off, the ten rays alone, scaled by the share of the batch mean
    # (float32 policy: regrouping an fp32 sum, the bar of test_data_parallel_gradients_equal_full_batch; under mixed_float16
    # the 13 x larger d_rgb of the small batch rounds to other fp16 values)
    if policy == "float32":
        c.set_train_sample_culling(False)
        _, g10c, g10f = c.train_gradients(om, dm, p["tgt"][ni:ni + 10], sc, sf, p["u_c"][:10], p["u_f"][:10])
        assert S.relerr(gc * ((ni + 10) / 10.0), g10c) <= 1e-5 and S.relerr(gf * ((ni + 10) / 10.0), g10f) <= 1e-5
    c.close()


# ---- 6. one kept row ---------------------------------------------------------------------------------------------------------
ONE_ROW_RAYS, ONE_ROW_CELLS = [180, 150, 210], [(8, 9, 5), (7, 11, 2)]


def one_row_scene(oracle, golden_ckpt):
    """Three rays through the middle of the box, four coarse depths each, uniform in disparity at draws of 0.5 (strictly inside a
    ray's interval), and a grid of two cells on the first ray -- one where the ray then has a sample, one further along where it
    has none; the other two rays meet neither and lose every sample.  The pair was found on the CPU by trying the pairs of cells
    the ray crosses (tests/occupancy_ref.py::z_values for the depths) for one that keeps exactly one coarse sample with a
    non-zero gradient.  (A grid of one cell would narrow the ray to that cell and keep all four.)"""
    p = K.train_scene(oracle, golden_ckpt, 360, 4, 6, 4)
    grid = np.zeros((16, 16, 16), bool)
    for cell in ONE_ROW_CELLS:
        grid[cell] = True
    sel = ONE_ROW_RAYS
    return dict(p, o=p["o"][sel], d=p["d"][sel], n=3, u_c=np.full((3, 4), 0.5, np.float32), u_f=p["u_f"][:3], tgt=p["tgt"][:3]), grid


def test_one_kept_row(oracle, golden_ckpt, capsys):
    """One network row in the coarse pass (a padded tile of 127 empty rows), six in the fine pass: finite gradients that match
    the restatement at the alpha = 0.05 bars of the half-full grid's test.  (At alpha = 1 the golden weights are a linear map whose
    outputs saturate the sigmoid on this one sample: float32 autograd itself returns zeros there, no yardstick.)"""
    alpha = 0.05
    p, grid = one_row_scene(oracle, golden_ckpt)
    c = K.culled_context(p, grid, True, leaky_relu_alpha=alpha)
    c.set_sampling("lindisp")
    c.train_begin(5e-4)
    z = c.get_z_values_for_rays(p["o"], p["d"], p["sc"], uniform_values=p["u_c"])
    assert c.sample_occupancy(p["o"], p["d"], z).tolist() == [[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    args = (p["bc"], p["bf"], p["o"], p["d"], p["tgt"], z, p["u_f"], TC.grid_keep(*G.GOLDEN_BOX, grid))
    r = TC.train_gradients(*args, alpha=alpha)
    tag = f"[one kept coarse row, alpha {alpha:g}]"
    with capsys.disabled():
        kept = check_conditions(p, r, grid, 0.0, 1.0, tag)
    assert kept[0] == 1
    c.read_culling()
    m, gc, gf = c.train_gradients(p["o"], p["d"], p["tgt"], p["sc"], p["sf"], p["u_c"], p["u_f"])
    assert c.read_culling() == (3 * 10, sum(kept))
    assert np.isfinite(gc).all() and np.isfinite(gf).all() and gc.any()
    assert abs(m["loss"] - r["loss"]) <= 2e-6 * r["loss"]
    tol, cos_min = (2e-4, 0.9999999) if alpha == 1.0 else (5e-2, 0.999)
    with capsys.disabled():
        print(f"\n{tag} vs float64: coarse {S.relerr(gc, r['grad_coarse']):.2e}, fine "
              f"{S.relerr(gf, r['grad_fine']) if r['grad_fine'].any() else 0.0:.2e} of max|g|", end="")
    r32 = S.f32(TC.train_gradients, *args, alpha=alpha)
    for net, g in (("coarse", gc), ("fine", gf)):
        ref = r["grad_" + net]
        if not ref.any():
            assert not g.any()
            continue
        assert S.relerr(g, ref) <= tol and S.cos(g, ref) > cos_min
        with capsys.disabled():
            if alpha == 1.0:
                GB.check_fp32_smooth(g, ref, r32["grad_" + net], BLOCKS, tol, f"{tag} {net}")
            elif net == "fine":
                GB.check_fp32_masks(g, ref, r32["grad_" + net], BLOCKS, f"{tag} {net}")
    c.close()


# ---- 7. the step and the counters ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["float32", "mixed_float16"])
def test_train_step_is_gradients_plus_apply_and_counts_its_rows(oracle, golden_ckpt, policy):
    n, sc, sf = 130, 8, 16
    p = K.train_scene(oracle, golden_ckpt, n, sc, sf, 7)
    w = []
    for split in (False, True):
        c = K.culled_context(p, K.HALF_GRID, True)
        c.train_begin(5e-4, mixed_float16=policy == "mixed_float16")
        for _ in range(2):
            if split:
                c.train_gradients(p["o"], p["d"], p["tgt"], sc, sf, p["u_c"], p["u_f"], want_blobs=False)
                c.train_apply()
            else:
                c.train_step(p["o"], p["d"], p["tgt"], sc, sf, p["u_c"], p["u_f"])
        assert c.train_loss_scale()[1:] == (2, 0)
        samples, kept = c.read_culling()
        assert samples == 2 * n * (sc + sf) and 0 < kept < samples
        w.append((c.get_weights(0), c.get_weights(1)))
        if split:
            # the coarse pass's share of the counter: a coarse-only call against the verdict entry point on the same depths
            z = c.get_z_values_for_rays(p["o"], p["d"], sc, uniform_values=p["u_c"])
            want = int(c.sample_occupancy(p["o"], p["d"], z).sum())
            assert want == int(K.sample_keep(p["o"], p["d"], z, *G.GOLDEN_BOX, K.HALF_GRID, K.F32).sum())
            c.train_gradients(p["o"], p["d"], p["tgt"], sc, 0, p["u_c"], want_blobs=False)
            assert c.read_culling() == (n * sc, want) and 0 < want < n * sc
        c.close()
    S.assert_same_bits_each(w[1], w[0])
    assert not np.array_equal(w[0][0], p["bc"]) and not np.array_equal(w[0][1], p["bf"])


# ---- 8. the other networks ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [1.0, 0.05])
@pytest.mark.parametrize("lx,n_angles", [(5, 0), (5, 1), (10, 2)])
def test_the_other_networks_under_a_half_full_grid(oracle, golden_ckpt, lx, n_angles, alpha, capsys):
    """The xyz-only network, the one-angle network and a wide-PE network (10 octaves), 37 x (11+19), float32 policy,
    Glorot weights with a positive density bias: the culled step against the restatement as in test 3."""
    import nerf_and_dietnerf_amd as N
    kw = dict(n_pos_enc_xyz=lx, n_pos_enc_dir=4, n_angles=n_angles)
    p = K.train_scene(oracle, golden_ckpt, 37, 11, 19, SEED_OTHER)
    p["bc"], p["bf"] = N.glorot_blob(21, **kw), N.glorot_blob(22, **kw)
    p["bc"][-1] = p["bf"][-1] = 1.5
    c = K.culled_context(p, K.HALF_GRID, True, precision="auto", leaky_relu_alpha=alpha, **kw)
    c.train_begin(5e-4)
    tag = f"[culled 37 x (11+19), Lx {lx}, n_angles {n_angles}, alpha {alpha:g}]"
    # One LeakyReLU mask flip (tests/test_gpu_train.py has the signature; tests/test_gpu_encodings.py names its own the same way):
    # at alpha = 0.05 the xyz-only network's device forward puts one pre-activation of layer 9 of the fine pass on the other side
    # of zero than float64 -- every block of layers 0..9 is off by 2.3e-3..3.4e-3 relative L2, the two heads above (10, 11) sit
    # at the fp32 floor, and float32 autograd has no flip here (1.6e-6).  The forward's arithmetic is the un-culled step's:
    # the blocks of layers 0..9 keep the blob-wide bar, every block above is asserted.
    flip = {(5, 0, 0.05): 9}.get((lx, n_angles, alpha))
    _step_against_restatement(c, p, K.HALF_GRID, alpha, True, GB.blocks(lx, 4, n_angles), tag, capsys, flip=flip, **kw)
    c.close()


# ---- 9. the model class --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cull", [True, False])
def test_fit_trains_under_the_grid(golden_ckpt, cull):
    import nerf_and_dietnerf_amd as N
    rc = {"n_render_samples_coarse": 8, "n_render_samples_fine": 16, "scene_box": [list(G.GOLDEN_BOX[0]), list(G.GOLDEN_BOX[1])],
          "occupancy_grid": {"resolution": 16, "sigma_threshold": 10.0, "dilate": 0, "update_every": 1, "warmup_epochs": 0,
                             "cull_train_samples": cull}}
    net = dict(S.NET, n_rays_in_batch_train=64)
    m = N.NeRF(net, rc, float(golden_ckpt["near"]), float(golden_ckpt["far"]), precision="f16x3")
    m.set_weights(golden_ckpt["blob_coarse"], golden_ckpt["blob_fine"])
    assert m.ctx.train_sample_culling is cull and m.ctx.sample_culling is False
    m.compile(5e-4)
    img = golden_ckpt["img_train"][::4, ::4][:12, :11].astype(np.float32) / 255.0
    ds = N.prepare_ds(64, [golden_ckpt["c2w_train"]], [img], float(golden_ckpt["fov"]), m.ctx, seed=0)
    bakes, bake = [], m.update_occupancy_grid
    m.update_occupancy_grid = lambda *a, **k: bakes.append(bake(*a, **k)) or bakes[-1]
    m.ctx.read_culling()
    hist = N.fit(m, ds, epochs=2)
    assert len(hist) == 2 and all(np.isfinite(h["loss"]) for h in hist)
    assert len(bakes) == 2 and all(0 < b < 16 ** 3 for b in bakes)       # baked at the start of either epoch
    samples, kept = m.ctx.read_culling()
    if cull:
        assert samples == 2 * 12 * 11 * (8 + 16) and 0 < kept < samples
    else:
        assert (samples, kept) == (0, 0)
    m.ctx.close()


# ---- 10. data parallel: shards with different row counts --------------------------------------------------------------------------
def test_the_mean_of_two_shards_is_the_full_batch(oracle, golden_ckpt):
    """What a data-parallel step reduces: each rank's gradient blobs of its own shard, whatever row counts its passes kept.  Two
    shards of one batch with different kept counts, computed one after the other on one context, average to the full-batch culled
    gradients at the bar of tests/test_gpu_train.py::test_data_parallel_gradients_equal_full_batch."""
    n, sc, sf = 128, 8, 16
    p = K.train_scene(oracle, golden_ckpt, n, sc, sf, 11)
    c = K.culled_context(p, K.HALF_GRID, True)
    c.train_begin(5e-4)
    c.read_culling()
    _, gc_full, gf_full = c.train_gradients(p["o"], p["d"], p["tgt"], sc, sf, p["u_c"], p["u_f"])
    full = c.read_culling()
    parts, kept = [], []
    for sl in (slice(0, 64), slice(64, 128)):
        _, gc, gf = c.train_gradients(p["o"][sl], p["d"][sl], p["tgt"][sl], sc, sf, p["u_c"][sl], p["u_f"][sl])
        parts.append((gc, gf))
        kept.append(c.read_culling()[1])
    c.close()
    assert kept[0] != kept[1] and sum(kept) == full[1] and 0 < full[1] < full[0]
    gc = (parts[0][0].astype(np.float64) + parts[1][0]) / 2
    gf = (parts[0][1].astype(np.float64) + parts[1][1]) / 2
    assert S.relerr(gc, gc_full) <= 1e-5 and S.relerr(gf, gf_full) <= 1e-5
    GB.check_equal(gc.astype(np.float32), gc_full, BLOCKS, 1e-5, "two shards, coarse")
    GB.check_equal(gf.astype(np.float32), gf_full, BLOCKS, 1e-5, "two shards, fine")
