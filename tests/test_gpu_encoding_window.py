"""The encoding window on the device (include/nerf_mi355.h: nerf_ctx_set_encoding_window).

The window is folded into the weights while the operand streams are packed, so almost every check is bit-equality against
the same library WITHOUT a window, loaded with the blob fl32(W (.) S) that numpy computes from the reference table of
tests/encoding_window_ref.py (written from the row rule, not from the library's tables):

    forward       outputs under (W, window w)  ==  outputs under (fl32(W (.) S), no window)
    gradients     g under (W, window w)        ==  fl32(S (.) g'),  g' from a fresh trainer on fl32(W (.) S) without a window

Windows: "distinct" has all-different non-dyadic weights per octave (a swapped octave, sin / cos pair or component shows),
"zeros" is [1, 1, 0.3, 0, 0]-like with exact zeros.  Shapes: 16 rays x (8 + 8) and 7 x (33 + 32) (odd counts: row padding).
"""
import numpy as np
import pytest

import encoding_window_ref as W
import grad_blocks as GB
from occupancy_ref import GOLDEN_BOX as BOX
import support

pytestmark = pytest.mark.gpu

SHAPES = [(16, 8, 8), (7, 33, 32)]
COT = ("d_rgb", "d_depth", "d_weights", "d_z")


def _windows(lx, ld, seed=0):
    rng = np.random.default_rng(1000 + seed)

    def zeros_like(n):
        z = n // 2
        return np.array([1.0] * (n - z - 1) + [0.3] + [0.0] * z, np.float32)
    return {"distinct": ((0.1 + 0.8 * rng.random(lx)).astype(np.float32), (0.1 + 0.8 * rng.random(ld)).astype(np.float32)),
            "zeros": (zeros_like(lx), zeros_like(ld))}


def _setup(oracle, golden_ckpt, lx, ld, na):
    """Blobs and bounds: the golden checkpoint at the default geometry, else the Glorot blobs of tests/test_gpu_encodings.py."""
    import nerf_and_dietnerf_amd as N
    if (lx, ld, na) == (5, 4, 2):
        return golden_ckpt["blob_coarse"], golden_ckpt["blob_fine"], float(golden_ckpt["near"]), float(golden_ckpt["far"])
    bc, bf = N.glorot_blob(3, **support.kw(lx, ld, na)), N.glorot_blob(4, **support.kw(lx, ld, na))
    bc[-1] = bf[-1] = 1.5                   # lift sigma: Glorot networks are almost transparent
    return bc, bf, 0.5, 2.5


def _problem(oracle, n, sc, sf, near, far, na, seed=0):
    o, d, rng = support.oracle_rays(oracle, n, seed)         # n <= 64: drawn without replacement
    z = np.sort(rng.uniform(near, far, (n, sc)).astype(np.float32), axis=1)
    pts = rng.uniform(-1, 1, (3 * n + 1, 3)).astype(np.float32)
    views = None if na == 0 else rng.uniform(-1, 1, (3 * n + 1, na + 1)).astype(np.float32)
    s = sc + sf
    cot = {"d_rgb": (n, 3), "d_depth": (n,), "d_weights": (n, s), "d_z": (n, s)}
    return dict(n=n, sc=sc, sf=sf, o=o, d=d, z=z, pts=pts, views=views, u_c=rng.random((n, sc), dtype=np.float32),
                u_f=rng.random((n, sf), dtype=np.float32), tgt=rng.random((n, 3), dtype=np.float32),
                cot={k: (rng.standard_normal(v) * 0.1).astype(np.float32) for k, v in cot.items()})


def _ctx(kw, near, far, bc, bf, window=None, precision="fp32", alpha=0.05, window_first=False):
    import nerf_and_dietnerf_amd as N
    ctx = N.Context(near=near, far=far, precision=precision, leaky_relu_alpha=alpha, **kw)
    if window is not None and window_first:
        ctx.set_encoding_window(*window)
    ctx.load_weights(0, bc)
    ctx.load_weights(1, bf)
    if window is not None and not window_first:
        ctx.set_encoding_window(*window)
    return ctx


def _forward(ctx, p):
    """Every forward evaluation of test 4: [(name, array)]."""
    out = [(f"render[{i}]", a) for i, a in
           enumerate(ctx.render(p["o"], p["d"], p["sc"], p["sf"], p["u_c"], p["u_f"], want_depth=True))]
    for which in (0, 1):
        out += [(f"render_rays[{which}][{i}]", a) for i, a in enumerate(ctx.render_rays(which, p["o"], p["d"], p["z"]))]
        out.append((f"model_predict[{which}]", ctx.model_predict(which, p["pts"], p["views"])))
    ctx.set_scene_box(*BOX)
    for which in (0, 1):
        out.append((f"density_lattice[{which}]", ctx.density_lattice(which, 8)))
    ctx.set_scene_box(None)
    return [(k, np.array(v)) for k, v in out]


def _same(got, ref, label):
    assert [k for k, _ in got] == [k for k, _ in ref]
    bad = [k for (k, a), (_, b) in zip(got, ref) if a.shape != b.shape or not np.array_equal(a, b)]
    assert not bad, f"{label}: outputs differ: {bad}"
    assert all(np.isfinite(a).all() for _, a in got), label


def _draws(p):
    return (p["sc"], p["sf"], p["u_c"], p["u_f"])


def _scaled(S, g):
    return (np.asarray(S, np.float32) * np.asarray(g, np.float32)).astype(np.float32)


FORWARD_CASES = ([(5, 4, 2, prec) for prec in ("fp32", "f16x3", "bf16x3", "f16")] +
                 [(10, 4, 2, prec) for prec in ("f16x3", "bf16x3", "f16")] +
                 [(5, 4, 0, "f16x3"), (5, 4, 1, "f16x3"), (3, 2, 1, "fp32"), (10, 2, 0, "bf16x3")])


@pytest.mark.parametrize("lx,ld,na,precision", FORWARD_CASES)
def test_forward_equals_the_folded_blob_bit_for_bit(oracle, golden_ckpt, lx, ld, na, precision):
    """Test 4: render (rgb and every extra output; at f16x3 / bf16x3 with view directions its coarse pass is the sigma-only
    network), render_rays and model_predict of both networks and density_lattice(8)."""
    kw = support.kw(lx, ld, na)
    bc, bf, near, far = _setup(oracle, golden_ckpt, lx, ld, na)
    for name, (wx, wd) in _windows(lx, ld, lx + ld + na).items():
        S = W.scale_table(lx, ld, na, wx, wd)
        assert (S != 1).any()
        a = _ctx(kw, near, far, bc, bf, (wx, wd), precision)
        b = _ctx(kw, near, far, W.fold(bc, S), W.fold(bf, S), None, precision)
        got_w = a.encoding_window()
        np.testing.assert_array_equal(got_w[0], wx)
        np.testing.assert_array_equal(got_w[1], wd if na else np.ones(ld, np.float32))
        assert b.encoding_window() is None
        for n, sc, sf in SHAPES:
            p = _problem(oracle, n, sc, sf, near, far, na, seed=n)
            _same(_forward(a, p), _forward(b, p), f"({lx},{ld},{na}) {precision} {name} {n}x({sc}+{sf})")
        np.testing.assert_array_equal(a.get_weights(0), bc)         # the master weights are never scaled
        np.testing.assert_array_equal(a.get_weights(1), bf)
        a.close(); b.close()


def _train_all(ctx, p, rays=True):
    """train_gradients, then the slot forward / backward with all four cotangents (and the ray gradients)."""
    m, gc, gf = ctx.train_gradients(p["o"], p["d"], p["tgt"], *_draws(p))
    out = {"metrics": m, "gc": gc.copy(), "gf": gf.copy()}
    if rays:
        ctx.train_set_ray_gradients(True)
    fwd = ctx.train_render_forward_outputs(0, p["o"], p["d"], *_draws(p))
    out["fwd"] = {k: np.array(v) for k, v in fwd.items()}
    back = ctx.train_render_backward_outputs(0, **p["cot"], want_rays=rays)
    out["rgc"], out["rgf"] = back[0].copy(), back[1].copy()
    if rays:
        out["d_o"], out["d_d"] = back[2].copy(), back[3].copy()
        ctx.train_set_ray_gradients(False)
    return out


def test_off_is_off(oracle, golden_ckpt):
    """Test 5: never set, set to None, set to all ones, set and cleared -- the same bits everywhere; get_weights returns W
    after each, and under an active window too (with and without a trainer)."""
    lx, ld, na = 5, 4, 2
    kw = support.kw(lx, ld, na)
    bc, bf, near, far = _setup(oracle, golden_ckpt, lx, ld, na)
    wx, wd = _windows(lx, ld)["distinct"]
    p = _problem(oracle, *SHAPES[0], near, far, na)
    results = {}
    for how in ("never", "none", "ones", "cleared"):
        ctx = _ctx(kw, near, far, bc, bf, precision="f16x3")
        if how == "none":
            ctx.set_encoding_window(None, None)
        elif how == "ones":
            ctx.set_encoding_window(np.ones(lx), np.ones(ld))
        elif how == "cleared":
            ctx.set_encoding_window(wx, wd)
            assert ctx.encoding_window() is not None
            np.testing.assert_array_equal(ctx.get_weights(0), bc)
            ctx.set_encoding_window()
        assert ctx.encoding_window() is None
        fwd = _forward(ctx, p)
        ctx.train_begin(5e-4)
        if how == "cleared":                     # ... and through a trainer: on, a pass, off again
            ctx.set_encoding_window(wx, wd)
            ctx.train_gradients(p["o"], p["d"], p["tgt"], *_draws(p))
            np.testing.assert_array_equal(ctx.get_weights(1), bf)
            ctx.set_encoding_window(None, None)
        results[how] = (fwd, _train_all(ctx, p))
        ctx.train_end()
        np.testing.assert_array_equal(ctx.get_weights(0), bc)
        np.testing.assert_array_equal(ctx.get_weights(1), bf)
        ctx.close()
    ref_f, ref_t = results["never"]
    for how in ("none", "ones", "cleared"):
        f, t = results[how]
        _same(f, ref_f, how)
        assert t["metrics"] == ref_t["metrics"], how
        for k in ("gc", "gf", "rgc", "rgf", "d_o", "d_d"):
            assert np.array_equal(t[k], ref_t[k]), (how, k)
        for k in ref_t["fwd"]:
            assert np.array_equal(t["fwd"][k], ref_t["fwd"][k]), (how, k)


@pytest.mark.parametrize("lx,ld,na", [(5, 4, 2), (10, 4, 2), (3, 2, 0), (4, 3, 1)])
@pytest.mark.parametrize("sampler_gradient", [True, False])
def test_trainer_gradients_float32_policy(oracle, golden_ckpt, lx, ld, na, sampler_gradient):
    """Test 6, float32 policy: train_gradients and the slot forward / backward with all four cotangents and the ray gradients."""
    kw = support.kw(lx, ld, na)
    bc, bf, near, far = _setup(oracle, golden_ckpt, lx, ld, na)
    blocks = GB.blocks(lx, ld, na)
    prec = "fp32" if lx <= 5 else "f16x3"
    for name, (wx, wd) in _windows(lx, ld, 7 * lx + na).items():
        S = W.scale_table(lx, ld, na, wx, wd)
        for n, sc, sf in SHAPES:
            label = f"({lx},{ld},{na}) sampler {sampler_gradient} {name} {n}x({sc}+{sf})"
            p = _problem(oracle, n, sc, sf, near, far, na, seed=n + 1)
            a = _ctx(kw, near, far, bc, bf, (wx, wd), prec)
            b = _ctx(kw, near, far, W.fold(bc, S), W.fold(bf, S), None, prec)
            res = []
            for ctx in (a, b):
                ctx.train_begin(5e-4, sampler_gradient=sampler_gradient)
                res.append(_train_all(ctx, p))
                ctx.close()
            ra, rb = res
            assert ra["metrics"] == rb["metrics"], label
            for k in ("gc", "gf", "rgc", "rgf"):
                # (render()'s outputs reach the coarse network through the sampler alone: without its term that blob is zero)
                assert np.abs(rb[k]).max() > 0 or (k == "rgc" and not sampler_gradient), (label, k)
                GB.check_equal(ra[k], _scaled(S, rb[k]), blocks, 0, f"{label} {k}")
            for k in rb["fwd"]:
                assert np.array_equal(ra["fwd"][k], rb["fwd"][k]), (label, k)
            for k in ("d_o", "d_d"):
                assert np.abs(rb[k]).max() > 0 and np.array_equal(ra[k], rb[k]), (label, k)


def test_trainer_gradients_mixed_float16_policy(oracle, golden_ckpt):
    """Test 6, mixed_float16: equal wherever S is 0 or 1, within 1 ulp (fp32) elsewhere -- the loss scale, a power of two, is
    taken off after the window's factor instead of before it --, the same loss scale and the same verdict."""
    lx, ld, na = 5, 4, 2
    kw = support.kw(lx, ld, na)
    bc, bf, near, far = _setup(oracle, golden_ckpt, lx, ld, na)
    for name, (wx, wd) in _windows(lx, ld, 3).items():
        S = W.scale_table(lx, ld, na, wx, wd)
        exact = (S == 0) | (S == 1)
        for n, sc, sf in SHAPES:
            p = _problem(oracle, n, sc, sf, near, far, na, seed=n + 2)
            res, scales = [], []
            for blobs, window in (((bc, bf), (wx, wd)), ((W.fold(bc, S), W.fold(bf, S)), None)):
                ctx = _ctx(kw, near, far, *blobs, window, "f16x3")
                ctx.train_begin(5e-4, mixed_float16=True)
                res.append(_train_all(ctx, p))
                scales.append(ctx.train_loss_scale())
                ctx.close()
            ra, rb = res
            assert scales[0] == scales[1] and ra["metrics"] == rb["metrics"]
            for k in ("gc", "gf", "rgc", "rgf"):
                want = _scaled(S, rb[k])
                assert np.isfinite(ra[k]).all() and np.abs(want).max() > 0
                assert np.array_equal(ra[k][exact], want[exact]), (name, k)
                assert (np.abs(ra[k] - want) <= np.spacing(np.abs(want))).all(), (name, k)
            for k in rb["fwd"]:
                assert np.array_equal(ra["fwd"][k], rb["fwd"][k]), (name, k)
            for k in ("d_o", "d_d"):
                assert np.array_equal(ra[k], rb[k]), (name, k)


def test_trainer_gradients_reference_trainer(oracle, golden_ckpt, monkeypatch):
    """Test 6, the exact-fp32 layer-wise trainer (NERF_TRAIN_FORWARD=gemm): launch_relayout and its reductions."""
    monkeypatch.setenv("NERF_TRAIN_FORWARD", "gemm")
    lx, ld, na = 5, 4, 2
    kw = support.kw(lx, ld, na)
    bc, bf, near, far = _setup(oracle, golden_ckpt, lx, ld, na)
    wx, wd = _windows(lx, ld, 5)["distinct"]
    S = W.scale_table(lx, ld, na, wx, wd)
    p = _problem(oracle, *SHAPES[1], near, far, na, seed=4)
    res = []
    for blobs, window in (((bc, bf), (wx, wd)), ((W.fold(bc, S), W.fold(bf, S)), None)):
        ctx = _ctx(kw, near, far, *blobs, window)
        ctx.train_begin(5e-4)
        res.append(ctx.train_gradients(p["o"], p["d"], p["tgt"], *_draws(p)))
        ctx.close()
    (ma, gca, gfa), (mb, gcb, gfb) = res
    assert ma == mb
    GB.check_equal(gca, _scaled(S, gcb), GB.blocks(lx, ld, na), 0, "reference trainer, coarse")
    GB.check_equal(gfa, _scaled(S, gfb), GB.blocks(lx, ld, na), 0, "reference trainer, fine")


def test_accumulate_does_not_rescale_what_is_there(oracle, golden_ckpt):
    """Test 7: tests/test_gpu_render_outputs.py::test_accumulate_adds_to_the_ray_loss_gradients under a window -- the
    accumulated blob is the sum of the two calls' gradients to 1e-6 of max|g| (a first contribution scaled a second time
    would miss by 1 - w of its windowed rows)."""
    lx, ld, na = 5, 4, 2
    bc, bf, near, far = _setup(oracle, golden_ckpt, lx, ld, na)
    wx, wd = _windows(lx, ld, 9)["distinct"]
    p = _problem(oracle, *SHAPES[0], near, far, na, seed=5)
    ctx = _ctx(support.kw(lx, ld, na), near, far, bc, bf, (wx, wd), alpha=1.0)
    ctx.train_begin(5e-4)
    ctx.train_render_forward_outputs(0, p["o"], p["d"], *_draws(p), outputs=("rgb",))
    gc, gf = ctx.train_render_backward_outputs(0, **p["cot"])
    _, gc1, gf1 = ctx.train_gradients(p["o"], p["d"], p["tgt"], *_draws(p))
    ctx.train_render_forward_outputs(0, p["o"], p["d"], *_draws(p), outputs=("rgb",))
    gc2, gf2 = ctx.train_render_backward_outputs(0, **p["cot"], accumulate=True)
    assert np.abs(gf2 - (gf1 + gf)).max() <= 1e-6 * np.abs(gf2).max()
    assert np.abs(gc2 - (gc1 + gc)).max() <= 1e-6 * max(np.abs(gc2).max(), 1e-30)
    # ... and a third call on top, through train_render_backward
    ctx.train_render_forward(0, p["o"], p["d"], *_draws(p))
    gc3, gf3 = ctx.train_render_backward(0, p["cot"]["d_rgb"], accumulate=True)
    ctx.train_render_forward(0, p["o"], p["d"], *_draws(p))
    gc0, gf0 = ctx.train_render_backward(0, p["cot"]["d_rgb"])
    assert np.abs(gf3 - (gf2 + gf0)).max() <= 1e-6 * np.abs(gf3).max()
    assert np.abs(gc3 - (gc2 + gc0)).max() <= 1e-6 * max(np.abs(gc3).max(), 1e-30)
    ctx.close()


@pytest.mark.parametrize("mixed", [False, True])
def test_optimizer_leaves_closed_rows_alone(oracle, golden_ckpt, mixed):
    """Test 8: one train_step under a window with zeros leaves every master weight whose S is 0 at its initial bits and
    moves the rows with S > 0; train_step is train_gradients + train_apply under the same window, bit for bit."""
    lx, ld, na = 5, 4, 2
    kw = support.kw(lx, ld, na)
    bc, bf, near, far = _setup(oracle, golden_ckpt, lx, ld, na)
    wx, wd = _windows(lx, ld)["zeros"]
    S = W.scale_table(lx, ld, na, wx, wd)
    p = _problem(oracle, *SHAPES[0], near, far, na, seed=6)
    a = _ctx(kw, near, far, bc, bf, (wx, wd))
    a.train_begin(5e-4, mixed_float16=mixed)
    a.train_step(p["o"], p["d"], p["tgt"], *_draws(p))
    b = _ctx(kw, near, far, bc, bf, (wx, wd))
    b.train_begin(5e-4, mixed_float16=mixed)
    b.train_gradients(p["o"], p["d"], p["tgt"], *_draws(p), want_blobs=False)
    b.train_apply()
    assert a.train_loss_scale() == b.train_loss_scale() and a.train_loss_scale()[1] == 1
    for which, w0 in ((0, bc), (1, bf)):
        wa = a.get_weights(which)
        np.testing.assert_array_equal(wa, b.get_weights(which))
        assert (S == 0).any() and np.array_equal(wa[S == 0], w0[S == 0])
        for name, ix in GB.blocks(lx, ld, na):
            if name in ("k0", "k4[xyz]", "k8[dir]", "k10[dir]"):
                rows = S[ix].reshape(-1, W.layer_shapes(lx, ld, na)[int(name[1:].split("[")[0])][1])
                moved = (wa[ix] != w0[ix]).reshape(rows.shape)
                assert moved[rows[:, 0] > 0].any(axis=1).all(), (which, name)      # every open row moved somewhere
    a.close(); b.close()


def test_order_change_and_persistence(oracle, golden_ckpt):
    """Test 9: (set, load) == (load, set); a changed window makes the next train_gradients a fresh trainer's under the new
    one; train_begin / train_end leave it in place; no change while a render slot holds a forward pass (the rule chosen)."""
    lx, ld, na = 5, 4, 2
    kw = support.kw(lx, ld, na)
    bc, bf, near, far = _setup(oracle, golden_ckpt, lx, ld, na)
    wins = _windows(lx, ld, 11)
    w1, w2 = wins["distinct"], wins["zeros"]
    p = _problem(oracle, *SHAPES[1], near, far, na, seed=7)
    a = _ctx(kw, near, far, bc, bf, w1, "f16x3", window_first=True)
    b = _ctx(kw, near, far, bc, bf, w1, "f16x3", window_first=False)
    _same(_forward(a, p), _forward(b, p), "set-then-load vs load-then-set")
    a.train_begin(5e-4)
    np.testing.assert_array_equal(a.encoding_window()[0], w1[0])
    a.train_gradients(p["o"], p["d"], p["tgt"], *_draws(p))
    a.set_encoding_window(*w2)
    second = a.train_gradients(p["o"], p["d"], p["tgt"], *_draws(p))
    b.set_encoding_window(*w2)
    b.train_begin(5e-4)
    fresh = b.train_gradients(p["o"], p["d"], p["tgt"], *_draws(p))
    assert second[0] == fresh[0] and np.array_equal(second[1], fresh[1]) and np.array_equal(second[2], fresh[2])
    # the slot rule
    a.train_render_forward(0, p["o"], p["d"], *_draws(p))
    with pytest.raises(RuntimeError, match="render slot 0 holds a forward pass"):
        a.set_encoding_window(*w1)
    np.testing.assert_array_equal(a.encoding_window()[0], w2[0])
    a.train_render_backward(0, p["cot"]["d_rgb"])
    a.set_encoding_window(*w1)
    a.train_end()
    got = a.encoding_window()
    np.testing.assert_array_equal(got[0], w1[0]); np.testing.assert_array_equal(got[1], w1[1])
    # ... and the render path after train_end still runs under it
    b.train_end()
    b.set_encoding_window(*w1)
    _same(_forward(a, p), _forward(b, p), "after train_end")
    # validation: the range and the offending index
    with pytest.raises(RuntimeError, match=r"\[0, 1\].*w_xyz\[2\]"):
        a.set_encoding_window([1, 1, 1.5, 1, 1], None)
    with pytest.raises(RuntimeError, match=r"\[0, 1\].*w_dir\[3\]"):
        a.set_encoding_window(None, [1, 1, 1, float("nan")])
    with pytest.raises(ValueError, match="5 values"):
        a.set_encoding_window([1, 1, 1], None)
    a.close(); b.close()
    # w_dir on an xyz-only context: accepted, no effect
    c = None
    import nerf_and_dietnerf_amd as N
    c = N.Context(near=near, far=far, precision="f16x3", **support.kw(5, 4, 0))
    c.set_encoding_window(None, [0.5, 0.5, 0.5, 0.5])
    assert c.encoding_window() is None
    c.close()


def test_fit_follows_the_schedule(oracle, golden_ckpt):
    """Test 10: the config key through NeRF.compile and fit(): epoch 0's window after compile, every epoch's at its start,
    off once the schedule has run out."""
    import torch
    import nerf_and_dietnerf_amd as N
    lx, ld, na = 5, 4, 2
    bc, bf, near, far = _setup(oracle, golden_ckpt, lx, ld, na)
    net_cfg = {"hidden_layer_dim": 256, "last_hidden_layer_dim": 128, "leaky_relu_alpha": 0.05, "n_pos_enc_dim_xyz": lx,
               "n_pos_enc_view_dir": ld, "n_angles_for_model": na, "n_rays_in_batch_train": 16, "n_rays_in_batch_render": 16}
    ren = {"n_render_samples_coarse": 8, "n_render_samples_fine": 8,
           "encoding_window": {"kind": "cosine", "start": 1.5, "epochs": 2, "dirs": True}}
    model = N.NeRF(net_cfg, ren, near, far)
    model.set_weights(bc, bf)
    assert model.ctx.encoding_window() is None
    model.compile(5e-4)
    p = _problem(oracle, 32, 8, 8, near, far, na, seed=8)
    ds = N.RayDataset(*(torch.as_tensor(p[k], device="cuda") for k in ("o", "d")),
                      torch.as_tensor(np.tile(p["tgt"], (1, 1)), device="cuda"), 16)
    seen = []
    hook = model.encoding_window_epoch

    def spy():
        hook()
        seen.append(model.ctx.encoding_window())
    model.encoding_window_epoch = spy

    def expect(e):
        alpha = 1.5 + (5.0 - 1.5) * min(e / 2, 1.0)
        return W.cosine_window(alpha, lx).astype(np.float32), W.cosine_window(alpha * ld / lx, ld).astype(np.float32)
    np.testing.assert_array_equal(model.ctx.encoding_window()[0], expect(0)[0])      # compile applied epoch 0
    hist = N.fit(model, ds, epochs=2)
    assert len(hist) == 2 and len(seen) == 2 and all(np.isfinite(h["loss"]) for h in hist)
    for e in (0, 1):
        np.testing.assert_array_equal(seen[e][0], expect(e)[0])
        np.testing.assert_array_equal(seen[e][1], expect(e)[1])
    assert not np.array_equal(seen[0][0], seen[1][0])
    N.fit(model, ds, epochs=1)                    # epoch 2 = the schedule's end: alpha = L, the window is off
    assert seen[2] is None and model.ctx.encoding_window() is None
    model.ctx.close()
