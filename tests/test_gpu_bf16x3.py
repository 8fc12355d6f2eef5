"""The bf16x3 render mode on the device (precision="bf16x3", NERF_PRECISION_BF16X3; csrc/mlp_bf16x3.hip,
mlp_bf16x3_wide.hip): fp32-class results -- 1e-4 RGB against the fp32 oracle -- with fp32's exponent range.

Every test here fails on a library without the mode (the context cannot be created).  Shared inputs, weights and the CPU
emulation of the kernels' arithmetic: tests/bf16_variants.py; the CPU side of the same checks: tests/test_bf16x3_host.py.

Raw outputs, kernel against the emulation of its own arithmetic: the bar is 4 x the emulation's own error against the
fp32 oracle on the same inputs (relative to max(1, |ref|)); the factor covers the order of the fp32 additions inside the
MFMA, which the emulation does not model.  The test measures the figure on the CPU when it runs; measured when the mode
was built (coarse / fine network of bf16_variants.blobs, 4173 rows):
    (5,4,2)  3.84e-6 / 4.96e-6   -> bar 1.53e-5 / 1.99e-5        (3,2,2)   4.08e-6 / 3.24e-6   -> 1.63e-5 / 1.30e-5
    (5,4,1)  3.89e-6 / 3.75e-6   -> bar 1.56e-5 / 1.50e-5        (10,4,2)  3.91e-6 / 5.15e-6   -> 1.56e-5 / 2.06e-5
    (5,4,0)  4.43e-6 / 4.14e-6   -> bar 1.77e-5 / 1.66e-5        (7,2,0)   4.34e-6 / 4.86e-6   -> 1.74e-5 / 1.94e-5"""
import types

import numpy as np
import pytest

import bf16_variants as B
import support as S
from video_ref import (DEPTH_BAR, DEPTH_MEAN_BAR, DEPTH_SELF_MARGIN, NET, RGB_BAR, RGB_MEAN_BAR, RGB_SELF_MARGIN,
                       frames, psnr, scene, tours)  # noqa: F401  (frames, scene: fixtures)

pytestmark = pytest.mark.gpu

NEAR, FAR = 0.6, 2.4
WEIGHTS_ONLY, WITH_RGB = ("weights",), ("weights", "rgb")      # outputs {weights}: the sigma-only path; with rgb: the full network


# ---- 1. parity ----
@pytest.mark.parametrize("lx,ld,na", B.GEOMETRIES)
def test_parity_with_the_oracle_and_with_its_own_emulation(oracle, lx, ld, na, capsys):
    """render with explicit draws (64 rays, 64 + 128) and render_image against the fp32 oracle: RGB <= 1e-4; model_predict
    against the emulation of the kernel's arithmetic at 4 x the emulation's own error (module docstring), and against
    the oracle; nothing non-finite."""
    bc, bf = B.blobs(lx, ld, na)
    kw = B.kw(lx, ld, na)
    ctx = S.blob_context((bc, bf), lx, ld, na, precision="bf16x3")
    try:
        coarse, fine = oracle.unpack_blob(bc, **kw), oracle.unpack_blob(bf, **kw)
        o, d, rng = B.rays(64, 2 + lx + 7 * ld + 31 * na)
        uc, uf = rng.random((64, 64), dtype=np.float32), rng.random((64, 128), dtype=np.float32)
        got = ctx.render(o, d, 64, 128, uc, uf)
        ref = oracle.render(coarse, fine, o, d, NEAR, FAR, uc, uf, **kw)
        e_render = float(np.abs(got[0] - ref[0]).max())
        c2w = oracle.get_sphere_matrix(1.0, -25.0, 40.0, 0.0).astype(np.float32)
        img = ctx.render_image(c2w, 0.6, 32, 32, 4096, 64, 128, seed=7)
        ref_img = oracle.render_image(coarse, fine, c2w, 0.6, 32, 32, NEAR, FAR, 64, 128, seed=7, **kw)
        e_img = float(np.abs(img[0] - ref_img[0]).max())
        with capsys.disabled():
            print(f"\n[bf16x3 ({lx},{ld},{na})] RGB vs oracle: render {e_render:.2e}, render_image {e_img:.2e}", end="")
        assert np.isfinite(got[0]).all() and np.isfinite(img[0]).all()
        assert e_render <= B.RGB_BAR and e_img <= B.RGB_BAR
        xyz, dirs = B.inputs(B.RAW_ROWS, na)
        for which, (layers, ref_raw, emu_raw, fig) in enumerate(B.raw_figures(lx, ld, na)):
            raw = ctx.model_predict(which, xyz, dirs)
            e_emu, e_ref, bar = B.rel_err(raw, emu_raw), B.rel_err(raw, ref_raw), B.RAW_BAR_FACTOR * fig
            with capsys.disabled():
                print(f"\n[bf16x3 ({lx},{ld},{na}) net {which}] raw: emulation vs oracle {fig:.3e} -> bar {bar:.3e}; kernel vs "
                      f"emulation {e_emu:.3e}, kernel vs oracle {e_ref:.3e}", end="")
            assert np.isfinite(raw).all()
            assert e_emu <= bar, (which, e_emu, bar)
        assert ctx.read_nonfinite() == 0
    finally:
        ctx.close()


# ---- 2. range ----
def test_range_beyond_fp16(oracle, golden_ckpt, capsys):
    """The shipped coarse network with layer 1 x 3e4 and layer 2 / 3e4 (the same function; the CPU side is
    test_bf16x3_host.py::test_range_blob_...), rendered out to depth 6 where layer-1 activations pass 65504: f16x3 counts
    non-finite rows, bf16x3 counts none, is finite and within 1e-4 RGB of the oracle."""
    near, far = B.RANGE_BOUNDS
    big, bf = B.range_blob(golden_ckpt["blob_coarse"]), golden_ckpt["blob_fine"]
    c2w, fov = golden_ckpt["c2w_test"], float(golden_ckpt["fov"])
    ref = oracle.render_image(oracle.unpack_blob(big), oracle.unpack_blob(bf), c2w, fov, 12, 12, near, far, 64, 128, seed=3)[0]
    assert np.isfinite(ref).all()
    f16 = S.blob_context((big, bf), precision="f16x3", near=near, far=far)
    bf16 = S.blob_context((big, bf), near=near, far=far, precision="bf16x3")
    try:
        f16.render_image(c2w, fov, 12, 12, 0, 64, 128, seed=3)
        n16 = f16.read_nonfinite()
        img = bf16.render_image(c2w, fov, 12, 12, 0, 64, 128, seed=3)[0]
        nbf = bf16.read_nonfinite()
        err = float(np.abs(img - ref).max())
        with capsys.disabled():
            print(f"\n[range blob] non-finite rows: f16x3 {n16}, bf16x3 {nbf}; bf16x3 RGB vs oracle {err:.2e}", end="")
        assert n16 > 0
        assert nbf == 0 and np.isfinite(img).all() and err <= B.RGB_BAR
    finally:
        f16.close()
        bf16.close()


# ---- 3. sigma-only coarse pass ----
@pytest.mark.parametrize("lx,ld,na", [(5, 4, 2), (5, 4, 1), (3, 2, 2)])
def test_sigma_only_coarse_pass_is_bit_identical(oracle, lx, ld, na):
    """A coarse render_rays that asks for the weights alone runs mlp_bf16x3_sig_kernel; with rgb as well, the full kernel:
    the same bits, from one row to every workgroup looping twice.  And an rgb-only render_image equals the render with all
    six outputs."""
    ctx = S.blob_context(B.blobs(lx, ld, na), lx, ld, na, precision="bf16x3")
    try:
        for n, s in [(1, 1), (1, 64), (37, 64), (129, 3), (2 * S.n_cus() * 128 + 77, 1), (2 * S.n_cus() * 2 + 1, 64)]:
            o, d, z = S.rays_towards_origin(n, s, NEAR, FAR)
            full = S.render_rays(ctx, 0, o, d, z, WITH_RGB)[0]
            S.assert_same_bits(S.render_rays(ctx, 0, o, d, z, WEIGHTS_ONLY)[0], full, f"({lx},{ld},{na}) N={n} S={s}", finite=True)
            if s > 1 and n > 1:
                assert full.max() > 1e-3
        c2w = oracle.get_sphere_matrix(1.0, -25.0, 40.0, 0.0).astype(np.float32)
        all_six = ctx.render_image(c2w, 0.6, 40, 40, 0, 64, 128, seed=5)
        only = ctx.render_image(c2w, 0.6, 40, 40, 0, 64, 128, seed=5, rgb_only=True)
        S.assert_same_bits(only[0], all_six[0], "rgb-only render_image vs all six outputs", finite=True)
        assert ctx.read_nonfinite() == 0
    finally:
        ctx.close()


# ---- 4. invariance ----
def test_batch_slab_and_mode_switch_invariance(oracle, golden_ckpt):
    """Batch size and slab decomposition do not change a bit of a bf16x3 render_image; f16x3 -> bf16x3 -> f16x3 on one
    context leaves the f16x3 result as it was."""
    c2w, fov = golden_ckpt["c2w_test"], float(golden_ckpt["fov"])
    near, far = float(golden_ckpt["near"]), float(golden_ckpt["far"])
    ctx = S.blob_context((golden_ckpt["blob_coarse"], golden_ckpt["blob_fine"]), precision="f16x3", near=near, far=far)
    try:
        h = w = 48
        before = ctx.render_image(c2w, fov, h, w, 0, 64, 128, seed=9)
        ctx.set_precision("bf16x3")
        whole = ctx.render_image(c2w, fov, h, w, 0, 64, 128, seed=9)
        assert np.count_nonzero(whole[0] != before[0]) > 0                    # another arithmetic, not the same kernel
        for batch in (128, 777, 4096):
            part = ctx.render_image(c2w, fov, h, w, batch, 64, 128, seed=9)
            for i, (a, b) in enumerate(zip(part, whole)):
                S.assert_same_bits(a, b, f"batch {batch}, output {i}", finite=True)
        cuts = [0, 1, 130, 1000, 1777, h * w]
        slabs = [ctx.render_image(c2w, fov, h, w, 512, 64, 128, seed=9, ray_begin=a, ray_count=b - a)
                 for a, b in zip(cuts[:-1], cuts[1:])]
        for i in range(6):
            glued = np.concatenate([np.asarray(s[i]) for s in slabs])
            S.assert_same_bits(glued, np.asarray(whole[i]).reshape(glued.shape), f"slabs, output {i}", finite=True)
        ctx.set_precision("f16x3")
        after = ctx.render_image(c2w, fov, h, w, 0, 64, 128, seed=9)
        for i, (a, b) in enumerate(zip(after, before)):
            S.assert_same_bits(a, b, f"f16x3 after the switch, output {i}", finite=True)
        assert ctx.read_nonfinite() == 0
    finally:
        ctx.close()


# ---- 5. after training ----
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("lx,ld,na", [(5, 4, 2), (10, 4, 2), (5, 4, 0)])
def test_render_after_train_steps_matches_fresh_context(oracle, lx, ld, na, mixed):
    """A bf16x3 render_image between optimizer steps (either policy) reads the device re-pack of the trained weights: the
    same bits as a fresh bf16x3 context loaded with get_weights()."""
    rng = np.random.default_rng(7)
    n, sc, sf = 512, 64, 128
    o, d, _ = S.rays_towards_origin(n, 1, NEAR, FAR, seed=9)
    tgt = rng.random((n, 3), dtype=np.float32)
    u_c, u_f = rng.random((n, sc), dtype=np.float32), rng.random((n, sf), dtype=np.float32)
    c2w = oracle.get_sphere_matrix(1.0, -25.0, 40.0, 0.0).astype(np.float32)
    trained = S.blob_context(B.blobs(lx, ld, na), lx, ld, na, precision="bf16x3")
    fresh = None
    try:
        start = trained.render_image(c2w, 0.6, 32, 32, 0, sc, sf, seed=4)
        trained.train_begin(5e-4, mixed_float16=mixed, initial_loss_scale=1024.0 if mixed else 0.0)
        for _ in range(3):
            trained.train_step(o, d, tgt, sc, sf, u_c, u_f)
        got = trained.render_image(c2w, 0.6, 32, 32, 0, sc, sf, seed=4)
        assert np.count_nonzero(got[0] != start[0]) > 0                       # the weights moved
        fresh = S.blob_context((trained.get_weights(0), trained.get_weights(1)), lx, ld, na, precision="bf16x3")
        want = fresh.render_image(c2w, 0.6, 32, 32, 0, sc, sf, seed=4)
        for i, (a, b) in enumerate(zip(got, want)):
            S.assert_same_bits(a, b, f"trained vs fresh, output {i}", finite=True)
        trained.train_end()
    finally:
        trained.close()
        if fresh is not None:
            fresh.close()


@pytest.mark.parametrize("lx,na", [(5, 2), (5, 0), (7, 2), (7, 0)])
def test_every_resident_stream_follows_reloads_and_train_steps(oracle, lx, na):
    """One context, switched through every precision its config has a kernel for (fp32 only at Lx <= 5), renders the same
    bits as a fresh context created in that precision: (a) after the first load_weights, (b) after a second load_weights
    onto the streams already allocated, (c) after three train_steps (the device re-pack of every stream) and after a
    load_weights under the running trainer.  67 rays x (12 coarse, 12 + 20 fine) samples: 804 and 2144 rows, a ragged last
    128-row tile in both passes.  The four configs are the four classes csrc/nerf_kernels.h::render_streams tells apart."""
    n, sc, sf = 67, 12, 20
    o, d, rng = B.rays(n, seed=21)
    tgt = rng.random((n, 3), dtype=np.float32)
    u_c, u_f = rng.random((n, sc), dtype=np.float32), rng.random((n, sf), dtype=np.float32)
    precisions = (["fp32"] if lx <= 5 else []) + ["f16x3", "f16", "bf16x3"]

    def check(ctx, pair, label):
        for p in precisions:
            ctx.set_precision(p)
            got = ctx.render(o, d, sc, sf, u_c, u_f)
            fresh = S.blob_context(pair, lx, 4, na, precision=p)
            try:
                want = fresh.render(o, d, sc, sf, u_c, u_f)
            finally:
                fresh.close()
            for i, (a, b) in enumerate(zip(got, want)):
                np.testing.assert_array_equal(a, b, err_msg=f"{label}, {p}, output {i}")

    first, second, third = (B.blobs(lx, 4, na, seed=s) for s in (11, 31, 51))
    ctx = S.blob_context(first, lx, 4, na, precision=precisions[0])
    try:
        check(ctx, first, "(a) first load")
        for which, blob in enumerate(second):
            ctx.load_weights(which, blob)
        check(ctx, second, "(b) second load")
        ctx.train_begin(5e-4)
        for _ in range(3):
            ctx.train_step(o, d, tgt, sc, sf, u_c, u_f)
        trained = (ctx.get_weights(0), ctx.get_weights(1))
        assert np.count_nonzero(trained[0] != second[0]) > 0 and np.count_nonzero(trained[1] != second[1]) > 0
        check(ctx, trained, "(c) after three train steps")
        for which, blob in enumerate(third):
            ctx.load_weights(which, blob)
        check(ctx, third, "(c) load under the running trainer")
        ctx.train_end()
    finally:
        ctx.close()


@pytest.mark.parametrize("lx,ld,na", [(5, 4, 2), (3, 2, 1), (8, 4, 2), (5, 4, 0)])
def test_reloading_a_blob_gives_its_first_render_again(oracle, lx, ld, na):
    """nerf_load_weights re-packs every resident stream from the blob on the device, onto the streams the first load
    allocated and in stream order behind the renders already enqueued.  Load A, render, load B, load A again: in every
    precision the config has a kernel for (fp32 only at Lx <= 5) the last render has the bits of the first and of a fresh
    context created in that precision, and B's render in between had others.  64 rays x (12 coarse, 12 + 20 fine)
    samples; one config per class csrc/nerf_kernels.h::render_streams tells apart, one of them with fewer octaves than
    the layout its tables are written for."""
    n, sc, sf = 64, 12, 20
    o, d, rng = B.rays(n, seed=23)
    u_c, u_f = rng.random((n, sc), dtype=np.float32), rng.random((n, sf), dtype=np.float32)
    precisions = (["fp32"] if lx <= 5 else []) + ["f16x3", "f16", "bf16x3"]
    blob_a, blob_b = B.blobs(lx, ld, na, seed=13), B.blobs(lx, ld, na, seed=33)

    def load(ctx, pair):
        for which, blob in enumerate(pair):
            ctx.load_weights(which, blob)

    def render_all(ctx):
        out = {}
        for p in precisions:
            ctx.set_precision(p)
            out[p] = ctx.render(o, d, sc, sf, u_c, u_f)
        return out

    ctx = S.blob_context(blob_a, lx, ld, na, precision=precisions[0])
    try:
        first = render_all(ctx)
        load(ctx, blob_b)
        other = render_all(ctx)
        load(ctx, blob_a)
        last = render_all(ctx)
        for p in precisions:
            fresh = S.blob_context(blob_a, lx, ld, na, precision=p)
            try:
                want = fresh.render(o, d, sc, sf, u_c, u_f)
            finally:
                fresh.close()
            assert np.count_nonzero(other[p][0] != first[p][0]) > 0, p
            for i, (a, b, c) in enumerate(zip(last[p], first[p], want)):
                np.testing.assert_array_equal(a, b, err_msg=f"{p}, output {i}: A again vs A first")
                np.testing.assert_array_equal(a, c, err_msg=f"{p}, output {i}: A again vs a fresh context")
        assert ctx.read_nonfinite() == 0
    finally:
        ctx.close()


# ---- 6. precision="auto" on a wide network ----
def test_auto_falls_back_to_bf16x3_on_a_wide_network(oracle, golden_ckpt):
    """Lx 10 has no exact-fp32 kernel: under precision="auto" a weight set that leaves the fp16 range is re-rendered in
    bf16x3 (sticky, counted), and new weights return to f16x3."""
    import nerf_and_dietnerf_amd as N
    from integration import mi355_shim
    near, far = B.RANGE_BOUNDS
    fov, c2w = float(golden_ckpt["fov"]), golden_ckpt["c2w_test"]
    big = B.widen_blob(B.range_blob(golden_ckpt["blob_coarse"]), 10)
    fine = B.widen_blob(golden_ckpt["blob_fine"], 10)
    plain = B.widen_blob(golden_ckpt["blob_coarse"], 10)

    class _Keras:
        def __init__(self, blob):
            self.blob = blob
            self.layers = [types.SimpleNamespace(activation=types.SimpleNamespace(alpha=0.05))]

        def get_weights(self):
            return [self.blob]
    ref_model = types.SimpleNamespace(n_pos_enc_dim_xyz=10, n_pos_enc_view_dir=4, n_angles_for_model=2, near_boundary=near,
                                      far_boundary=far, n_render_samples_coarse=64, n_render_samples_fine=128,
                                      batch_size_render=4096, model_coarse=_Keras(big), model_fine=_Keras(fine))
    seeds = iter(range(100, 200))
    ctx = mi355_shim.attach(ref_model, to_tensor=lambda a: a, seed_source=lambda: next(seeds))      # precision: the default
    bf = S.blob_context((big, fine), 10, 4, 2, near=near, far=far, precision="bf16x3")
    f16x3 = S.blob_context((plain, fine), 10, 4, 2, precision="f16x3", near=near, far=far)
    try:
        assert ctx.precision == "auto" and ctx.cfg.precision == N._lib.NERF_PRECISION_F16X3
        img = ref_model.render_image(c2w, fov, 24, 24)                                                  # seed 100
        assert np.isfinite(img[0]).all() and ctx.auto_fallbacks == 1
        assert ctx.cfg.precision == N._lib.NERF_PRECISION_BF16X3
        want = bf.render_image(c2w, fov, 24, 24, 0, 64, 128, seed=100)
        for i, (a, b) in enumerate(zip(img, want)):
            S.assert_same_bits(a, b, f"auto fallback vs plain bf16x3, output {i}", finite=True)
        img2 = ref_model.render_image(c2w, fov, 24, 24)                                                 # seed 101
        S.assert_same_bits(img2[0], bf.render_image(c2w, fov, 24, 24, 0, 64, 128, seed=101)[0], "second call", finite=True)
        assert ctx.auto_fallbacks == 1 and ctx.cfg.precision == N._lib.NERF_PRECISION_BF16X3
        ref_model.model_coarse = _Keras(plain)
        ctx.refresh_weights()
        assert ctx.cfg.precision == N._lib.NERF_PRECISION_F16X3
        img3 = ref_model.render_image(c2w, fov, 24, 24)                                                 # seed 102
        assert ctx.cfg.precision == N._lib.NERF_PRECISION_F16X3 and ctx.auto_fallbacks == 1
        S.assert_same_bits(img3[0], f16x3.render_image(c2w, fov, 24, 24, 0, 64, 128, seed=102)[0], "ordinary weights stay on f16x3",
                           finite=True)
    finally:
        for c in (ctx, bf, f16x3):
            c.close()


# ---- 7. reference frames ----
def test_bf16x3_matches_reference_frames(golden_ckpt, frames, scene, capsys):  # noqa: F811
    """The stored frames of the reference's three camera tours (the first ten of each and every other one: all 234) in
    bf16x3 under the clauses tests/test_video_pins.py applies to f16x3."""
    import nerf_and_dietnerf_amd as N
    model = N.NeRF(NET, {"n_render_samples_coarse": 64, "n_render_samples_fine": 128}, scene["near"], scene["far"],
                   device=0, precision="bf16x3")
    model.set_weights(golden_ckpt["blob_coarse"], golden_ckpt["blob_fine"])
    try:
        for tour, mats in tours(frames, scene).items():
            idx = frames[tour + "_index"]
            assert len(idx) >= 10
            ref = frames[tour + "_rgb"].astype(np.float32) / 255
            refd = frames[tour + "_depth"].astype(np.float32) / 255
            a, ad = N.render_video(model, mats[idx], scene["fov"], 50, 50, seed=0, equalize_depth=True)
            b, bd = N.render_video(model, mats[idx], scene["fov"], 50, 50, seed=100000, equalize_depth=True)
            a, b = np.clip(a, 0, 1), np.clip(b, 0, 1)
            p = np.array([psnr(a[k], ref[k]) for k in range(len(idx))])
            p_self = np.array([psnr(a[k], b[k]) for k in range(len(idx))])
            d = np.array([psnr(ad[k], refd[k]) for k in range(len(idx))])
            d_self = np.array([psnr(ad[k], bd[k]) for k in range(len(idx))])
            with capsys.disabled():
                print(f"\n[bf16x3 {tour}] rgb min {p.min():.2f} mean {p.mean():.2f} dB; depth min {d.min():.2f} mean "
                      f"{d.mean():.2f} dB", end="")
            assert np.all(p >= np.minimum(RGB_BAR, p_self - RGB_SELF_MARGIN)), (tour, p.min())
            assert np.all(d >= np.minimum(DEPTH_BAR, d_self - DEPTH_SELF_MARGIN)), (tour, d.min())
            assert p.mean() >= RGB_MEAN_BAR[tour] and d.mean() >= DEPTH_MEAN_BAR[tour], (tour, p.mean(), d.mean())
            if tour != "sphere":
                assert p.min() >= RGB_BAR, (tour, p.min())
        assert model.ctx.read_nonfinite() == 0
    finally:
        model.ctx.close()


# ---- 8. rate ----
def test_rate_against_f16x3(golden_ckpt, capsys):
    """MLP-kernel time of 256 x 256, 64 + 128, rgb-only frames (nerf_ctx_enable_timing; 5 warm-up, 20 timed, median), f16x3
    and bf16x3 alternately in one process.  A sanity floor only: bf16x3 at no less than half the f16x3 rate (same MFMA
    count and rate, one conversion less per pair).  The measured ratio is recorded in DESIGN.md section 4.1."""
    c2w, fov = golden_ckpt["c2w_test"], float(golden_ckpt["fov"])
    near, far = float(golden_ckpt["near"]), float(golden_ckpt["far"])
    ctxs = {p: S.blob_context((golden_ckpt["blob_coarse"], golden_ckpt["blob_fine"]), precision=p, near=near, far=far)
            for p in ("f16x3", "bf16x3")}
    try:
        ms = {p: [] for p in ctxs}
        rows = 0
        for it in range(25):
            for p, ctx in ctxs.items():
                ctx.enable_timing(True)
                ctx.render_image(c2w, fov, 256, 256, 0, 64, 128, seed=it, rgb_only=True, device_out=True)
                t, _, rows = ctx.read_timing()
                ctx.enable_timing(False)
                if it >= 5:
                    ms[p].append(t)
        med = {p: float(np.median(v)) for p, v in ms.items()}
        rate = {p: 256 * 256 / med[p] / 1e3 for p in med}            # M rays/s of MLP-kernel time
        ratio = rate["bf16x3"] / rate["f16x3"]
        with capsys.disabled():
            print(f"\n[rate, 256 x 256, 64 + 128, rgb only, {rows} MLP rows per frame] f16x3 {med['f16x3']:.3f} ms "
                  f"({rate['f16x3']:.3f} M rays/s), bf16x3 {med['bf16x3']:.3f} ms ({rate['bf16x3']:.3f} M rays/s): "
                  f"bf16x3 / f16x3 = {ratio:.3f}", end="")
        assert all(c.read_nonfinite() == 0 for c in ctxs.values())
        assert ratio >= 0.5, ratio
    finally:
        for c in ctxs.values():
            c.close()
