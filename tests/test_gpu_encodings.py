"""Networks with other positional-encoding octave counts than the default (n_pos_enc_dim_xyz 1..10, n_pos_enc_view_dir 1..4;
src/NeRF.py:249-339 builds the layers from these keys): render, model_predict, the training gradients under both policies,
the backward through render(), fit / checkpoint, all against the oracles at the bars the default geometry is held to.

Lx <= 5 runs on the default geometry's kernels, Lx 6..10 on their wide-PE build (10 octaves, 4 PE k-steps; fp16-core modes
only): the octaves a network does not have are still encoded on the device, but their weight rows are packed as zeros (the
way the n_angles = 1 network's y slots are), so the products are exact zeros --
`test_fewer_octaves_equal_the_default_network_with_zero_rows` pins that bit for bit."""
import numpy as np
import pytest

import grad_blocks as GB
import support as S

pytestmark = pytest.mark.gpu


RGB_TOL = {"fp32": 1e-4, "f16x3": 1e-4, "f16": 3e-2}          # the bars of the (5, 4) render tests
RAW_TOL = {"fp32": 5e-5, "f16x3": 5e-5, "f16": 5e-2}          # model_predict, relative to max(1, |ref|)

# (Lx, Ld, n_angles); Ld is unused by the xyz-only network (n_angles 0)
GEOMETRIES = [(5, 2, 2), (3, 4, 2), (1, 1, 2), (4, 3, 1), (2, 2, 1), (4, 4, 0), (1, 4, 0)]
WIDE_GEOMETRIES = [(10, 4, 2), (6, 4, 2), (7, 3, 1), (10, 4, 0), (8, 2, 2)]      # the wide-PE kernels


def _prec(lx, precision="fp32"):
    """The exact-fp32 mode exists for Lx <= 5; the wide-PE networks' fp32-class mode is f16x3."""
    return precision if lx <= 5 or precision != "fp32" else "f16x3"


def _blobs(lx, ld, na, seed=3):
    import nerf_and_dietnerf_amd as N
    bc, bf = N.glorot_blob(seed, **S.kw(lx, ld, na)), N.glorot_blob(seed + 1, **S.kw(lx, ld, na))
    bc[-1] = bf[-1] = 1.5                   # lift sigma: Glorot networks are almost transparent
    return bc, bf


def _spread(blob, lx, ld, na, L=5):
    """The (L, 4) blob (L = 5, or 10 for the wide-PE layout) of the same network: zero rows for the octaves it does not have (Python restatement of the
    library's layout, written from the reference's encodings: [x, sin_k, cos_k, ...] per xyz component, [sin_k, cos_k, ...]
    per direction component)."""
    from oracle import nerf_oracle as O
    small = O.unpack_blob(blob, **S.kw(lx, ld, na))
    wide = O.unpack_blob(np.zeros(O.blob_size(**S.kw(L, 4, na)), np.float32), **S.kw(L, 4, na))
    XC = 1 + 2 * L

    def xyz_rows():
        out = []
        for c in range(3):
            out.append((c * (1 + 2 * lx), c * XC))
            for k in range(lx):
                for h in range(2):
                    out.append((c * (1 + 2 * lx) + 1 + 2 * k + h, c * XC + 1 + 2 * k + h))
        return out

    def dir_rows(ncomp):
        return [(c * 2 * ld + 2 * k + h, c * 8 + 2 * k + h) for c in range(ncomp) for k in range(ld) for h in range(2)]

    parts = []
    for l, ((ks, bs), (kw_, bw)) in enumerate(zip(small, wide)):
        kw_ = kw_.copy()
        if l == 0:
            for s, w in xyz_rows():
                kw_[w] = ks[s]
        elif l == 4:
            for s, w in xyz_rows():
                kw_[w] = ks[s]
            kw_[3 * XC:] = ks[3 + 6 * lx:]
        elif na != 0 and l in (8, 10):
            kw_[:256] = ks[:256]
            for s, w in dir_rows(na + 1):
                kw_[256 + w] = ks[256 + s]
        else:
            kw_ = ks
        parts += [kw_.ravel(), bs]
    return np.concatenate(parts).astype(np.float32)


def _rays(oracle, n, seed):
    rng = np.random.default_rng(seed)
    o = np.concatenate([rng.uniform(-0.3, 0.3, (n, 3)), np.ones((n, 1))], 1).astype(np.float32)
    d = np.concatenate([rng.uniform(-1, 1, (n, 3)), np.zeros((n, 1))], 1).astype(np.float32)
    return o, d, rng


@pytest.mark.parametrize("precision", ["fp32", "f16x3", "f16"])
@pytest.mark.parametrize("lx,ld,na", GEOMETRIES + WIDE_GEOMETRIES)
def test_render_and_model_predict(oracle, lx, ld, na, precision):
    """render (explicit draws, 64 + 128), render_image (Philox draws, 32 x 32) and model_predict (incl. |x| up to 40)
    against the oracle with the network's own encodings."""
    import nerf_and_dietnerf_amd as N
    near, far = 0.6, 2.4
    kw = S.kw(lx, ld, na)
    if lx > 5 and precision == "fp32":
        # no exact-fp32 kernel for the wide-PE networks: refused loudly, at creation and when switched to
        with pytest.raises(RuntimeError, match="not fp32"):
            N.Context(near=near, far=far, precision="fp32", **kw)
        ctx = N.Context(near=near, far=far, precision="f16x3", **kw)
        with pytest.raises(RuntimeError, match="not fp32"):
            ctx.set_precision("fp32")
        ctx.close()
        return
    ctx = N.Context(near=near, far=far, precision=precision, **kw)
    bc, bf = _blobs(lx, ld, na)
    assert ctx.blob_size() == bc.size == N.blob_size(**kw)
    ctx.load_weights(0, bc)
    ctx.load_weights(1, bf)
    coarse, fine = oracle.unpack_blob(bc, **kw), oracle.unpack_blob(bf, **kw)
    o, d, rng = _rays(oracle, 64, 2 + lx + 7 * ld + 31 * na)
    uc, uf = rng.random((64, 64), dtype=np.float32), rng.random((64, 128), dtype=np.float32)
    got = ctx.render(o, d, 64, 128, uc, uf)
    ref = oracle.render(coarse, fine, o, d, near, far, uc, uf, **kw)
    assert np.isfinite(got[0]).all()
    assert np.abs(got[0] - ref[0]).max() <= RGB_TOL[precision]
    c2w = oracle.get_sphere_matrix(1.0, -25.0, 40.0, 0.0).astype(np.float32)
    img = ctx.render_image(c2w, 0.6, 32, 32, 4096, 64, 128, seed=7)
    ref_img = oracle.render_image(coarse, fine, c2w, 0.6, 32, 32, near, far, 64, 128, seed=7, **kw)
    assert np.abs(img[0] - ref_img[0]).max() <= RGB_TOL[precision]
    pts = np.concatenate([rng.uniform(-1, 1, (300, 3)), rng.uniform(-40, 40, (100, 3))]).astype(np.float32)
    views = None if na == 0 else rng.uniform(-1, 1, (400, na + 1)).astype(np.float32)
    for which, layers in ((0, coarse), (1, fine)):
        raw = ctx.model_predict(which, pts, views)
        rref = oracle.model_predict(layers, pts, views, lx, ld)
        assert np.abs(raw - rref).max() <= RAW_TOL[precision] * max(1.0, np.abs(rref).max())
    assert ctx.read_nonfinite() == 0
    ctx.close()


@pytest.mark.parametrize("lx,ld,na", [(3, 2, 2), (1, 3, 1), (2, 4, 0), (7, 3, 1), (6, 2, 2), (9, 4, 0)])
def test_fewer_octaves_equal_the_default_network_with_zero_rows(oracle, lx, ld, na):
    """An (Lx, Ld) network renders BIT-IDENTICALLY to the (L, 4) network whose extra octave rows are zero (L = 5, or 10 for
    Lx 6..9: the wide-PE kernels), in every precision: the same kernels, the same operand streams."""
    import nerf_and_dietnerf_amd as N
    near, far = 0.6, 2.4
    L = 5 if lx <= 5 else 10
    bc, bf = _blobs(lx, ld, na, seed=11)
    wc, wf = _spread(bc, lx, ld, na, L), _spread(bf, lx, ld, na, L)
    small = N.Context(near=near, far=far, precision=_prec(lx), **S.kw(lx, ld, na))
    wide = N.Context(near=near, far=far, precision=_prec(L), **S.kw(L, 4, na))
    small.load_weights(0, bc); small.load_weights(1, bf)
    wide.load_weights(0, wc); wide.load_weights(1, wf)
    # the spread is the right network (the oracle with (5, 4) encodings on it agrees with the (Lx, Ld) oracle)
    o, d, rng = _rays(oracle, 48, 5)
    uc, uf = rng.random((48, 32), dtype=np.float32), rng.random((48, 64), dtype=np.float32)
    r_small = oracle.render(oracle.unpack_blob(bc, **S.kw(lx, ld, na)), oracle.unpack_blob(bf, **S.kw(lx, ld, na)), o, d,
                            near, far, uc, uf, **S.kw(lx, ld, na))
    r_wide = oracle.render(oracle.unpack_blob(wc, **S.kw(L, 4, na)), oracle.unpack_blob(wf, **S.kw(L, 4, na)), o, d, near,
                           far, uc, uf, **S.kw(L, 4, na))
    assert np.abs(r_small[0] - r_wide[0]).max() <= 1e-6
    for precision in ("fp32", "f16x3", "f16") if L == 5 else ("f16x3", "f16"):
        small.set_precision(precision)
        wide.set_precision(precision)
        a = small.render(o, d, 32, 64, uc, uf)
        b = wide.render(o, d, 32, 64, uc, uf)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
    small.close()
    wide.close()


def _train_problem(oracle, n=48, sc=16, sf=24, seed=0):
    """The rays and draws of S.golden_problem (n <= 64) for this file's Glorot networks, on the bounds 0.5 .. 2.5."""
    o, d, rng = S.oracle_rays(oracle, n, seed)
    return dict(o=o, d=d, u_c=rng.random((n, sc), dtype=np.float32), u_f=rng.random((n, sf), dtype=np.float32),
                tgt=rng.random((n, 3), dtype=np.float32), sc=sc, sf=sf, near=0.5, far=2.5)


@pytest.mark.parametrize("lx,ld,na", [(5, 2, 2), (2, 3, 1), (3, 4, 0), (10, 4, 2), (10, 4, 0), (6, 3, 1)])
def test_training_gradients_float32_policy(oracle, lx, ld, na, capsys):
    """train_gradients (loss, both networks, the sampler term) against float64 autograd with the network's encodings:
    the bars of test_gpu_train.py::test_gradients_coarse_and_fine (alpha 1: 2e-4 of max|g|; alpha 0.05: 5e-2, cosine
    0.999); after one optimizer step the trained weights (re-packed on the device for the render path) read back at the
    network's own size and render bit-identically to a fresh context loaded with them."""
    from oracle import train_oracle as T
    import nerf_and_dietnerf_amd as N
    p = _train_problem(oracle, seed=lx + 10 * ld)
    kw = S.kw(lx, ld, na)
    bc, bf = _blobs(lx, ld, na, seed=21)
    for alpha in (1.0, 0.05):
        ctx = N.Context(near=p["near"], far=p["far"], leaky_relu_alpha=alpha, precision=_prec(lx), **kw)
        ctx.load_weights(0, bc); ctx.load_weights(1, bf)
        ctx.train_begin(5e-4, sampler_gradient=True)
        m, gc, gf = ctx.train_gradients(p["o"], p["d"], p["tgt"], p["sc"], p["sf"], p["u_c"], p["u_f"])
        r = T.train_gradients(bc, bf, p["o"], p["d"], p["tgt"], p["near"], p["far"], p["u_c"], p["u_f"],
                              sampler_grad=True, alpha=alpha, **kw)
        ec, ef = S.relerr(gc, r["grad_coarse"]), S.relerr(gf, r["grad_fine"])
        with capsys.disabled():
            print(f"\n[({lx},{ld},{na}) float32 policy, alpha {alpha}] vs float64 autograd: coarse {ec:.2e}, "
                  f"fine {ef:.2e} of max|g|", end="")
        # Lx >= 6: the top octave multiplies the fp32 sample position by 2^9 pi, so its one-ulp rounding (float64 in the oracle)
        # moves the angle by ~1e-4 rad -- the layer-wise exact-fp32 trainer, which shares no kernel with the wide-PE path,
        # shows the same 2e-3 of max|g| (test_layerwise_exact_fp32_trainer): that is the arithmetic class, not a kernel error
        wide = lx > 5
        assert abs(m["loss"] - r["loss"]) <= (1e-5 if wide else 2e-6) * r["loss"]
        assert np.isfinite(gc).all() and np.isfinite(gf).all()
        tol, cos_min = ((5e-3 if wide else 2e-4), (0.9999 if wide else 0.9999999)) if alpha == 1.0 else (5e-2, 0.999)
        assert ec <= tol and S.cos(gc, r["grad_coarse"]) > cos_min
        assert ef <= tol and S.cos(gf, r["grad_fine"]) > cos_min
        # block by block.  alpha 1: 2e-4 of each block's own max where float32 autograd resolves the block.  At Lx >= 6 the top
        # octave's fp32 angle rounding (below) keeps most blocks at the blob-relative bar by that rule; one block it does not
        # catch is named: (10,4,0) fine b11, 2.4e-4 of its own max.  b11 is the plain sum over all rows of d(loss)/d(sigma):
        # a 1e-4 rad error of the top-octave angle moves neighbouring samples' sigma the same way, which a sum over rows does
        # not average out, and the oracle's float32 run need not round 2^9 pi x where the device does, so its own 7e-5 there
        # does not bound the device's figure.
        # alpha 0.05, the fine network by relative L2: float32 autograd has no mask flip on these problems (4e-6..9e-6), the
        # device forward has one at (5,2,2) (layer 4: k0 4.3e-4 .. b4 2.6e-4, all twelve blocks of layers 0..4 and no other)
        # (see "One LeakyReLU mask flip" in tests/test_gpu_train.py): the blocks of layers 0..4 keep the blob-wide bar there,
        # every block above is asserted.  (3,4,0): k0 8.0e-5, b0 7.7e-5, under the bar's floor of 2e-4.
        r32 = S.f32(T.train_gradients, bc, bf, p["o"], p["d"], p["tgt"], p["near"], p["far"], p["u_c"], p["u_f"],
                   sampler_grad=True, alpha=alpha, **kw)
        blks = GB.blocks(lx, ld, na)
        with capsys.disabled():
            tag = f"[({lx},{ld},{na}) float32 policy, alpha {alpha:g}]"
            if alpha == 1.0:
                GB.check_fp32_smooth(gc, r["grad_coarse"], r32["grad_coarse"], blks, tol, tag + " coarse")
                GB.check_fp32_smooth(gf, r["grad_fine"], r32["grad_fine"], blks, tol, tag + " fine",
                                     named=("b11",) if (lx, ld, na) == (10, 4, 0) else ())
            else:
                flip = {(5, 2, 2): 4}.get((lx, ld, na))
                GB.check_fp32_masks(gf, r["grad_fine"], r32["grad_fine"], blks, tag + " fine",
                                    named=() if flip is None else GB.layers_up_to(blks, flip))
        if alpha == 1.0:
            # one optimizer step, then the trained weights read back and render like a fresh context loaded with them
            ctx.train_step(p["o"], p["d"], p["tgt"], p["sc"], p["sf"], p["u_c"], p["u_f"])
            wc, wf = ctx.get_weights(0), ctx.get_weights(1)
            assert wc.size == bc.size and not np.array_equal(wc, bc)
            out = ctx.render(p["o"], p["d"], p["sc"], p["sf"], p["u_c"], p["u_f"])
            fresh = N.Context(near=p["near"], far=p["far"], leaky_relu_alpha=alpha, precision=_prec(lx), **kw)
            fresh.load_weights(0, wc); fresh.load_weights(1, wf)
            ref = fresh.render(p["o"], p["d"], p["sc"], p["sf"], p["u_c"], p["u_f"])
            np.testing.assert_array_equal(out[0], ref[0])
            fresh.close()
        ctx.close()


@pytest.mark.parametrize("lx,ld,na", [(3, 2, 2), (2, 4, 0), (10, 2, 2)])
def test_layerwise_exact_fp32_trainer(oracle, lx, ld, na, monkeypatch, capsys):
    """The layer-wise exact-fp32 reference trainer behind NERF_TRAIN_FORWARD=gemm (GEMMs over the encoded inputs in the
    network's own column layout, the encoding backward on the compact layout) at alpha 1 with the sampler term: 2e-4 of
    max|g| against float64 autograd."""
    from oracle import train_oracle as T
    import nerf_and_dietnerf_amd as N
    monkeypatch.setenv("NERF_TRAIN_FORWARD", "gemm")
    p = _train_problem(oracle, seed=7)
    kw = S.kw(lx, ld, na)
    bc, bf = _blobs(lx, ld, na, seed=27)
    ctx = N.Context(near=p["near"], far=p["far"], leaky_relu_alpha=1.0, precision=_prec(lx), **kw)
    ctx.load_weights(0, bc); ctx.load_weights(1, bf)
    ctx.train_begin(5e-4, sampler_gradient=True)
    m, gc, gf = ctx.train_gradients(p["o"], p["d"], p["tgt"], p["sc"], p["sf"], p["u_c"], p["u_f"])
    r = T.train_gradients(bc, bf, p["o"], p["d"], p["tgt"], p["near"], p["far"], p["u_c"], p["u_f"], sampler_grad=True,
                          alpha=1.0, **kw)
    tol = 5e-3 if lx > 5 else 2e-4          # Lx >= 6: the fp32 angle rounding of the top octave (see the float32-policy test)
    assert abs(m["loss"] - r["loss"]) <= (1e-5 if lx > 5 else 2e-6) * r["loss"]
    assert S.relerr(gc, r["grad_coarse"]) <= tol and S.relerr(gf, r["grad_fine"]) <= tol
    r32 = S.f32(T.train_gradients, bc, bf, p["o"], p["d"], p["tgt"], p["near"], p["far"], p["u_c"], p["u_f"], sampler_grad=True,
               alpha=1.0, **kw)
    with capsys.disabled():
        GB.check_fp32_smooth(gc, r["grad_coarse"], r32["grad_coarse"], GB.blocks(lx, ld, na), tol, f"[({lx},{ld},{na}) layer-wise] coarse")
        GB.check_fp32_smooth(gf, r["grad_fine"], r32["grad_fine"], GB.blocks(lx, ld, na), tol, f"[({lx},{ld},{na}) layer-wise] fine")
    ctx.close()


@pytest.mark.parametrize("lx,ld,na", [(5, 2, 2), (2, 3, 1), (3, 4, 0), (10, 4, 2), (10, 4, 0), (6, 3, 1)])
def test_training_gradients_mixed_float16_policy(oracle, lx, ld, na, capsys):
    """mixed_float16 against the autograd oracle that rounds where the kernels round, with the network's encodings, at
    the bars test_gpu_train.py holds Glorot networks of the other n_angles variants to (coarse 3e-2, fine 5e-3 of
    max|g|, alpha 1, sampler term on)."""
    from oracle import train_oracle as T
    import nerf_and_dietnerf_amd as N
    p = _train_problem(oracle, seed=3 + lx + 10 * ld)
    kw = S.kw(lx, ld, na)
    bc, bf = _blobs(lx, ld, na, seed=25)
    ctx = N.Context(near=p["near"], far=p["far"], leaky_relu_alpha=1.0, precision=_prec(lx), **kw)
    ctx.load_weights(0, bc); ctx.load_weights(1, bf)
    # Lx >= 6: the sampler term's 1e5 gain (its 1e-5 clamp) acts on top-octave angles that fp16 and the emulation round
    # differently by up to 2^9 pi ulps of the position; checked without it there (the fine network, which it does not touch,
    # is checked either way)
    wide = lx > 5
    ctx.train_begin(5e-4, mixed_float16=True, sampler_gradient=not wide)
    m, gc, gf = ctx.train_gradients(p["o"], p["d"], p["tgt"], p["sc"], p["sf"], p["u_c"], p["u_f"])
    r16 = T.train_gradients(bc, bf, p["o"], p["d"], p["tgt"], p["near"], p["far"], p["u_c"], p["u_f"],
                            sampler_grad=not wide, alpha=1.0, fp16_loss_scale=32768.0, **kw)
    qc, qf = S.relerr(gc, r16["grad_coarse"]), S.relerr(gf, r16["grad_fine"])
    with capsys.disabled():
        print(f"\n[({lx},{ld},{na}) mixed_float16] vs the fp16-emulating oracle: coarse {qc:.2e}, fine {qf:.2e} of max|g|",
              end="")
    assert np.isfinite(gc).all() and np.isfinite(gf).all()
    assert abs(m["loss"] - r16["loss"]) <= (1e-3 if wide else 2e-5) * r16["loss"]
    assert qc <= 3e-2 and qf <= (2e-2 if wide else 5e-3)
    e32 = S.f32(T.train_gradients, bc, bf, p["o"], p["d"], p["tgt"], p["near"], p["far"], p["u_c"], p["u_f"],
               sampler_grad=not wide, alpha=1.0, fp16_loss_scale=32768.0, **kw)
    with capsys.disabled():
        GB.check_mixed(gc, r16["grad_coarse"], e32["grad_coarse"], GB.blocks(lx, ld, na), f"[({lx},{ld},{na}) mixed_float16] coarse")
        GB.check_mixed(gf, r16["grad_fine"], e32["grad_fine"], GB.blocks(lx, ld, na), f"[({lx},{ld},{na}) mixed_float16] fine")
    ctx.close()


@pytest.mark.parametrize("policy", ["float32", "mixed_float16"])
def test_backward_through_render(oracle, policy, capsys):
    """train_render_gradients (DietNeRF's backward through render(), 55 + 55 samples, sampler term) at (Lx 5, Ld 2, the
    shipped 100px_robot config's direction octaves) and (Lx 2, Ld 1): float32 policy vs float64 autograd at 2e-4 of
    max|g| (test_backward_through_render), mixed_float16 vs the fp16-emulating oracle at coarse 3e-2 / fine 5e-3
    (test_backward_through_render_mixed_policy)."""
    from oracle import train_oracle as T
    import nerf_and_dietnerf_amd as N
    mixed = policy == "mixed_float16"
    for lx, ld in ((5, 2), (2, 1), (10, 4), (7, 2)):
        kw = S.kw(lx, ld, 2)
        p = _train_problem(oracle, n=40, sc=55, sf=55, seed=9)
        rng = np.random.default_rng(3)
        d_rgb = (rng.standard_normal((40, 3)) * 0.1).astype(np.float32)
        bc, bf = _blobs(lx, ld, 2, seed=41)
        ctx = N.Context(near=p["near"], far=p["far"], leaky_relu_alpha=1.0, precision=_prec(lx), **kw)
        ctx.load_weights(0, bc); ctx.load_weights(1, bf)
        sg = not (mixed and lx > 5)
        ctx.train_begin(5e-4, mixed_float16=mixed, sampler_gradient=sg)
        rgb, gc, gf = ctx.train_render_gradients(p["o"], p["d"], d_rgb, p["sc"], p["sf"], p["u_c"], p["u_f"])
        r = T.render_gradients(bc, bf, p["o"], p["d"], d_rgb, p["near"], p["far"], p["u_c"], p["u_f"], alpha=1.0, sampler_grad=sg,
                               fp16_loss_scale=32768.0 if mixed else None, **kw)
        ec, ef = S.relerr(gc, r["grad_coarse"]), S.relerr(gf, r["grad_fine"])
        with capsys.disabled():
            print(f"\n[({lx},{ld},2) backward through render(), {policy}] coarse {ec:.2e}, fine {ef:.2e} of max|g|", end="")
        assert np.isfinite(gc).all() and np.isfinite(gf).all()
        wide = lx > 5     # the top octave's angle rounding (see the training-gradient tests): wider bars, sampler term off
        if mixed:
            assert np.abs(rgb - r["rgb"]).max() <= 2e-3
            assert (not gc.any()) if wide else ec <= 3e-2
            assert ef <= (2e-2 if wide else 5e-3)
        else:
            assert np.abs(rgb - r["rgb"]).max() <= 5e-5
            assert ec <= (5e-3 if wide else 2e-4) and ef <= (5e-3 if wide else 2e-4)
        ctx.close()


@pytest.mark.parametrize("policy", ["float32", "mixed_float16"])
def test_fit_and_checkpoint(tmp_path, policy, capsys):
    """NeRF from a net_config with n_pos_enc_dim_xyz 10 (the original paper's setting; the wide-PE kernels) and with
    n_pos_enc_dim_xyz 3 / n_pos_enc_view_dir 2, on the shipped alexander50 views: fit's loss falls over three epochs, the
    test-view PSNR is within 1.5 dB of that of the default (5, 4) network trained the same way in the same test, and a saved
    checkpoint reloads into a fresh NeRF that renders bit-identically.  The 1.5 dB bar was set before the first run, not
    derived from the reference; (3, 2) first measured 21.21 vs 21.58 dB (float32) and 21.20 vs 22.02 dB (mixed_float16)."""
    import os
    import torch
    import nerf_and_dietnerf_amd as N
    root = os.path.join(os.path.dirname(__file__), "golden")
    images, poses, fov, near, far, _, _ = N.get_data_from_colmap(os.path.join(root, "alexander50"))
    idx_test = 19
    train_idx = N.get_train_images_indices(len(images), idx_test)
    target = torch.as_tensor(images[idx_test], device="cuda")
    ren = {"n_render_samples_coarse": 64, "n_render_samples_fine": 128}
    mixed = policy == "mixed_float16"
    psnr, losses = {}, {}
    for lx, ld in ((5, 4), (3, 2), (10, 4)):
        net_cfg = {"hidden_layer_dim": 256, "last_hidden_layer_dim": 128, "leaky_relu_alpha": 0.05,
                   "n_pos_enc_dim_xyz": lx, "n_pos_enc_view_dir": ld, "n_angles_for_model": 2,
                   "n_rays_in_batch_train": 4096, "n_rays_in_batch_render": 4096}
        kw = S.kw(lx, ld, 2)
        model = N.NeRF(net_cfg, ren, near, far)
        model.set_weights(N.glorot_blob(0, **kw), N.glorot_blob(1, **kw))
        model.compile(4.0e-4, mixed_float16=mixed)
        ds = N.prepare_ds(4096, poses[train_idx], images[train_idx], fov, model.ctx, seed=0)
        hist = N.fit(model, ds, epochs=3)
        losses[lx] = [h["loss"] for h in hist]
        rgb = model.render_image(poses[idx_test], fov, 50, 50, seed=1000, device_out=True, rgb_only=True)[0]
        psnr[lx] = float(-10 * torch.log10(torch.mean((rgb - target) ** 2)))
        if lx != 5:
            path = tmp_path / "NeRF_model_epoch_003.h5"
            model.save_weights(path)
            again = N.NeRF(net_cfg, ren, near, far)
            again.load_weights(path)
            for m in (model, again):
                m.ctx.set_precision(_prec(lx))
            a = model.render_image(poses[idx_test], fov, 24, 24, seed=5)
            b = again.render_image(poses[idx_test], fov, 24, 24, seed=5)
            np.testing.assert_array_equal(a[0], b[0])
            again.ctx.close()
        model.ctx.close()
    with capsys.disabled():
        for lx in (3, 10):
            print(f"\n[fit, {policy}, 3 epochs] loss (Lx {lx}) " + " ".join(f"{x:.4f}" for x in losses[lx]) +
                  f"; test-view PSNR {psnr[lx]:.2f} dB vs {psnr[5]:.2f} dB for (5, 4)", end="")
    for lx in (3, 10):
        assert losses[lx][-1] < losses[lx][0]
        assert abs(psnr[lx] - psnr[5]) <= 1.5


def test_get_nerf_with_fewer_direction_octaves(tmp_path):
    """config.get_nerf (ExecutionRun.get_nerf) from a reference YAML with n_pos_enc_view_dir 2 (what the shipped
    100px_robot_36pics_sphere.yaml asks for) and nothing saved: Glorot weights of the config's own layer shapes, one epoch
    on four views trains, and the trained weights go to a checkpoint of those shapes."""
    import os
    import nerf_and_dietnerf_amd as N
    from nerf_and_dietnerf_amd import config as C, keras_h5
    from oracle import nerf_oracle as O
    here = os.path.dirname(os.path.abspath(__file__))
    cfg = C.load_config(os.path.join(here, "golden", "configs", "50px_alexander_71pics_sphere_nerf.yaml"))
    cfg[C.DATASET_LOCATION] = "alexander50"
    cfg[C.NEURAL_NET]["n_pos_enc_view_dir"] = 2
    images, poses, fov, near, far, _, _ = C.get_data(cfg, os.path.join(here, "golden"))
    model = C.get_nerf(cfg, near, far, save_location=None)
    kw = S.kw(cfg[C.NEURAL_NET]["n_pos_enc_dim_xyz"], 2, cfg[C.NEURAL_NET]["n_angles_for_model"])
    assert model.ctx.blob_size() == N.blob_size(**kw)
    _, tr_img, tr_pose = C.get_train_data(cfg, images, poses)
    ds = N.prepare_ds(cfg[C.NEURAL_NET][C.N_RAYS_IN_BATCH_TRAIN], tr_pose[:4], tr_img[:4], fov, model.ctx)
    hist = N.fit(model, ds, epochs=1)
    assert np.isfinite(hist[0]["loss"])
    path = str(tmp_path / "NeRF_model_epoch_001.h5")
    model.save_weights(path)
    shapes = [t.shape for t in next(iter(keras_h5.read_keras_weights(path).values()))[0::2]]
    assert shapes == [tuple(s) for s in O.layer_shapes(**kw)]
    model.ctx.close()
