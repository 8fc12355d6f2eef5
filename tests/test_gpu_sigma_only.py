"""The sigma-only coarse pass of the f16x3 mode (mlp_f16x3_sig_kernel + the weights-only composite, csrc/nerf_api.hip,
dev_render_rays): a coarse render_rays call that asks for the weights alone -- the coarse pass of NeRF.render -- must
return the very bits of the full kernel's weights output.

Both paths are reached through nerf_render_rays on one context: outputs {weights} take the sigma-only path, outputs
{weights, rgb} the full network.  Row counts cover one row, ragged tiles, and 2 x CUs x 128 + 77 rows (every workgroup
of the persistent grid loops at least twice: the weight stream wraps).  The trainer's path re-packs the sigma-only
stream on the device from its own gather table (train_api.hip, train_flush_weights); a render between train_steps must
match a context freshly loaded with the trained weights bit for bit."""
import numpy as np
import pytest

import f16_variants as V
import support as S

pytestmark = pytest.mark.gpu

NEAR, FAR = 0.6, 2.4
WEIGHTS_ONLY, WITH_RGB = ("weights",), ("weights", "rgb")      # outputs {weights}: the sigma-only path; with rgb: the full network


def _shapes():
    return [(1, 1), (1, 64), (37, 64), (129, 3), (2 * S.n_cus() * 128 + 77, 1), (2 * S.n_cus() * 2 + 1, 64)]


def _check_all_shapes(ctx, label):
    for n, s in _shapes():
        o, d, z = S.rays_towards_origin(n, s, NEAR, FAR)
        full = S.render_rays(ctx, 0, o, d, z, WITH_RGB)[0]
        sig = S.render_rays(ctx, 0, o, d, z, WEIGHTS_ONLY)[0]
        S.assert_same_bits(sig, full, f"{label} N={n} S={s}", finite=True)
        if s > 1 and n > 1:
            assert full.max() > 1e-3, (label, n, s)      # the weights are not trivially zero


@pytest.mark.parametrize("lx,ld,na", [(5, 4, 2), (5, 4, 1), (3, 2, 2)])
def test_weights_only_coarse_pass_is_bit_identical(lx, ld, na):
    ctx = S.blob_context(V.blobs(lx, ld, na), lx, ld, na)
    try:
        _check_all_shapes(ctx, f"({lx},{ld},{na})")
        assert ctx.read_nonfinite() == 0
    finally:
        ctx.close()


def test_weights_only_coarse_pass_glorot_weights():
    import nerf_and_dietnerf_amd as N
    ctx = S.blob_context((N.glorot_blob(0), N.glorot_blob(1)))
    try:
        for n, s in _shapes():
            o, d, z = S.rays_towards_origin(n, s, NEAR, FAR)
            S.assert_same_bits(S.render_rays(ctx, 0, o, d, z, WEIGHTS_ONLY)[0], S.render_rays(ctx, 0, o, d, z, WITH_RGB)[0],
                               f"glorot N={n} S={s}", finite=True)
    finally:
        ctx.close()


def test_weights_only_coarse_pass_shipped_checkpoint(golden_ckpt):
    ctx = S.blob_context((golden_ckpt["blob_coarse"], golden_ckpt["blob_fine"]))
    try:
        _check_all_shapes(ctx, "shipped checkpoint")
    finally:
        ctx.close()


def test_render_between_train_steps_matches_fresh_network():
    """The trained network's sigma-only stream comes from the trainer's gather table: its coarse weights and the whole
    render must equal those of a context loaded from the trained blobs."""
    rng = np.random.default_rng(7)
    n, sc, sf = 512, 64, 128
    o, d, _ = S.rays_towards_origin(n, 1, NEAR, FAR, seed=9)
    tgt = rng.random((n, 3), dtype=np.float32)
    u_c, u_f = rng.random((n, sc), dtype=np.float32), rng.random((n, sf), dtype=np.float32)
    trained = S.blob_context(V.blobs(5, 4, 2))
    fresh = None
    try:
        trained.train_begin(5e-4)
        for _ in range(2):
            trained.train_step(o, d, tgt, sc, sf, u_c, u_f)
        _, _, z = S.rays_towards_origin(n, sc, NEAR, FAR, seed=10)
        w_tr = S.render_rays(trained, 0, o, d, z, WEIGHTS_ONLY)[0]
        S.assert_same_bits(w_tr, S.render_rays(trained, 0, o, d, z, WITH_RGB)[0], "trained: sigma-only vs full", finite=True)
        r_tr = trained.render(o, d, sc, sf, u_c, u_f)
        fresh = S.blob_context((trained.get_weights(0), trained.get_weights(1)))
        S.assert_same_bits(w_tr, S.render_rays(fresh, 0, o, d, z, WEIGHTS_ONLY)[0], "trained vs fresh: coarse weights", finite=True)
        r_fr = fresh.render(o, d, sc, sf, u_c, u_f)
        for i, (a, b) in enumerate(zip(r_tr, r_fr)):
            S.assert_same_bits(np.asarray(a), np.asarray(b), f"trained vs fresh: render output {i}", finite=True)
        trained.train_end()
    finally:
        trained.close()
        if fresh is not None:
            fresh.close()
