"""The sigma-only coarse pass of the f16x3 mode (mlp_f16x3_sig_kernel + the weights-only composite, csrc/nerf_api.hip,
dev_render_rays): a coarse render_rays call that asks for the weights alone -- the coarse pass of NeRF.render -- must
return the very bits of the full kernel's weights output.

Both paths are reached through nerf_render_rays on one context: outputs {weights} take the sigma-only path, outputs
{weights, rgb} the full network.  Row counts cover one row, ragged tiles, and 2 x CUs x 128 + 77 rows (every workgroup
of the persistent grid loops at least twice: the weight stream wraps).  The trainer's path re-packs the sigma-only
stream on the device from its own gather table (train_api.hip, train_flush_weights); a render between train_steps must
match a context freshly loaded with the trained weights bit for bit."""
import ctypes as C

import numpy as np
import pytest

import f16_variants as V

pytestmark = pytest.mark.gpu

NEAR, FAR = 0.6, 2.4


def _n_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _rays(n, s, seed=3):
    """n rays towards the origin from radius ~2, and n x s sorted depths in [NEAR, FAR]."""
    rng = np.random.default_rng(seed)
    o = np.zeros((n, 4), np.float32)
    o[:, :3] = rng.uniform(-0.3, 0.3, (n, 3))
    o[:, 2] += 1.5
    d = np.zeros((n, 4), np.float32)
    d[:, :3] = rng.uniform(-0.4, 0.4, (n, 3))
    d[:, 2] = -1.0
    z = np.sort(rng.uniform(NEAR, FAR, (n, s)), axis=1).astype(np.float32)
    return o, d, z


def _render_rays(ctx, o, d, z, with_rgb):
    """nerf_render_rays on the coarse network with outputs {weights} (with_rgb False) or {weights, rgb}."""
    from nerf_and_dietnerf_amd import _lib
    n, s = z.shape
    w = np.full((n, s), np.nan, np.float32)
    rgb = np.full((n, 3), np.nan, np.float32)
    outs = _lib.NerfOutputs()
    outs.weights = w.ctypes.data
    if with_rgb:
        outs.rgb = rgb.ctypes.data
    _lib.check(ctx.lib.nerf_render_rays(ctx.h, 0, o.ctypes.data, d.ctypes.data, z.ctypes.data, n, s, C.byref(outs),
                                        _lib.NERF_MEM_HOST))
    return w


def _context(blob_pair, lx=5, ld=4, na=2):
    import nerf_and_dietnerf_amd as N
    ctx = N.Context(near=NEAR, far=FAR, precision="f16x3", **V.kw(lx, ld, na))
    for which, blob in enumerate(blob_pair):
        ctx.load_weights(which, blob)
    return ctx


def _assert_same_bits(a, b, label):
    assert a.shape == b.shape and np.isfinite(a).all(), label
    diff = int(np.count_nonzero(a.view(np.uint32) != b.view(np.uint32)))
    assert diff == 0, (label, diff, float(np.abs(a - b).max()))


def _shapes():
    return [(1, 1), (1, 64), (37, 64), (129, 3), (2 * _n_cus() * 128 + 77, 1), (2 * _n_cus() * 2 + 1, 64)]


def _check_all_shapes(ctx, label):
    for n, s in _shapes():
        o, d, z = _rays(n, s)
        full = _render_rays(ctx, o, d, z, True)
        sig = _render_rays(ctx, o, d, z, False)
        _assert_same_bits(sig, full, f"{label} N={n} S={s}")
        if s > 1 and n > 1:
            assert full.max() > 1e-3, (label, n, s)      # the weights are not trivially zero


@pytest.mark.parametrize("lx,ld,na", [(5, 4, 2), (5, 4, 1), (3, 2, 2)])
def test_weights_only_coarse_pass_is_bit_identical(lx, ld, na):
    ctx = _context(V.blobs(lx, ld, na), lx, ld, na)
    try:
        _check_all_shapes(ctx, f"({lx},{ld},{na})")
        assert ctx.read_nonfinite() == 0
    finally:
        ctx.close()


def test_weights_only_coarse_pass_glorot_weights():
    import nerf_and_dietnerf_amd as N
    ctx = _context((N.glorot_blob(0), N.glorot_blob(1)))
    try:
        for n, s in _shapes():
            o, d, z = _rays(n, s)
            _assert_same_bits(_render_rays(ctx, o, d, z, False), _render_rays(ctx, o, d, z, True), f"glorot N={n} S={s}")
    finally:
        ctx.close()


def test_weights_only_coarse_pass_shipped_checkpoint(golden_ckpt):
    ctx = _context((golden_ckpt["blob_coarse"], golden_ckpt["blob_fine"]))
    try:
        _check_all_shapes(ctx, "shipped checkpoint")
    finally:
        ctx.close()


def test_render_between_train_steps_matches_fresh_network():
    """The trained network's sigma-only stream comes from the trainer's gather table: its coarse weights and the whole
    render must equal those of a context loaded from the trained blobs."""
    rng = np.random.default_rng(7)
    n, sc, sf = 512, 64, 128
    o, d, _ = _rays(n, 1, seed=9)
    tgt = rng.random((n, 3), dtype=np.float32)
    u_c, u_f = rng.random((n, sc), dtype=np.float32), rng.random((n, sf), dtype=np.float32)
    trained = _context(V.blobs(5, 4, 2))
    fresh = None
    try:
        trained.train_begin(5e-4)
        for _ in range(2):
            trained.train_step(o, d, tgt, sc, sf, u_c, u_f)
        _, _, z = _rays(n, sc, seed=10)
        w_tr = _render_rays(trained, o, d, z, False)
        _assert_same_bits(w_tr, _render_rays(trained, o, d, z, True), "trained: sigma-only vs full")
        r_tr = trained.render(o, d, sc, sf, u_c, u_f)
        fresh = _context((trained.get_weights(0), trained.get_weights(1)))
        _assert_same_bits(w_tr, _render_rays(fresh, o, d, z, False), "trained vs fresh: coarse weights")
        r_fr = fresh.render(o, d, sc, sf, u_c, u_f)
        for i, (a, b) in enumerate(zip(r_tr, r_fr)):
            _assert_same_bits(np.asarray(a), np.asarray(b), f"trained vs fresh: render output {i}")
        trained.train_end()
    finally:
        trained.close()
        if fresh is not None:
            fresh.close()
