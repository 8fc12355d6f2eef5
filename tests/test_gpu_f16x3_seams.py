"""The schedule of the 3-pass render kernels (mlp_f16x3_kernel, mlp_f16x3_sig_kernel; csrc/mlp_f16x3.hip) across layer
and tile boundaries: fragment sets that ping-pong between layers, state handed from one body to the next, a persistent
loop in which a workgroup runs several tiles.  None of that may change a bit of any row.

(a) Launch-split invariance.  A row's result depends on that row alone, so the rows of one launch must equal, bit for
    bit, the same rows computed in separate launches of at most CUs x 128 rows -- launches in which no workgroup sees a
    second tile, so nothing is carried over from a previous tile and nothing is fetched ahead for a next one.
(b) Agreement with the exact-fp32 mode of the same context within the bar of tests/test_gpu_parity.py::
    test_f16x3_model_predict: 5e-5 relative to max(1, |ref|).  model_predict: on the raw outputs, as there.
    render_rays returns composited quantities: rgb_samples = sigmoid(raw rgb) (a 1/4-contraction, |.| < 1) is held to
    5e-5; the weights of all samples but a ray's last are held to (FAR - NEAR) x 5e-5, because
    w_s = alpha_s T_s with alpha = 1 - exp(-relu(sigma) delta) moves by at most sum_{k <= s} delta_k |d sigma_k|
    <= (z_(s+1) - z_0) max|d sigma|.  A ray's last sample has delta = 1e9, its weight is a step function of sigma's
    sign and is left to (a).
(c) read_nonfinite() == 0.

Row counts: 1; 127, 129, 257 (ragged tiles); 2 CUs 128 + 77 and 3 CUs 128 + 1 (every workgroup runs 2-3 tiles, the weight
ring wraps).  model_predict (mode 1) and render_rays with S = 1 run exactly these; S = 3 and S = 64 (the ray changes inside
a wave's 32 rows) run the fewest rays that give at least as many rows.  render_rays with outputs {weights} is the
sigma-only kernel, with more outputs the full network.  Networks: plain Glorot blobs, Glorot kernels with random biases
and a lifted sigma bias (tests/f16_variants.py), and the shipped epoch-95 checkpoint."""
import numpy as np
import pytest

import f16_variants as V
import support as S

pytestmark = pytest.mark.gpu

NEAR, FAR = 0.6, 2.4
BAR = 5e-5                      # tests/test_gpu_parity.py::test_f16x3_model_predict
NETS = ("glorot", "glorot_biased", "checkpoint")
SAMPLES = (1, 3, 64)


def _row_counts():
    cus = S.n_cus()
    return [1, 127, 129, 257, 2 * cus * 128 + 77, 3 * cus * 128 + 1]


ROW_IDS = ["1", "127", "129", "257", "2wg+77", "3wg+1"]


@pytest.fixture(scope="module")
def contexts(golden_ckpt):
    import nerf_and_dietnerf_amd as N
    blobs = {"glorot": (N.glorot_blob(0), N.glorot_blob(1)), "glorot_biased": V.blobs(5, 4, 2),
             "checkpoint": (golden_ckpt["blob_coarse"], golden_ckpt["blob_fine"])}
    ctxs = {name: S.blob_context(pair, near=NEAR, far=FAR) for name, pair in blobs.items()}
    yield ctxs
    for ctx in ctxs.values():
        ctx.close()


def _rel(a, ref):
    return float(np.abs(a - ref).max()) / max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("rows_i", range(6), ids=ROW_IDS)
@pytest.mark.parametrize("net", NETS)
def test_model_predict_split_invariant_and_fp32_class(contexts, net, rows_i):
    ctx = contexts[net]
    m = _row_counts()[rows_i]
    step = S.n_cus() * 128
    xyz, dirs = V.inputs(m, 2)
    for which in (0, 1):
        one = ctx.model_predict(which, xyz, dirs)
        parts = np.concatenate([ctx.model_predict(which, xyz[i:i + step], dirs[i:i + step]) for i in range(0, m, step)])
        S.assert_same_bits(one, parts, f"{net} net {which} M={m}: one launch vs launches of <= {step} rows", finite=True)
        ctx.set_precision("fp32")
        try:
            ref = ctx.model_predict(which, xyz, dirs)
        finally:
            ctx.set_precision("f16x3")
        err = _rel(one, ref)
        print(f"{net} net {which} M={m}: f16x3 vs fp32 mode rel err {err:.3e}")
        assert err <= BAR, (net, which, m, err)
    assert ctx.read_nonfinite() == 0


@pytest.mark.parametrize("rows_i", range(6), ids=ROW_IDS)
@pytest.mark.parametrize("s", SAMPLES)
@pytest.mark.parametrize("net", NETS)
def test_render_rays_split_invariant_and_fp32_class(contexts, net, s, rows_i):
    ctx = contexts[net]
    rows = _row_counts()[rows_i]
    n = (rows + s - 1) // s                      # the fewest rays with at least `rows` rows
    per = max(1, (S.n_cus() * 128) // s)          # rays of a launch in which no workgroup sees a second tile
    o, d, z = S.rays_towards_origin(n, s, NEAR, FAR)
    for full in (True, False):
        label = f"{net} {'full' if full else 'sigma-only'} N={n} S={s}"
        outputs = ("weights", "rgb_samples") if full else ("weights",)       # {weights} alone: the sigma-only kernel
        w, *rs = S.render_rays(ctx, 0, o, d, z, outputs)
        cut = [S.render_rays(ctx, 0, o[i:i + per], d[i:i + per], z[i:i + per], outputs) for i in range(0, n, per)]
        S.assert_same_bits(w, np.concatenate([c[0] for c in cut]), label + ": weights, one launch vs split", finite=True)
        if full:
            S.assert_same_bits(rs[0], np.concatenate([c[1] for c in cut]), label + ": rgb_samples, one launch vs split",
                               finite=True)
        ctx.set_precision("fp32")
        try:
            w_ref, rs_ref = S.render_rays(ctx, 0, o, d, z, ("weights", "rgb_samples"))
        finally:
            ctx.set_precision("f16x3")
        if s > 1:
            err_w = float(np.abs(w[:, :-1] - w_ref[:, :-1]).max())
            print(f"{label}: weights (all but the last sample) vs fp32 mode max-abs {err_w:.3e}")
            assert err_w <= (FAR - NEAR) * BAR, (label, err_w)
        if full:
            err_c = float(np.abs(rs[0] - rs_ref).max())
            print(f"{label}: rgb_samples vs fp32 mode max-abs {err_c:.3e}")
            assert err_c <= BAR, (label, err_c)
    assert ctx.read_nonfinite() == 0
