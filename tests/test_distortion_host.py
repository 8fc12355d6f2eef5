"""The distortion loss without a GPU: the prefix-sum restatement the kernel evaluates against the pairwise definition, two
rays worked by hand, the C ABI's three new names in header, binding and Context, and render_config["distortion_loss"]."""
import os
import re

import numpy as np
import pytest

import distortion_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR, FAR = 2.0, 6.0


@pytest.mark.parametrize("s", [1, 2, 63, 64, 65, 129, 256])
def test_restatement_equals_the_pairwise_definition(s):
    """float64 on both sides: the O(S) form is the double sum and its autograd gradient, to rounding (values up to ~2)."""
    w, z = D.operator_inputs(5, s, NEAR, FAR, seed=s)
    assert not D.has_ties(z, NEAR, FAR)
    ref = D.pairwise_grads(w, z, NEAR, FAR)
    got = D.restated(w, z, NEAR, FAR, np.float64)
    for name, a, b in zip(("L_ray", "dL/dw", "dL/dz"), got, ref):
        assert a.shape == b.shape and a.dtype == np.float64
        assert np.abs(a - b).max() <= 1e-13, (name, s, float(np.abs(a - b).max()))
    assert not got[0][1] and not got[1][1].any() and not got[2][1].any()         # the all-zero ray


def test_two_samples_by_hand():
    """near 0, far 1, z = (0.2, 0.6): t = (0.2, 0.6), intervals [0.2, 0.6], [0.6, 1]: m = (0.4, 0.8), d = (0.4, 0.4).
    With w = (a, b): L = 2 a b |0.4 - 0.8| + (a^2 + b^2) 0.4 / 3 = 0.8 a b + (a^2 + b^2) 0.4 / 3.
    dL/da = 0.8 b + 0.8 a / 3, dL/db = 0.8 a + 0.8 b / 3.
    z_0 moves t_0 only: m_0 by 1/2, d_0 by -1: dL/dz_0 = 2 a b (-1/2) - a^2 / 3 = -a b - a^2 / 3.
    z_1 moves t_1: m_0 by 1/2, d_0 by +1, m_1 by 1/2, d_1 by -1; the pair term depends on m_1 - m_0 only, which does not move:
    dL/dz_1 = a^2 / 3 - b^2 / 3."""
    a, b = 0.3, 0.5
    w, z = np.array([[a, b]]), np.array([[0.2, 0.6]])
    want = (0.8 * a * b + (a * a + b * b) * 0.4 / 3, [0.8 * b + 0.8 * a / 3, 0.8 * a + 0.8 * b / 3],
            [-a * b - a * a / 3, (a * a - b * b) / 3])
    for got in (D.restated(w, z, 0.0, 1.0), D.pairwise_grads(w, z, 0.0, 1.0)):
        np.testing.assert_allclose(got[0], [want[0]], rtol=0, atol=1e-15)
        np.testing.assert_allclose(got[1], [want[1]], rtol=0, atol=1e-15)
        np.testing.assert_allclose(got[2], [want[2]], rtol=0, atol=1e-15)


def test_all_weight_in_one_sample():
    """A ray whose weight sits in sample k alone has no pair term: L = w^2 d_k / 3 exactly -- in the restatement at float32
    too, where every cancelling term is an exact zero."""
    s, k, wk = 9, 4, np.float32(0.75)
    z = (NEAR + (FAR - NEAR) * (np.arange(s) + 0.5) / s).astype(np.float32)[None]
    w = np.zeros((1, s), np.float32)
    w[0, k] = wk
    for dtype in (np.float64, np.float32):
        f = np.dtype(dtype).type
        t = (z.astype(dtype) - f(NEAR)) / (f(FAR) - f(NEAR))
        d_k = t[0, k + 1] - t[0, k]
        loss, dw, dz = D.restated(w, z, NEAR, FAR, dtype)
        assert loss[0] == f(wk) * f(wk) * d_k / f(3)
        assert dw[0, k] == f(2) * f(wk) * d_k / f(3)
        # the empty samples feel the mass at distance |m_i - m_k|: dL/dw_i = 2 w_k |m_i - m_k|
        m = (t[0] + np.append(t[0, 1:], f(1))) * f(0.5)
        np.testing.assert_allclose(np.delete(dw[0], k), np.delete(2 * f(wk) * np.abs(m - m[k]), k), rtol=0, atol=1e-6)
        # only the two ends of the interval move the loss
        assert not np.delete(dz[0], [k, k + 1]).any() and dz[0, k] < 0 < dz[0, k + 1]
    # the last sample owns [t_{S-1}, 1]
    w[:] = 0
    w[0, s - 1] = wk
    loss, _, _ = D.restated(w, z, NEAR, FAR, np.float64)
    assert abs(loss[0] - 0.75 ** 2 * (1.0 - (float(z[0, -1]) - NEAR) / (FAR - NEAR)) / 3) <= 1e-15


def test_header_binding_and_context_agree():
    import nerf_and_dietnerf_amd as N
    with open(os.path.join(ROOT, "include", "nerf_mi355.h")) as f:
        text = f.read()
    names = ("nerf_train_set_distortion_weights", "nerf_train_read_distortion_sums", "nerf_distortion_loss")
    bound = {n: args for n, _, args in N._lib.SYMBOLS}
    for n in names:
        assert re.search(r"\bint " + n + r"\(nerf_ctx\* ctx", text), n
        assert n in bound
    assert len(bound["nerf_train_set_distortion_weights"]) == 3 and len(bound["nerf_train_read_distortion_sums"]) == 3
    assert len(bound["nerf_distortion_loss"]) == 9
    assert re.search(r"#define NERF_ABI_VERSION 6\b", text) and N._lib.NERF_ABI_VERSION == 6
    for m in ("train_set_distortion_weights", "train_read_distortion_sums", "distortion_loss"):
        assert callable(getattr(N.Context, m))
    # the header says which paths ignore the regulariser
    doc = text[text.index("ABI 6+, distortion loss"):text.index("int nerf_train_set_distortion_weights")]
    assert "nerf_train_render_gradients" in doc and "do not apply it" in doc
    lib = N._lib.load()
    for n in names:
        assert getattr(lib, n)


def test_render_config_key():
    from nerf_and_dietnerf_amd import config, render
    assert config.DISTORTION_LOSS == render.DISTORTION_LOSS == "distortion_loss"
    chk = render.check_distortion_loss
    assert chk(0.01) == (0.01, 0.01) and chk(0) == (0.0, 0.0) and chk(np.float32(0.5)) == (0.5, 0.5)
    assert chk([0.0, 0.02]) == (0.0, 0.02) and chk((1, 2)) == (1.0, 2.0) and chk(np.array([0.25, 0.0])) == (0.25, 0.0)
    for bad in (True, False, -0.1, float("nan"), float("inf"), [0.1], [0.1, 0.2, 0.3], [0.1, -1.0], [True, 0.1],
                [0.1, float("nan")], "0.1", None, {"coarse": 0.1}):
        with pytest.raises(ValueError, match="distortion_loss"):
            chk(bad)


def test_nerf_reports_the_sums_only_under_a_weight():
    """NeRF.train_read_extra_metric_sums is what dataset.fit merges into an epoch's history: no keys without the regulariser."""
    import nerf_and_dietnerf_amd as N

    class Ctx:
        def train_read_distortion_sums(self):
            return {"distortion_coarse": 0.5, "distortion_fine": 0.25}, 2

    m = object.__new__(N.NeRF)
    m.ctx = Ctx()
    assert m.train_read_extra_metric_sums() == ({}, 0)
    for off in (None, (0.0, 0.0)):
        m.distortion_weights = off
        assert m.train_read_extra_metric_sums() == ({}, 0)
    m.distortion_weights = (0.0, 0.01)
    assert m.train_read_extra_metric_sums() == ({"distortion_coarse": 0.5, "distortion_fine": 0.25}, 2)
    # DietNeRF keeps its own key and merges these
    d = object.__new__(N.DietNeRF)
    d.ctx, d._extra_sums, d.distortion_weights = Ctx(), None, (0.01, 0.01)
    assert d.train_read_extra_metric_sums() == ({"distortion_coarse": 0.5, "distortion_fine": 0.25,
                                                 "cosine_similarity_loss": 0.0}, 0)
    d.distortion_weights = None
    assert d.train_read_extra_metric_sums() == ({"cosine_similarity_loss": 0.0}, 0)
