"""The encoding window without a GPU: the interface (header, binding, package), the folding identity the design rests on
(float64 autograd, oracle/train_oracle.py), the window formulas, the config key's schedule and the validation errors."""
import os
import re

import numpy as np
import pytest

import encoding_window_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"nerf_ctx_set_encoding_window": 3, "nerf_ctx_get_encoding_window": 4}


def test_new_entry_points_are_declared_bound_wrapped_and_exported():
    import nerf_and_dietnerf_amd as N
    text = open(os.path.join(ROOT, "include", "nerf_mi355.h")).read()
    declared = set(re.findall(r"\b(nerf_[a-z_]+)\s*\(", text))
    bound = {name: args for name, _, args in N._lib.SYMBOLS}
    lib = N._lib.load()
    for name, nargs in NEW.items():
        assert name in declared, name
        assert name in bound and len(bound[name]) == nargs, name
        assert getattr(lib, name) is not None
    assert re.search(r"#define\s+NERF_ABI_VERSION\s+6\b", text) and N._lib.NERF_ABI_VERSION == 6 and lib.nerf_abi_version() == 6
    for method in ("set_encoding_window", "encoding_window"):
        assert callable(getattr(N.Context, method))
    for method in ("set_encoding_alpha", "encoding_window_epoch"):
        assert callable(getattr(N.NeRF, method)) and getattr(N.DietNeRF, method) is getattr(N.NeRF, method)
    assert N.encoding_window is N.render.encoding_window and "encoding_window" in N.__all__
    assert N.config.ENCODING_WINDOW == N.render.ENCODING_WINDOW == "encoding_window"
    # the semantics the header owes its reader
    doc = text[text.index("Coarse-to-fine positional encoding"):text.index("int nerf_ctx_get_encoding_window")]
    doc = re.sub(r"\s*\n \*\s*", " ", doc)
    for phrase in ("the master weights are never scaled", "gradients are with respect to the master weights",
                   "the pass-through component always has weight 1", "survives nerf_train_begin"):
        assert phrase in doc, phrase


@pytest.mark.parametrize("L,Ld,na", [(5, 4, 2), (10, 4, 1), (3, 2, 0)])
def test_scale_table_layout_matches_the_oracles_blob(oracle, L, Ld, na):
    """The reference table has the blob's size and layer shapes, its windowed rows are whole rows, and there are exactly as
    many of them as the rule says."""
    kw = dict(n_pos_enc_xyz=L, n_pos_enc_dir=Ld, n_angles=na)
    rng = np.random.default_rng(L)
    wx, wd = (0.1 + 0.8 * rng.random(L)).astype(np.float32), (0.1 + 0.8 * rng.random(Ld)).astype(np.float32)
    S = W.scale_table(L, Ld, na, wx, wd)
    assert S.size == oracle.blob_size(**kw)
    layers = oracle.unpack_blob(S, **kw)
    assert [k.shape for k, _ in layers] == W.layer_shapes(L, Ld, na)
    rows = 0
    for l, (k, b) in enumerate(layers):
        assert (b == 1).all() and (k == k[:, :1]).all()
        rows += int((k[:, 0] != 1).sum())
        if l in (0, 4):
            assert (k[0::1 + 2 * L][:3] == 1).all()                       # the pass-through rows
            np.testing.assert_array_equal(k[1:1 + 2 * L:2, 0], wx)       # component 0: the sin rows, octave by octave
            np.testing.assert_array_equal(k[2 * (1 + 2 * L) + 2:3 * (1 + 2 * L):2, 0], wx)       # component 2: the cos rows
    assert rows == 2 * 6 * L + (0 if na == 0 else 2 * 2 * Ld * (na + 1))


@pytest.mark.parametrize("L,Ld,na", [(5, 4, 0), (5, 4, 1), (5, 4, 2), (10, 4, 0), (10, 4, 1), (10, 4, 2), (3, 2, 0), (3, 2, 1),
                                     (3, 2, 2)])
def test_folding_identity_in_float64(oracle, monkeypatch, L, Ld, na):
    """The network with MASKED encoding features and blob W computes what the unmodified network computes with blob W (.) S,
    and its weight gradients are S (.) those of the latter: outputs and gradients of the whole training graph (both
    networks, the sampler term) to 1e-12 relative, in float64."""
    import torch
    from oracle import train_oracle as T
    import nerf_and_dietnerf_amd as N
    kw = dict(n_pos_enc_xyz=L, n_pos_enc_dir=Ld, n_angles=na)
    rng = np.random.default_rng(100 * L + 10 * Ld + na)
    wx, wd = 0.1 + 0.8 * rng.random(L), 0.1 + 0.8 * rng.random(Ld)
    wx[rng.integers(L)] = 0.0                                            # one octave fully closed
    S = W.scale_table(L, Ld, na, wx, wd).astype(np.float64)
    mx, md = W.masks(L, Ld, na, wx.astype(np.float32), wd.astype(np.float32))
    blobs = [N.glorot_blob(3 + i, **kw) for i in range(2)]
    for b in blobs:
        b[-1] = 1.5
    n, sc, sf = 6, 5, 4
    o = np.concatenate([rng.uniform(-0.3, 0.3, (n, 3)), np.ones((n, 1))], 1)
    d = np.concatenate([rng.uniform(-1, 1, (n, 3)), np.zeros((n, 1))], 1)
    tgt, u_c, u_f = rng.random((n, 3)), rng.random((n, sc), dtype=np.float32), rng.random((n, sf), dtype=np.float32)
    fw = dict(n_xyz=L, n_dir=Ld, n_angles=na, alpha=0.05)

    def params(blob64):
        out, off = [], 0
        for rows, cols in W.layer_shapes(L, Ld, na):
            for shape in ((rows, cols), (cols,)):
                size = int(np.prod(shape))
                out.append(torch.tensor(blob64[off:off + size].reshape(shape), dtype=torch.float64, requires_grad=True))
                off += size
        assert off == blob64.size
        return out

    def run(ps):
        loss, mse_c, mse_f, z_f = T.train_forward(ps[0], ps[1], o, d, tgt, 0.7, 1.7, u_c, u_f, **fw)
        loss.backward()
        return [float(v.detach()) for v in (loss, mse_c, mse_f)], z_f.detach().numpy(), [T.params_to_blob([t.grad for t in p]) for p in ps]

    folded = run([params(b.astype(np.float64) * S) for b in blobs])
    plain_pe = T._pe

    def masked_pe(x, n_enc, passthrough):
        m = mx if passthrough else md
        return plain_pe(x, n_enc, passthrough) * torch.tensor(m, dtype=x.dtype)
    monkeypatch.setattr(T, "_pe", masked_pe)
    masked = run([params(b.astype(np.float64)) for b in blobs])
    np.testing.assert_allclose(masked[0], folded[0], rtol=1e-12, atol=0)
    np.testing.assert_allclose(masked[1], folded[1], rtol=1e-12, atol=0)
    for g, gp in zip(masked[2], folded[2]):
        assert np.abs(gp).max() > 0
        assert np.abs(g - S * gp).max() <= 1e-12 * np.abs(gp).max()
        assert not g[S == 0].any()


def test_window_formulas():
    import nerf_and_dietnerf_amd as N
    for kind, ref in (("cosine", W.cosine_window), ("linear", W.linear_window)):
        for n in (1, 4, 5, 10):
            assert not N.encoding_window(0.0, n, kind).any()
            assert (N.encoding_window(float(n), n, kind) == 1).all() and (N.encoding_window(n + 3.5, n, kind) == 1).all()
            for alpha in (0.25, 1.0, 2.5, 3.75, n - 0.5):
                w = N.encoding_window(alpha, n, kind)
                assert w.dtype == np.float32 and w.shape == (n,)
                np.testing.assert_array_equal(w, ref(alpha, n).astype(np.float32))
    np.testing.assert_array_equal(N.encoding_window(2.5, 5), np.array([1, 1, 0.5, 0, 0], np.float32))
    np.testing.assert_array_equal(N.encoding_window(2.25, 5, "linear"), np.array([1, 1, 0.25, 0, 0], np.float32))
    with pytest.raises(ValueError, match="kind"):
        N.encoding_window(1.0, 5, "hann")
    with pytest.raises(ValueError, match="n_octaves"):
        N.encoding_window(1.0, 0)
    with pytest.raises(ValueError, match="finite"):
        N.encoding_window(float("nan"), 5)


class _StubCtx:
    def __init__(self):
        self.calls = []

    def set_encoding_window(self, xyz=None, dirs=None):
        self.calls.append((None if xyz is None else np.array(xyz), None if dirs is None else np.array(dirs)))


def _stub_model(cfg, L=5, Ld=4):
    """A NeRF with no context behind it: the schedule is host arithmetic over set_encoding_window."""
    import nerf_and_dietnerf_amd as N
    m = N.NeRF.__new__(N.NeRF)
    m.ctx, m.n_pos_enc_dim_xyz, m.n_pos_enc_view_dir = _StubCtx(), L, Ld
    m.window_config = None if cfg is None else N.render.check_encoding_window(cfg, L)
    m._window_epochs = 0
    return m


def test_config_schedule_on_a_stub_model():
    m = _stub_model({"epochs": 4, "start": 1.0, "kind": "linear", "dirs": True})
    for e in range(6):
        m.encoding_window_epoch()
        alpha = 1.0 + (5.0 - 1.0) * min(e / 4, 1.0)
        wx, wd = m.ctx.calls[-1]
        np.testing.assert_array_equal(wx, W.linear_window(alpha, 5).astype(np.float32))
        np.testing.assert_array_equal(wd, W.linear_window(alpha * 4 / 5, 4).astype(np.float32))
    assert (m.ctx.calls[4][0] == 1).all() and (m.ctx.calls[4][1] == 1).all()       # alpha reached L: all ones = off
    # defaults: cosine, 0 .. L, directions at full band
    m = _stub_model({"epochs": 2})
    for e, alpha in enumerate((0.0, 2.5, 5.0, 5.0)):
        m.encoding_window_epoch()
        wx, wd = m.ctx.calls[-1]
        np.testing.assert_array_equal(wx, W.cosine_window(alpha, 5).astype(np.float32))
        assert wd is None
    # an absent key leaves everything as it was
    m = _stub_model(None)
    m.encoding_window_epoch()
    assert m.ctx.calls == []


def test_fit_calls_the_window_hook_before_the_grid_hook():
    import nerf_and_dietnerf_amd as N
    order = []

    class Ctx:
        def train_read_metric_sums(self):
            return {}, 0

    class Model:
        ctx = Ctx()

        def encoding_window_epoch(self):
            order.append("window")

        def occupancy_grid_epoch(self):
            order.append("grid")

        def train_step(self, batch, group=None, want_metrics=True):
            order.append("step")
    N.fit(Model(), [1, 2], epochs=2)
    assert order == ["window", "grid", "step", "step"] * 2


def test_validation_errors():
    import nerf_and_dietnerf_amd as N
    check = N.render.check_encoding_window
    assert check({"epochs": 3}, 5) == {"kind": "cosine", "start": 0.0, "end": 5.0, "epochs": 3, "dirs": False}
    with pytest.raises(ValueError, match="unknown encoding_window keys"):
        check({"epochs": 3, "epoch": 1}, 5)
    with pytest.raises(ValueError, match="epochs"):
        check({"kind": "cosine"}, 5)
    with pytest.raises(ValueError, match="positive integer"):
        check({"epochs": 0}, 5)
    with pytest.raises(ValueError, match="positive integer"):
        check({"epochs": 1.5}, 5)
    with pytest.raises(ValueError, match="kind"):
        check({"epochs": 2, "kind": "step"}, 5)
    with pytest.raises(ValueError, match="start <= end"):
        check({"epochs": 2, "start": 3.0, "end": 2.0}, 5)
    with pytest.raises(ValueError, match="dict"):
        check(5, 5)
