"""Encoding geometries on the host side (no device needed): the library accepts every network with
n_pos_enc_dim_xyz 1..10 and n_pos_enc_view_dir 1..4 (src/NeRF.py:249-339 builds its layers from these keys), sizes their
weight blobs the way the reference's Keras models do, and refuses everything else with a message that names the ranges."""
import ctypes

import numpy as np
import pytest

LX_RANGE = range(1, 11)
LD_RANGE = range(1, 5)


def _cfg(lx, ld, n_angles, hidden=256, last=128):
    import nerf_and_dietnerf_amd as N
    return N._lib.NerfConfig(lx, ld, n_angles, hidden, last, 0.05, 2.0, 6.0, 0, 0)


@pytest.mark.parametrize("n_angles", [0, 1, 2])
def test_blob_size_matches_the_keras_layer_shapes(n_angles):
    import nerf_and_dietnerf_amd as N
    from oracle import nerf_oracle as O
    lib = N._lib.load()
    for lx in LX_RANGE:
        for ld in LD_RANGE:
            kw = dict(n_pos_enc_xyz=lx, n_pos_enc_dir=ld, n_angles=n_angles)
            got = lib.nerf_blob_size(ctypes.byref(_cfg(lx, ld, n_angles)))
            assert got == N.blob_size(**kw) == O.blob_size(**kw), (lx, ld, n_angles, got, N._lib.last_error())
    # the default geometry keeps its size; the original paper's Lx = 10: 63 inputs to layer 0, 319 to the skip
    assert lib.nerf_blob_size(ctypes.byref(_cfg(5, 4, 2))) == 514332
    assert lib.nerf_blob_size(ctypes.byref(_cfg(10, 4, 2))) == 514332 + 2 * 30 * 256


@pytest.mark.parametrize("lx,ld,hidden", [(0, 4, 256), (11, 4, 256), (16, 4, 256), (5, 0, 256), (5, 5, 256),
                                          (-1, 2, 256), (10, 5, 256), (5, 4, 128)])
def test_unsupported_geometries_fail_with_the_supported_ranges(lx, ld, hidden):
    import nerf_and_dietnerf_amd as N
    lib = N._lib.load()
    bad = _cfg(lx, ld, 2, hidden=hidden)
    assert lib.nerf_blob_size(ctypes.byref(bad)) == 0
    msg = N._lib.last_error()
    assert "n_pos_enc_dim_xyz 1..10" in msg and "n_pos_enc_view_dir 1..4" in msg, msg
    h = ctypes.c_void_p()
    assert lib.nerf_ctx_create(ctypes.byref(bad), ctypes.byref(h)) != 0 and not h.value


@pytest.mark.parametrize("lx,ld,n_angles", [(5, 2, 2), (3, 4, 1), (1, 1, 2), (4, 4, 0), (10, 4, 2), (10, 4, 0)])
def test_checkpoint_round_trip_keeps_the_layer_shapes(tmp_path, lx, ld, n_angles):
    """save_nerf_checkpoint / read_keras_weights at other encodings: every tensor comes back with the shape the
    reference's model has (oracle.layer_shapes) and the blob is unchanged.  (The .h5 layer is pure Python: it also
    carries geometries the native library does not run.)"""
    import nerf_and_dietnerf_amd as N
    from nerf_and_dietnerf_amd import keras_h5
    from oracle import nerf_oracle as O
    kw = dict(n_pos_enc_xyz=lx, n_pos_enc_dir=ld, n_angles=n_angles)
    bc, bf = N.glorot_blob(1, **kw), N.glorot_blob(2, **kw)
    path = str(tmp_path / "NeRF_model_epoch_001.h5")
    keras_h5.save_nerf_checkpoint(path, bc, bf, **kw)
    models = keras_h5.read_keras_weights(path)
    shapes = O.layer_shapes(**kw)
    assert len(models) == 2
    for tensors in models.values():
        assert [t.shape for t in tensors[0::2]] == [tuple(s) for s in shapes]
        assert [t.shape for t in tensors[1::2]] == [(o,) for _, o in shapes]
    rc, rf = keras_h5.load_nerf_checkpoint(path)
    np.testing.assert_array_equal(rc, bc)
    np.testing.assert_array_equal(rf, bf)


@pytest.mark.parametrize("lx", [6, 10])
def test_wide_encodings_have_no_exact_fp32_kernel(lx):
    """n_pos_enc_dim_xyz 6..10 runs on the wide-PE fp16-core kernels only: a context asking for the exact-fp32 mode is
    refused before any device is touched, with the reason; f16x3 / f16 pass the configuration check."""
    import nerf_and_dietnerf_amd as N
    lib = N._lib.load()
    cfg = N._lib.NerfConfig(lx, 4, 2, 256, 128, 0.05, 2.0, 6.0, N._lib.NERF_PRECISION_FP32, 0)
    h = ctypes.c_void_p()
    assert lib.nerf_ctx_create(ctypes.byref(cfg), ctypes.byref(h)) != 0 and not h.value
    assert "not fp32" in N._lib.last_error()
    for p in (N._lib.NERF_PRECISION_F16X3, N._lib.NERF_PRECISION_F16):
        ok = N._lib.NerfConfig(lx, 4, 2, 256, 128, 0.05, 2.0, 6.0, p, 0)
        assert lib.nerf_blob_size(ctypes.byref(ok)) == N.blob_size(n_pos_enc_xyz=lx, n_pos_enc_dir=4, n_angles=2)
