"""The sigma-first operand stream of the rgb-skipping f16x3 kernel (csrc/mlp_f16x3.hip: mlp_f16x3_rgbskip_kernel): the gather
table of every config that keeps it against the hashes recorded in tests/golden/stream_table_hashes_rgbskip.txt (64-bit FNV-1a
over the table's int32 entries, the format of stream_table_hashes.txt).  The table was checked slot by slot against the full
stream's when the hashes were recorded: layers 0..7 the same chunks, the sigma tile the full stream's fifth tile of layer 8,
the four rgb tiles its first four, zero padding behind both.  Host only: no device is touched."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND = b"f16x3skip"          # the kind by the name the fixture gives it
NO_SUCH_KIND = 2 ** 64 - 1


def _recorded():
    rows = []
    with open(os.path.join(ROOT, "tests", "golden", "stream_table_hashes_rgbskip.txt")) as f:
        for line in f:
            key, digest = line.rsplit(" ", 1)
            kv = dict(p.split("=") for p in key.split()[:4])
            assert key.split()[4] == "f16x3skip", key
            rows.append((int(kv["lx"]), int(kv["ld"]), int(kv["na"]), int(kv["which"]), digest.strip()))
    return rows


def _hash_fn():
    from nerf_and_dietnerf_amd import _lib
    fn = _lib.load().nerf_debug_stream_table_hash
    fn.restype = C.c_ulonglong
    fn.argtypes = [C.c_int] * 4 + [C.c_char_p]
    return fn


def test_kind_is_looked_up_by_name():
    assert _hash_fn()(5, 4, 2, 1, b"no-such-kind") == NO_SUCH_KIND
    assert _hash_fn()(5, 4, 2, 1, KIND) not in (0, NO_SUCH_KIND)


def test_fixture_lists_every_config_that_keeps_the_stream():
    rows = _recorded()
    assert sorted((lx, ld, na, w) for lx, ld, na, w, _ in rows) == sorted(
        (lx, ld, na, w) for lx in (5, 3) for ld in (4, 2) for na in (2, 1) for w in (0, 1))


@pytest.mark.parametrize("lx,ld,na,which,digest", _recorded())
def test_sigma_first_table_hash(lx, ld, na, which, digest):
    assert f"{_hash_fn()(lx, ld, na, which, KIND):016x}" == digest


@pytest.mark.parametrize("lx,ld,na", [(10, 4, 2), (8, 2, 1), (5, 4, 0)])
def test_wide_and_xyz_only_networks_keep_no_such_stream(lx, ld, na):
    assert _hash_fn()(lx, ld, na, 1, KIND) == 0
