"""CPU checks of the audio-feature calls' host side (include/q2a_encoder.h): the packed output layout
q2a_packed_out_rows through lib/libq2a_host.so (no GPU, no HIP runtime), through libq2a.so and through
q2a.packed_out_rows, against a numpy prefix sum."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import q2a
from conftest import PKG, ROOT

T = 1500
ERR_ARG = -4
i32p = C.POINTER(C.c_int32)


def _bind(L):
    L.q2a_packed_out_rows.restype = C.c_int64
    L.q2a_packed_out_rows.argtypes = [i32p, C.c_int, C.c_int, i32p]
    return L


@pytest.fixture(scope="module")
def host_lib(host_build):
    return _bind(C.CDLL(os.path.join(PKG, "lib", "libq2a_host.so")))


def _rows(L, lens, t=T):
    kl = np.ascontiguousarray(lens, dtype=np.int32)
    out = np.full(len(kl) + 1, -7, dtype=np.int32)
    n = L.q2a_packed_out_rows(kl.ctypes.data_as(i32p), len(kl), t, out.ctypes.data_as(i32p))
    return n, out


def _want(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64) // 2)]).astype(np.int32)


def _cases():
    rng = np.random.default_rng(11)
    yield [1, 2, 3, 15, 16, 17, 31, 33, 365, 1481, 1489, 1500]
    yield [0] * 9
    yield [0, 1500, 0, 1, 0]
    for n in (1, 2, 64, 257):
        yield rng.integers(0, T + 1, size=n).tolist()


def test_packed_out_rows_host_library(host_lib):
    for lens in _cases():
        n, out = _rows(host_lib, lens)
        want = _want(lens)
        assert n == want[-1] and np.array_equal(out, want), lens


def test_packed_out_rows_python(host_build):
    for lens in _cases():
        n, out = q2a.packed_out_rows(lens)
        want = _want(lens)
        assert n == want[-1] and out.dtype == np.int32 and np.array_equal(out, want), lens
    n, out = q2a.packed_out_rows([5, 8, 0, 3], n_audio_ctx=8)
    assert n == 7 and list(out) == [0, 2, 6, 6, 7]


def test_packed_out_rows_of_no_clips(host_lib):
    out = np.full(1, -7, dtype=np.int32)
    assert host_lib.q2a_packed_out_rows(None, 0, T, out.ctypes.data_as(i32p)) == 0 and out[0] == 0
    n, os_ = q2a.packed_out_rows([])
    assert n == 0 and list(os_) == [0]


def test_packed_out_rows_rejects_bad_arguments(host_lib):
    for bad in ([-1], [T + 1], [10, 20, T + 1], [3, -2, 3]):
        n, out = _rows(host_lib, bad)
        assert n == ERR_ARG and (out == -7).all(), "nothing is written on an error"
        with pytest.raises(q2a.Q2AError) as ei:
            q2a.packed_out_rows(bad)
        assert ei.value.rc == ERR_ARG
    kl = np.array([4], dtype=np.int32)
    out = np.zeros(2, dtype=np.int32)
    klp, outp = kl.ctypes.data_as(i32p), out.ctypes.data_as(i32p)
    assert host_lib.q2a_packed_out_rows(klp, -1, T, outp) == ERR_ARG
    assert host_lib.q2a_packed_out_rows(klp, 1, 0, outp) == ERR_ARG
    assert host_lib.q2a_packed_out_rows(klp, 1, -5, outp) == ERR_ARG
    assert host_lib.q2a_packed_out_rows(klp, 1, T, None) == ERR_ARG
    assert host_lib.q2a_packed_out_rows(None, 1, T, outp) == ERR_ARG
    with pytest.raises(q2a.Q2AError):
        q2a.packed_out_rows([4], n_audio_ctx=0)


def test_packed_out_rows_is_exported_from_the_hip_library_too():
    L = _bind(q2a.lib())
    lens = [1500, 17, 0, 365]
    n, out = _rows(L, lens)
    assert n == 750 + 8 + 182 and np.array_equal(out, _want(lens))
    assert _rows(L, [T + 1])[0] == ERR_ARG


NEW_ENTRY_POINTS = ("q2a_packed_out_rows", "q2a_audio_features_device", "q2a_audio_features_device_mel",
                    "q2a_audio_features_host", "q2a_audio_features_host_mel", "q2a_test_pool_operand")


def test_new_entry_points_are_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "q2a_encoder.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = q2a.lib()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared"
        assert hasattr(L, name), f"{name} is not exported"
        assert name in q2a.EXPORTS
    for name in ("audio_features", "audio_features_device", "audio_features_device_mel", "audio_features_host",
                 "audio_features_host_mel", "test_pool_operand"):
        assert callable(getattr(q2a.Engine, name)), name


def test_new_entry_points_fail_cleanly_without_an_engine():
    """Without a HIP device no engine can be opened; the entry points answer a NULL engine with an error code before
    touching the device or the caller's arrays."""
    L = q2a.lib()
    kl = (C.c_int32 * 1)(100)
    ns = (C.c_int32 * 1)(160000)
    st = (C.c_int32 * 1)(-1)
    ol = (C.c_int32 * 1)(-1)
    assert L.q2a_audio_features_device(None, None, None, 0, ns, None, kl, 1, None, None, 750, ol, st, None) == ERR_ARG
    assert L.q2a_audio_features_device_mel(None, None, None, 0, 3000, ns, None, kl, 1, None, None, 750, ol, st, None) == ERR_ARG
    assert L.q2a_audio_features_host(None, None, None, ns, None, kl, 1, None, None, 750, ol, st) == ERR_ARG
    assert L.q2a_audio_features_host_mel(None, None, None, ns, None, kl, 1, None, None, 750, ol, st) == ERR_ARG
    assert L.q2a_test_pool_operand(None, 0, None, 1, kl, None, None, None, None, 0, None) == ERR_ARG
    assert st[0] == -1 and ol[0] == -1 and kl[0] == 100
