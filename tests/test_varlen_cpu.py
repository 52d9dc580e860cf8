"""CPU checks of the variable-length encode's host side (include/q2a_encoder.h): the packed layout q2a_varlen_rows
through lib/libq2a_host.so (no GPU, no HIP runtime), through libq2a.so and through q2a.varlen_rows, and the four new
entry points' declarations and exports."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import q2a
from conftest import PKG, ROOT

T = 1500
ERR_ARG = -4
NEW_ENTRY_POINTS = ("q2a_encode_device_varlen", "q2a_encode_host_varlen", "q2a_test_attention_varlen",
                    "q2a_test_block_varlen")

LENS = [1, 15, 16, 17, 1488, 1489, 1500, 0]
SEGS = [16, 16, 16, 32, 1488, 1500, 1500, 0]


def _bind(L):
    L.q2a_varlen_rows.restype = C.c_int64
    L.q2a_varlen_rows.argtypes = [C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(C.c_int32)]
    return L


@pytest.fixture(scope="module")
def host_lib(host_build):
    return _bind(C.CDLL(os.path.join(PKG, "lib", "libq2a_host.so")))


def _call(L, lens, n=None, t=T):
    kl = np.asarray(lens, dtype=np.int32)
    rs = np.full(len(kl) + 1, -7, dtype=np.int32)
    i32p = C.POINTER(C.c_int32)
    m = L.q2a_varlen_rows(kl.ctypes.data_as(i32p), len(kl) if n is None else n, t, rs.ctypes.data_as(i32p))
    return m, list(rs)


def _prefix(segs):
    return [0] + [int(x) for x in np.cumsum(segs)]


def test_varlen_rows_host_library(host_lib):
    assert SEGS == [0 if k == 0 else min((k + 15) // 16 * 16, T) for k in LENS]
    m, rs = _call(host_lib, LENS)
    assert rs == _prefix(SEGS)
    assert m == sum(SEGS) == rs[-1]


def test_varlen_rows_python(host_build):
    m, rs = q2a.varlen_rows(LENS)
    assert m == sum(SEGS) and list(rs) == _prefix(SEGS) and rs.dtype == np.int32
    m, rs = q2a.varlen_rows([5, 8, 0, 3], n_audio_ctx=8)   # another window: the cap follows it
    assert (m, list(rs)) == (24, [0, 8, 16, 16, 24])


def test_varlen_rows_every_length(host_lib):
    """Segments are whole 16-row blocks inside the window, hold the clip's rows, and waste at most 15."""
    lens = list(range(0, T + 1))
    m, rs = _call(host_lib, lens)
    segs = np.diff(rs)
    for k, s in zip(lens, segs):
        assert s == (0 if k == 0 else min((k + 15) // 16 * 16, T))
        assert k <= s <= k + 15 and (s % 16 == 0 or s == T)
    assert m == rs[-1] == segs.sum()


def test_varlen_rows_rejects_bad_arguments(host_lib):
    for bad in ([-1], [T + 1], [100, -5, 100], [100, T + 1]):
        m, rs = _call(host_lib, bad)
        assert m == ERR_ARG, bad
        assert all(r == -7 for r in rs), "nothing is written on an error"
        with pytest.raises(q2a.Q2AError) as ei:
            q2a.varlen_rows(bad)
        assert ei.value.rc == ERR_ARG
    for n in (0, -1):
        assert _call(host_lib, [100], n=n)[0] == ERR_ARG
    assert _call(host_lib, [1], t=0)[0] == ERR_ARG
    with pytest.raises(q2a.Q2AError):
        q2a.varlen_rows([])
    kl = (C.c_int32 * 1)(100)
    assert host_lib.q2a_varlen_rows(kl, 1, T, None) == ERR_ARG
    assert host_lib.q2a_varlen_rows(None, 1, T, kl) == ERR_ARG


def test_varlen_rows_is_exported_from_the_hip_library_too():
    L = _bind(q2a.lib())
    m, rs = _call(L, LENS)
    assert m == sum(SEGS) and rs == _prefix(SEGS)
    assert _call(L, [T + 1])[0] == ERR_ARG


def test_new_entry_points_are_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "q2a_encoder.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = q2a.lib()
    for name in NEW_ENTRY_POINTS + ("q2a_varlen_rows",):
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared"
        assert hasattr(L, name), f"{name} is not exported"
        assert name in q2a.EXPORTS
    for name in ("encode_device_varlen", "encode_host_varlen", "test_attention_varlen", "test_block_varlen"):
        assert callable(getattr(q2a.Engine, name))


def test_new_entry_points_fail_cleanly_without_an_engine():
    """Without a HIP device no engine can be opened; the entry points answer a NULL engine with an error code before
    touching the device, as the other entry points do."""
    L = q2a.lib()
    kl = (C.c_int32 * 1)(100)
    ns = (C.c_int32 * 1)(160000)
    st = (C.c_int32 * 1)(-1)
    i32p = C.POINTER(C.c_int32)
    assert L.q2a_encode_device_varlen(None, None, 0, ns, None, kl, 1, None, None, st, None) == ERR_ARG
    assert L.q2a_encode_host_varlen(None, None, ns, None, kl, 1, None, None, st) == ERR_ARG
    assert L.q2a_test_attention_varlen(None, None, None, None, 1, kl, None, None) == ERR_ARG
    assert L.q2a_test_block_varlen(None, 0, None, 1, kl, None) == ERR_ARG
    assert st[0] == -1
    assert C.cast(kl, i32p)[0] == 100


def test_padded_queries_alone_rebase_the_last_block():
    """The premise of tests/test_gpu_varlen.py::test_padded_queries_rebase_the_valid_rows, on the model of the kernel's
    re-base policy (tests/attn_model.py): in block 92 of the clip of varlen_cases the padded queries 1481 .. 1487
    trigger re-bases, and with them silenced the nine valid queries trigger none."""
    import attn_model
    import varlen_cases as vc
    assert (vc.VALID.start, vc.VALID.stop, vc.PADDED.stop) == (1472, 1481, 1488)
    for q, k, v in vc.rebase_heads():
        _, loud = attn_model.model(q, k, v, vc.KEY_LEN, [vc.BLOCK])
        _, quiet = attn_model.model(vc.quiet_padding(q), k, v, vc.KEY_LEN, [vc.BLOCK])
        assert loud[0] >= 1 and quiet[0] == 0, (loud, quiet)


def test_no_device_engine_open_fails_before_the_new_entry_points():
    import torch
    if torch.cuda.is_available():
        return   # a GPU is present: tests/test_gpu_varlen.py covers the calls
    L = q2a.lib()
    L.q2a_open.restype = C.c_void_p
    L.q2a_last_error.restype = C.c_char_p
    assert not L.q2a_open(b"/nonexistent.bin", 0)
    assert L.q2a_last_error()
