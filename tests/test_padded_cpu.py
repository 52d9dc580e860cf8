"""CPU checks of q2a_valid_lengths (include/q2a_encoder.h): the valid encoder positions and output vectors of a clip
shorter than the 30 s window, through lib/libq2a_host.so (no GPU, no HIP runtime), through libq2a.so, and through
q2a.valid_lengths."""
import ctypes as C
import os

import pytest

import q2a
from conftest import PKG

T = 1500
ERR_ARG = -4

# (n_samples, offset_ms) -> (enc_len, out_len)
CASES = [
    ((480000, 0), (1500, 750)),
    ((16000, 0), (50, 25)),
    ((116800, 0), (365, 182)),
    ((116800, 1000), (315, 157)),
    ((960000, 0), (1500, 750)),   # capped at the window
]


def _from_expression(n, offset_ms):
    """The same lengths from n_len_org = 1 + (n - 200) / 160 (the mel frames the reference computes), then conv2
    (stride 2) and AvgPool1d(2)."""
    n_len_org = 1 + (n - 200) // 160
    frames = min(max(n_len_org - offset_ms // 10, 1), 2 * T)
    enc = (frames - 1) // 2 + 1
    return enc, enc // 2


@pytest.fixture(scope="module")
def host_lib(host_build):
    L = C.CDLL(os.path.join(PKG, "lib", "libq2a_host.so"))
    L.q2a_valid_lengths.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    return L


def _call(L, n, off, t=T):
    a, b = C.c_int32(-7), C.c_int32(-7)
    rc = L.q2a_valid_lengths(n, off, t, C.byref(a), C.byref(b))
    return rc, (a.value, b.value)


@pytest.mark.parametrize("args,want", CASES)
def test_valid_lengths_host_library(host_lib, args, want):
    assert _from_expression(*args) == want
    assert _call(host_lib, *args) == (0, want)


@pytest.mark.parametrize("args,want", CASES)
def test_valid_lengths_python(host_build, args, want):
    assert q2a.valid_lengths(*args) == want
    assert q2a.valid_lengths(args[0], offset_ms=args[1], n_audio_ctx=T) == want


def test_valid_lengths_rejects_negative_arguments(host_lib):
    for bad in ((-1, 0, T), (16000, -10, T), (16000, 0, -1)):
        rc, _ = _call(host_lib, *bad)
        assert rc == ERR_ARG, bad
        with pytest.raises(q2a.Q2AError) as ei:
            q2a.valid_lengths(*bad)
        assert ei.value.rc == ERR_ARG


def test_valid_lengths_edges(host_lib):
    """Never below one encoder position (a clip too short to encode still gets a legal key length), NULL outputs are
    allowed, and the lengths grow monotonically with the sample count."""
    assert _call(host_lib, 0, 0) == (0, (1, 0))
    assert _call(host_lib, 16000, 30000) == (0, (1, 0))
    assert host_lib.q2a_valid_lengths(16000, 0, T, None, None) == 0
    prev = 0
    for n in range(0, 500000, 997):
        rc, (enc, out) = _call(host_lib, n, 0)
        assert rc == 0 and (enc, out) == _from_expression(n, 0) and prev <= enc <= T and out == enc // 2
        prev = enc


def test_valid_lengths_is_exported_from_the_hip_library_too():
    """libq2a.so exports the same function (it loads without a GPU)."""
    L = q2a.lib()
    L.q2a_valid_lengths.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    for args, want in CASES:
        assert _call(L, *args) == (0, want)
    assert _call(L, -1, 0)[0] == ERR_ARG
