"""CPU checks of the native-rate ingestion's host half: q2a_resampled_length (both libraries and the Python mirror)
against the formula, and q2a_read_wav_native on files written with Python's wave module (no GPU work)."""
import ctypes as C
import os
import subprocess
import wave

import numpy as np
import pytest

from conftest import PKG

ERR_ARG, ERR_UNSUPPORTED = -4, -6


@pytest.fixture(scope="module")
def libs():
    subprocess.check_call(["make", "-C", PKG, "-j8", "all"], stdout=subprocess.DEVNULL)
    out = [C.CDLL(os.path.join(PKG, "lib", n)) for n in ("libq2a_host.so", "libq2a.so")]
    for L in out:
        L.q2a_resampled_length.restype = C.c_int64
        L.q2a_resampled_length.argtypes = [C.c_int64, C.c_int]
        L.q2a_read_wav_native.argtypes = [C.c_char_p, C.POINTER(C.POINTER(C.c_int16)), C.POINTER(C.c_int64),
                                          C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.q2a_wav_free.argtypes = [C.c_void_p]
    return out


RATES = [8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000, 8025]


@pytest.mark.parametrize("rate", RATES)
def test_resampled_length(libs, rate):
    import q2a
    for n in (0, 1, 2, rate - 1, rate, rate + 1, 1323000, 2 ** 40 + 12345):
        want = (n * 16000 + rate - 1) // rate
        assert [L.q2a_resampled_length(n, rate) for L in libs] == [want, want]
        assert q2a.resampled_length(n, rate) == want


@pytest.mark.parametrize("n,rate,rc", [(-1, 48000, ERR_ARG), (2 ** 62, 48000, ERR_ARG), (100, 44101, ERR_UNSUPPORTED),
                                        (100, 7999, ERR_UNSUPPORTED), (100, 192001, ERR_UNSUPPORTED), (100, 0, ERR_UNSUPPORTED),
                                        (100, 16001, ERR_UNSUPPORTED)])
def test_resampled_length_errors(libs, n, rate, rc):
    import q2a
    assert [L.q2a_resampled_length(n, rate) for L in libs] == [rc, rc]
    with pytest.raises(q2a.Q2AError) as e:
        q2a.resampled_length(n, rate)
    assert e.value.rc == rc


def read_native(L, path):
    p, n, ch, hz = C.POINTER(C.c_int16)(), C.c_int64(), C.c_int(), C.c_int()
    rc = L.q2a_read_wav_native(str(path).encode(), C.byref(p), C.byref(n), C.byref(ch), C.byref(hz))
    if rc != 0:
        return rc, None, 0, 0
    a = np.ctypeslib.as_array(p, shape=(n.value, ch.value)).copy() if n.value else np.zeros((0, ch.value), np.int16)
    L.q2a_wav_free(p)
    return rc, a, ch.value, hz.value


@pytest.mark.parametrize("channels,cut", [(1, 0), (2, 0), (2, 1001)])
def test_read_wav_native(libs, tmp_path, channels, cut):
    """44.1 kHz mono and stereo; cut: bytes missing at the end of the data chunk (whole frames that are there come back)."""
    s16 = np.random.default_rng(channels).integers(-32768, 32768, (5000, channels), dtype=np.int16)
    path = tmp_path / "n.wav"
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(44100)
        w.writeframes(s16.tobytes())
    if cut:
        path.write_bytes(path.read_bytes()[:-cut])
    want = s16[: (s16.size * 2 - cut) // (2 * channels)]
    for L in libs:
        rc, a, ch, hz = read_native(L, path)
        assert (rc, ch, hz) == (0, channels, 44100)
        assert np.array_equal(a, want)


def test_read_wav_native_refuses(libs, tmp_path):
    path = tmp_path / "b.wav"
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(1)
        w.setframerate(44100)
        w.writeframes(bytes(100))
    (tmp_path / "bad.wav").write_bytes(b"ID3\x03" + bytes(100))
    assert read_native(libs[0], path)[0] == -2
    assert read_native(libs[0], tmp_path / "bad.wav")[0] == -1
