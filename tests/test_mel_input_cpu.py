"""CPU checks of the log-mel entry points' host arithmetic (include/q2a_encoder.h, "encode from log-mel features"):
q2a_mel_valid_lengths through lib/libq2a_host.so, libq2a.so and q2a.mel_valid_lengths; the key lengths
Engine.encode_features derives from a feature_attention_mask; and the window rule of tests/mel_cases.py against the
CPU oracle's copy of the reference's window. No GPU, no HIP runtime."""
import ctypes as C
import os
import types

import numpy as np
import pytest

import mel_cases as mc
import oracle_py
import q2a
from conftest import PKG

T = mc.N_CTX
ERR_ARG = -4


@pytest.fixture(scope="module")
def host_lib(host_build):
    L = C.CDLL(os.path.join(PKG, "lib", "libq2a_host.so"))
    i32p = C.POINTER(C.c_int32)
    L.q2a_valid_lengths.argtypes = [C.c_int, C.c_int, C.c_int, i32p, i32p]
    L.q2a_mel_valid_lengths.argtypes = [C.c_int, C.c_int, C.c_int, i32p, i32p]
    return L


def _call(f, a, b, t=T):
    x, y = C.c_int32(-7), C.c_int32(-7)
    rc = f(a, b, t, C.byref(x), C.byref(y))
    return rc, (x.value, y.value)


# 201 samples (the shortest clip with a mel frame of its own), around 1 s, 7.3 s, one short of / exactly / one past
# 30 s, more than 30 s
SAMPLES = [201, 359, 360, 361, 15999, 16000, 16001, 116800, 479999, 480000, 480001, 480200, 480360, 960000, 1200000]
# 0, an odd seek, a whole window, and offsets past the end of every clip but the longest
OFFSETS_MS = [0, 10, 1000, 10010, 29990, 30000, 59999, 75000]


def test_mel_valid_lengths_equals_valid_lengths_of_the_pcm(host_lib):
    """n_len = 1 + (n_samples - 200) / 160 frames from frame offset_ms / 10 give q2a_valid_lengths(n_samples,
    offset_ms): the two families agree on every clip the PCM entry points accept."""
    n_cases = 0
    for n in SAMPLES + list(range(201, 600000, 7919)):
        n_len = 1 + (n - 200) // 160
        for off in OFFSETS_MS:
            want = _call(host_lib.q2a_valid_lengths, n, off)
            assert want[0] == 0
            assert _call(host_lib.q2a_mel_valid_lengths, n_len, off // 10) == want, (n, off)
            assert want[1] == mc.valid_lengths(n_len, off // 10), (n, off)
            n_cases += 1
    assert n_cases > 500
    # an offset past the end: one encoder position, no output vector
    assert _call(host_lib.q2a_mel_valid_lengths, 100, 101) == (0, (1, 0))
    assert _call(host_lib.q2a_mel_valid_lengths, 100, 2**31 - 1) == (0, (1, 0))
    # capped at the window
    assert _call(host_lib.q2a_mel_valid_lengths, 2**31 - 1, 0) == (0, (T, T // 2))
    assert _call(host_lib.q2a_mel_valid_lengths, 3000, 0) == (0, (1500, 750))
    assert _call(host_lib.q2a_mel_valid_lengths, 777, 100) == (0, (339, 169))
    assert host_lib.q2a_mel_valid_lengths(777, 100, T, None, None) == 0


def test_mel_valid_lengths_errors(host_lib):
    for bad in ((0, 0, T), (-5, 0, T), (100, -1, T), (100, 0, 0), (100, 0, -3)):
        rc, out = _call(host_lib.q2a_mel_valid_lengths, *bad)
        assert rc == ERR_ARG and out == (-7, -7), bad
        with pytest.raises(q2a.Q2AError) as ei:
            q2a.mel_valid_lengths(*bad)
        assert ei.value.rc == ERR_ARG


def test_mel_valid_lengths_python_and_hip_library(host_build):
    assert q2a.mel_valid_lengths(777, 100) == (339, 169)
    assert q2a.mel_valid_lengths(3000) == (1500, 750)
    assert q2a.mel_valid_lengths(3000, seek=0, n_audio_ctx=100) == (100, 50)
    L = q2a.lib()   # libq2a.so exports the same function (it loads without a GPU)
    assert _call(L.q2a_mel_valid_lengths, 777, 100) == (0, (339, 169))
    assert _call(L.q2a_mel_valid_lengths, 0, 0)[0] == ERR_ARG
    for name in ("q2a_mel_valid_lengths", "q2a_encode_device_mel", "q2a_encode_host_mel", "q2a_test_frontend_mel",
                 "whisper_set_mel", "whisper_set_mel_with_state"):
        assert name in q2a.EXPORTS and hasattr(L, name), name


def test_features_key_len_is_the_hf_length_formula():
    """feature_attention_mask -> key_len: (L - 1) // 2 + 1 encoder positions, and the valid output vectors
    key_len // 2 the engine reports equal transformers' second step (e - 2) // 2 + 1, for every L in 1 .. 3000."""
    L = np.arange(1, mc.TM + 1)
    kl = q2a.features_key_len(L)
    assert kl.dtype == np.int32 and kl.min() == 1 and kl.max() == T
    for n, k in zip(L, kl):
        enc, out = mc.hf_lengths(int(n))
        assert (int(k), int(k) // 2) == (enc, out), n
        assert (int(k), int(k) // 2) == mc.valid_lengths(int(n), 0)


def test_encode_features_derives_the_key_lengths_from_the_mask():
    """Engine.encode_features on a numpy batch hands the host entry point the whole L frames of every clip and the
    mask's key lengths (a stand-in for the engine records the call: no GPU here)."""
    seen = {}

    def encode_host_mel(mels, kind=0, key_len=None, **kw):
        seen.update(n_len=[m.shape[1] for m in mels], kind=kind, key_len=None if key_len is None else list(key_len))
        return np.zeros((len(mels), 750, 8), np.float32), np.zeros(len(mels), np.int32), np.zeros(len(mels), np.int32)

    fake = types.SimpleNamespace(info=types.SimpleNamespace(n_mels=4, n_out=750), out_shape=(750, 8),
                                 encode_host_mel=encode_host_mel)
    x = np.zeros((3, 4, 3000), np.float32)
    mask = np.zeros((3, 3000), np.int64)
    for c, n in enumerate((3000, 777, 1)):
        mask[c, :n] = 1
    q2a.Engine.encode_features(fake, x, mask)
    assert seen == dict(n_len=[3000] * 3, kind=q2a.ENCODE_VARLEN, key_len=[1500, 389, 1])
    q2a.Engine.encode_features(fake, x, mask, kind="padded")
    assert seen["kind"] == q2a.ENCODE_PADDED and seen["key_len"] == [1500, 389, 1]
    q2a.Engine.encode_features(fake, x)
    assert seen["key_len"] is None
    _, ol = q2a.Engine.encode_features(fake, x, mask, kind="plain")
    assert seen["kind"] == q2a.ENCODE_PLAIN and seen["key_len"] is None and list(ol) == [750] * 3
    with pytest.raises(ValueError):
        q2a.Engine.encode_features(fake, np.zeros((3, 5, 3000), np.float32))
    with pytest.raises(ValueError):
        q2a.Engine.encode_features(fake, x, mask[:, :100])


def test_window_rule_equals_the_oracles_window():
    """mel_cases.mel_window (zeros from frame n_len on, frame by frame) equals oracle_py.Oracle.mel_window (the
    reference's memset + copy of [i0, i1) with the seek clamped to n_len) on ragged n_len and seek."""
    rng = np.random.default_rng(7)
    o = types.SimpleNamespace(m=types.SimpleNamespace(n_ctx=T))   # mel_window reads n_ctx alone
    for n_len, seek in mc.RAGGED:
        ld = n_len + 5
        mel = rng.standard_normal((6, ld)).astype(np.float32)
        got = mc.mel_window(mel, n_len, seek)
        want = oracle_py.Oracle.mel_window(o, mel[:, :n_len], seek)
        assert got.shape == want.shape == (6, mc.TM)
        assert np.array_equal(got, want), (n_len, seek)
        live = max(0, min(n_len - seek, mc.TM))
        assert not got[:, live:].any() and (live == 0 or got[:, :live].any())


def test_poisoned_layout_ends_with_the_last_readable_float():
    mels = [np.ones((3, n), np.float32) for n in (5, 2)]
    buf = mc.poisoned(mels, [5, 2], ld=6)
    assert buf.size == 3 * 6 + 2 * 6 + 2 and buf[-1] == 1.0
    rows = buf[:18].reshape(3, 6)
    assert (rows[:, :5] == 1).all() and np.isnan(rows[:, 5]).all()
    assert np.isnan(buf[18 + 2:18 + 6]).all() and (buf[18:20] == 1).all()
