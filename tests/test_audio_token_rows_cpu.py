"""CPU checks of the host side of the inputs_embeds calls (include/q2a_encoder.h): the row map q2a_audio_token_rows through
lib/libq2a_host.so (no GPU, no HIP runtime) and q2a.audio_token_rows against numpy.flatnonzero, and the argument errors
of Engine.inputs_embeds that are raised before anything touches a device."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import q2a
from conftest import PKG, ROOT

ERR_ARG = -4
FILL = -7
AUDIO = 151646
i32p = C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def host_lib(host_build):
    L = C.CDLL(os.path.join(PKG, "lib", "libq2a_host.so"))
    L.q2a_audio_token_rows.restype = C.c_int64
    L.q2a_audio_token_rows.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, i32p, C.c_int64]
    return L


def _ids(n, pattern, dtype, seed=5):
    """n ids of `dtype`, text ids 0 .. 999 with the audio id at the pattern's positions."""
    rng = np.random.default_rng(seed + n)
    ids = rng.integers(0, 1000, size=n).astype(dtype)
    if pattern == "all":
        ids[:] = AUDIO
    elif pattern == "first":
        ids[0] = AUDIO
    elif pattern == "last":
        ids[-1] = AUDIO
    elif pattern == "bernoulli":
        ids[rng.random(n) < 0.3] = AUDIO
    else:
        assert pattern == "none"
    return ids


def _call(L, ids, audio, map_cap, room=3):
    """q2a_audio_token_rows into a map of map_cap words with `room` filled words behind them -> (count, whole buffer)."""
    rm = np.full(map_cap + room, FILL, dtype=np.int32)
    n = L.q2a_audio_token_rows(ids.ctypes.data_as(C.c_void_p), ids.itemsize, ids.size, audio, rm.ctypes.data_as(i32p), map_cap)
    return n, rm


@pytest.mark.parametrize("dtype", [np.int32, np.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("pattern", ["none", "all", "first", "last", "bernoulli"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2048, 2049, 70001])
def test_host_twin_against_flatnonzero(host_lib, n, pattern, dtype):
    ids = _ids(n, pattern, dtype)
    want = np.flatnonzero(ids == AUDIO).astype(np.int32)
    # map_cap below, at and above the count: the first map_cap positions, then -1, and nothing behind map_cap
    for cap in sorted({0, max(len(want) - 1, 0), len(want), len(want) + 1, len(want) + 5}):
        count, rm = _call(host_lib, ids, AUDIO, cap)
        assert count == len(want), (n, pattern, cap)
        k = min(cap, len(want))
        assert np.array_equal(rm[:k], want[:k])
        assert np.all(rm[k:cap] == -1)
        assert np.all(rm[cap:] == FILL), "words behind map_cap were written"


def test_int64_ids_are_compared_on_all_64_bits(host_lib):
    ids = np.full(300, 7, dtype=np.int64)
    ids[[3, 64, 299]] = AUDIO
    ids[[4, 65, 128]] = AUDIO + (1 << 32)          # the low word alone equals the audio id
    ids[[5, 200]] = AUDIO - (1 << 32)
    ids[6] = AUDIO - (1 << 63)                     # the sign bit set above the same low word
    assert np.all((ids[[4, 65, 128, 5, 200, 6]] & 0xFFFFFFFF) == AUDIO)
    count, rm = _call(host_lib, ids, AUDIO, 5)
    assert count == 3 and list(rm[:5]) == [3, 64, 299, -1, -1]
    # and an audio id that only an int64 holds
    big = AUDIO + (1 << 40)
    ids[[10, 11]] = big
    count, rm = _call(host_lib, ids, big, 2)
    assert count == 2 and list(rm[:2]) == [10, 11]
    # an int32 array never matches it
    count, _ = _call(host_lib, np.full(50, AUDIO, dtype=np.int32), big, 2)
    assert count == 0
    # negative ids
    neg = np.array([-1, 5, -1, -2], dtype=np.int32)
    count, rm = _call(host_lib, neg, -1, 4)
    assert count == 2 and list(rm[:4]) == [0, 2, -1, -1]


def test_host_twin_argument_errors_write_nothing(host_lib):
    ids = _ids(100, "bernoulli", np.int64)
    rm = np.full(8, FILL, dtype=np.int32)
    p, q = ids.ctypes.data_as(C.c_void_p), rm.ctypes.data_as(i32p)
    f = host_lib.q2a_audio_token_rows
    assert f(p, 2, 100, AUDIO, q, 8) == ERR_ARG          # width
    assert f(p, 8, -1, AUDIO, q, 8) == ERR_ARG           # n_tokens
    assert f(p, 8, 2 ** 31, AUDIO, q, 8) == ERR_ARG
    assert f(None, 8, 100, AUDIO, q, 8) == ERR_ARG       # no ids
    assert f(p, 8, 100, AUDIO, q, -1) == ERR_ARG         # map_cap
    assert f(p, 8, 100, AUDIO, None, 8) == ERR_ARG       # no map for a positive map_cap
    assert np.all(rm == FILL)
    # the count alone: no map, map_cap 0; no tokens at all
    assert f(p, 8, 100, AUDIO, None, 0) == int((ids == AUDIO).sum())
    assert f(None, 8, 0, AUDIO, q, 2) == 0 and list(rm[:3]) == [-1, -1, FILL]


def test_python_audio_token_rows(host_build):
    ids = _ids(2 * 777, "bernoulli", np.int64).reshape(2, 777)
    want = np.flatnonzero(ids.reshape(-1) == AUDIO)
    n, rm = q2a.audio_token_rows(ids, AUDIO)
    assert n == len(want) and rm.dtype == np.int32 and np.array_equal(rm, want)
    n, rm = q2a.audio_token_rows(ids.astype(np.int32), AUDIO, map_cap=len(want) + 3)
    assert n == len(want) and np.array_equal(rm[:n], want) and list(rm[n:]) == [-1, -1, -1]
    n, rm = q2a.audio_token_rows(ids, AUDIO, map_cap=2)
    assert n == len(want) and np.array_equal(rm, want[:2])
    # a non-contiguous view is read in its own row-major order
    n, rm = q2a.audio_token_rows(ids[:, ::2], AUDIO)
    assert np.array_equal(rm, np.flatnonzero(ids[:, ::2].reshape(-1) == AUDIO))
    # it agrees with audio_token_runs wherever the tokens form runs
    runs = np.full((2, 50), 3, dtype=np.int64)
    runs[0, 4:9] = AUDIO
    runs[1, 45:] = AUDIO
    starts, lens = q2a.audio_token_runs(runs, AUDIO)
    n, rm = q2a.audio_token_rows(runs, AUDIO)
    assert np.array_equal(rm, np.concatenate([s + np.arange(k) for s, k in zip(starts, lens)]))
    with pytest.raises(ValueError):
        q2a.audio_token_rows(ids.astype(np.int16), AUDIO)
    with pytest.raises(ValueError):
        q2a.audio_token_rows(ids, AUDIO, map_cap=-1)


def test_inputs_embeds_argument_errors_need_no_gpu():
    """Everything Engine.inputs_embeds rejects before it touches a device: no engine handle or projector handle is read."""
    torch = pytest.importorskip("torch")
    eng = object.__new__(q2a.Engine)             # no library handle: a call that got past the checks would fail loudly
    proj = types.SimpleNamespace(d_out=256, h=None)
    ids = torch.zeros((2, 8), dtype=torch.int64)                     # a CPU tensor
    feats = torch.zeros((1, 128, 3000))
    with pytest.raises(ValueError, match="projector"):
        q2a.Engine.inputs_embeds(eng, feats, None, ids, AUDIO, None)
    for bad in (ids, ids.numpy(), [[1, 2]], None):
        with pytest.raises(ValueError, match="input_ids"):
            q2a.Engine.inputs_embeds(eng, feats, None, bad, AUDIO, proj)


@pytest.mark.parametrize("pattern,loads", [(r"k_ids_count", 8), (r"k_ids_place", 8), (r"k_embed_gather", 4)])
def test_new_kernels_issue_their_loads_together(tmp_path, pattern, loads):
    """tests/test_isa_loads.py's check on csrc/q2a_embeds.hip: the eight id loads of a wave and the four 16-byte loads
    of a gathered row go out before the first wait — no global load is followed at once by s_waitcnt vmcnt(0)."""
    from test_isa_loads import _disasm, _pick, _serial_loads
    stats = _serial_loads(_disasm("q2a_embeds.o", tmp_path))
    ks = _pick(stats, pattern)
    assert len(ks) == 2, ks                       # the int32 and the int64 instantiation
    for k in ks:
        n, serial = stats[k]
        assert n >= loads and serial == 0, (k, n, serial)


def test_exports_and_header_agree():
    src = open(os.path.join(ROOT, "include", "q2a_encoder.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("q2a_audio_token_rows", "q2a_projector_apply_ids", "q2a_inputs_embeds_device", "q2a_inputs_embeds_device_mel",
                 "q2a_test_audio_token_rows", "q2a_test_embed_gather"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in q2a.EXPORTS, name
    # the struct the Python mirror passes has the header's layout: 64 bytes
    assert C.sizeof(q2a.EmbedsSrc) == 64
    assert [f[0] for f in q2a.EmbedsSrc._fields_] == ["input_ids", "ids_width", "reserved", "n_tokens", "audio_token_id",
                                                     "embed_table", "vocab", "table_ld", "report_dev"]
