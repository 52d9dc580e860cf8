"""CPU checks of the host side of the audio-feature _to calls (include/q2a_encoder.h): the destination rows
q2a_feat_rows through lib/libq2a_host.so (no GPU, no HIP runtime) and q2a.feat_rows against a numpy restatement, and
q2a.audio_token_runs, which finds the clips' first rows in input_ids."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import q2a
from conftest import PKG, ROOT

ERR_ARG = -4
FILL = -7
i32p = C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def host_lib(host_build):
    L = C.CDLL(os.path.join(PKG, "lib", "libq2a_host.so"))
    L.q2a_feat_rows.restype = C.c_int64
    L.q2a_feat_rows.argtypes = [i32p, i32p, C.c_int, C.c_int64, i32p]
    return L


def _rows(L, out_len, clip_row, n_rows, want_map=True):
    ol = np.ascontiguousarray(out_len, dtype=np.int32)
    cr = None if clip_row is None else np.ascontiguousarray(clip_row, dtype=np.int32)
    rm = np.full(max(int(np.maximum(ol, 0).sum()), 0) + 4, FILL, dtype=np.int32)
    n = L.q2a_feat_rows(ol.ctypes.data_as(i32p), cr.ctypes.data_as(i32p) if cr is not None else None, len(ol), n_rows,
                        rm.ctypes.data_as(i32p) if want_map else None)
    return n, rm


def _want(out_len, clip_row):
    """The restatement: clip after clip, out_len[c] consecutive rows from clip_row[c] (packed: from the running total)."""
    rows, tot = [], 0
    for c, n in enumerate(out_len):
        start = tot if clip_row is None else clip_row[c]
        rows += [start + j for j in range(n)]
        tot += n
    return np.asarray(rows, dtype=np.int32)


def _good_cases():
    ol = [0, 1, 1, 7, 8, 8, 0, 15, 16, 182, 740, 744, 750]
    # reverse clip order with 3-row gaps (the GPU test's layout); the clips without rows point anywhere
    starts, at = [0] * len(ol), 5
    for c in reversed(range(len(ol))):
        starts[c] = at
        at += ol[c] + 3
    starts[0], starts[6] = -100, 10 ** 9
    yield ol, starts, at
    yield ol, None, sum(ol)                       # packed, exactly full
    yield ol, None, sum(ol) + 11
    yield [3, 2], [2, 5], 7                       # touching ranges, the last one ends at n_rows
    yield [3, 2], [5, 0], 8                       # a gap, clip order reversed
    yield [0, 0], [4, 4], 0                       # nothing to place, n_rows 0
    yield [4], [0], 4
    rng = np.random.default_rng(5)
    ol = rng.integers(0, 40, size=64).tolist()    # a random permutation of the clips with random gaps
    starts, at = [0] * 64, 0
    for c in rng.permutation(64):
        at += int(rng.integers(0, 4))
        starts[c] = at
        at += ol[c]
    yield ol, starts, at + 2


def test_feat_rows_host_library(host_lib):
    for ol, cr, n_rows in _good_cases():
        n, rm = _rows(host_lib, ol, cr, n_rows)
        want = _want(ol, cr)
        assert n == sum(ol) == len(want), (ol, cr)
        assert np.array_equal(rm[:n], want), (ol, cr)
        assert (rm[n:] == FILL).all(), "entries behind N_tot were written"
        assert len(set(want.tolist())) == n and ((want >= 0) & (want < n_rows)).all(), "the case itself is valid"
        assert _rows(host_lib, ol, cr, n_rows, want_map=False)[0] == n   # row_map may be NULL


def test_feat_rows_python(host_build):
    for ol, cr, n_rows in _good_cases():
        n, rm = q2a.feat_rows(ol, cr, n_rows)
        assert n == sum(ol) and rm.dtype == np.int32 and np.array_equal(rm, _want(ol, cr)), (ol, cr)
    own = np.full(6, FILL, dtype=np.int32)
    n, rm = q2a.feat_rows([2, 0, 3], [9, 1, 4], 11, row_map=own)
    assert n == 5 and rm is own and list(own) == [9, 10, 4, 5, 6, FILL]
    n, rm = q2a.feat_rows([], None, 0)
    assert n == 0 and len(rm) == 0


BAD = [
    ([3, 2], [-1, 5], 10, "a negative start"),
    ([3, 2], [0, -2147483648], 10, "a negative start"),
    ([3, 2], [0, 9], 10, "a range past n_rows"),
    ([3, 2], [8, 0], 10, "a range past n_rows"),
    ([3, 2], None, 4, "packed rows past n_rows"),
    ([3, 2], [0, 2147483647], 1 << 40, "a range past the int32 rows"),
    ([3, 2], [0, 2], 10, "an overlap of one row"),
    ([3, 2], [4, 4], 10, "the same start"),
    ([5, 1, 2], [0, 2, 8], 10, "a range inside another"),
    ([2, 0, 2, 3], [6, 0, 0, 1], 10, "an overlap of clips that are not neighbours in row order"),
    ([3, -1], [0, 5], 10, "a negative length"),
    ([3, 2], [0, 5], -1, "negative n_rows"),
]


@pytest.mark.parametrize("ol,cr,n_rows,why", BAD, ids=[b[3] for b in BAD])
def test_feat_rows_rejects(host_lib, ol, cr, n_rows, why):
    n, rm = _rows(host_lib, ol, cr, n_rows)
    assert n == ERR_ARG, why
    assert (rm == FILL).all(), "nothing is written to the map on an error"
    own = np.full(16, FILL, dtype=np.int32)
    with pytest.raises(q2a.Q2AError) as ei:
        q2a.feat_rows(ol, cr, n_rows, row_map=own)
    assert ei.value.rc == ERR_ARG and (own == FILL).all()


def test_feat_rows_bad_calls(host_lib):
    ol = np.array([2], dtype=np.int32)
    assert host_lib.q2a_feat_rows(ol.ctypes.data_as(i32p), None, -1, 10, None) == ERR_ARG
    assert host_lib.q2a_feat_rows(None, None, 1, 10, None) == ERR_ARG
    assert host_lib.q2a_feat_rows(None, None, 0, 10, None) == 0
    with pytest.raises(ValueError):
        q2a.feat_rows([1, 2], [0], 10)


# ---------------------------------------------------------------- audio_token_runs
AUDIO = 151646


def _runs_ref(ids, tok):
    starts, lens = [], []
    B, S = ids.shape
    for b in range(B):
        s = 0
        while s < S:
            if ids[b, s] == tok:
                e = s
                while e < S and ids[b, e] == tok:
                    e += 1
                starts.append(b * S + s)
                lens.append(e - s)
                s = e
            else:
                s += 1
    return starts, lens


def test_audio_token_runs():
    S = 12
    ids = np.full((2, S), 7, dtype=np.int64)
    ids[0, 3:8] = AUDIO                      # one run
    ids[1, 0:2] = AUDIO                      # two runs: one at the start of the sequence ...
    ids[1, 9:12] = AUDIO                     # ... one touching its end
    starts, lens = q2a.audio_token_runs(ids, AUDIO)
    assert list(starts) == [3, S + 0, S + 9] and list(lens) == [5, 2, 3]
    assert (list(starts), list(lens)) == _runs_ref(ids, AUDIO)
    # a run that ends a sequence and one that begins the next stay two runs
    ids2 = np.full((2, 6), 1, dtype=np.int32)
    ids2[0, 4:] = AUDIO
    ids2[1, :3] = AUDIO
    starts, lens = q2a.audio_token_runs(ids2, AUDIO)
    assert list(starts) == [4, 6] and list(lens) == [2, 3]
    # no run at all; a whole sequence of audio tokens
    starts, lens = q2a.audio_token_runs(np.zeros((3, 5), dtype=np.int64), AUDIO)
    assert len(starts) == 0 and len(lens) == 0
    starts, lens = q2a.audio_token_runs(np.full((1, 5), AUDIO), AUDIO)
    assert list(starts) == [0] and list(lens) == [5]
    rng = np.random.default_rng(3)
    ids3 = np.where(rng.random((5, 37)) < 0.5, AUDIO, 9)
    starts, lens = q2a.audio_token_runs(ids3, AUDIO)
    assert (list(starts), list(lens)) == _runs_ref(ids3, AUDIO)
    with pytest.raises(ValueError):
        q2a.audio_token_runs(np.zeros(5, dtype=np.int64), AUDIO)


def test_runs_feed_feat_rows(host_build):
    """The hand-off: the runs of input_ids, checked against out_len, are the clip_rows of the call."""
    ids = np.full((2, 20), 7, dtype=np.int64)
    ids[0, 2:9] = AUDIO
    ids[1, 1:4] = AUDIO
    ids[1, 10:20] = AUDIO
    starts, lens = q2a.audio_token_runs(ids, AUDIO)
    out_len = [7, 3, 10]
    assert list(lens) == out_len
    n, rm = q2a.feat_rows(out_len, starts, ids.size)
    assert n == 20 and np.array_equal(rm, np.flatnonzero(ids.reshape(-1) == AUDIO))


# ---------------------------------------------------------------- the ABI
NEW_ENTRY_POINTS = ("q2a_feat_rows", "q2a_projector_apply_to", "q2a_projector_regime", "q2a_audio_features_device_to",
                    "q2a_audio_features_device_mel_to")


def test_new_entry_points_are_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "q2a_encoder.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = q2a.lib()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared"
        assert hasattr(L, name), f"{name} is not exported"
        assert name in q2a.EXPORTS
    for name in ("audio_features_device_to", "audio_features_device_mel_to"):
        assert callable(getattr(q2a.Engine, name)), name
    assert callable(q2a.Projector.apply_to) and callable(q2a.Projector.regime)
    assert callable(q2a.feat_rows) and callable(q2a.audio_token_runs)
    assert (q2a.DT_F32, q2a.DT_F16, q2a.DT_BF16) == (0, 1, 2)
    assert C.sizeof(q2a.FeatDst) == 32


def test_new_entry_points_fail_cleanly_without_a_handle():
    """Without a HIP device nothing can be opened; the entry points answer NULL handles with an error code before
    touching the device or the caller's arrays."""
    L = q2a.lib()
    kl = (C.c_int32 * 1)(100)
    ns = (C.c_int32 * 1)(160000)
    st = (C.c_int32 * 1)(-1)
    ol = (C.c_int32 * 1)(-1)
    dst = q2a.feat_dst(0, 512, 10, q2a.DT_BF16)
    assert L.q2a_audio_features_device_to(None, None, None, 0, ns, None, kl, 1, C.byref(dst), None, None, 0, ol, st, None) == ERR_ARG
    assert L.q2a_audio_features_device_mel_to(None, None, None, 0, 3000, ns, None, kl, 1, C.byref(dst), None, None, 0, ol, st,
                                              None) == ERR_ARG
    assert L.q2a_projector_apply_to(None, None, 4, C.byref(dst), None, None) == ERR_ARG
    assert L.q2a_projector_regime(None, 4) == ERR_ARG
    assert st[0] == -1 and ol[0] == -1 and kl[0] == 100
