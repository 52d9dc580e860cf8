"""Encode from log-mel features on the GPU: the ingest kernel (q2a_exact.hip, k_mel_ingest) through
q2a_test_frontend_mel, the entry points q2a_encode_device_mel / q2a_encode_host_mel, whisper_set_mel + whisper_encode /
whisper_full, bin/q2a_main -mel and Engine.encode_features.

Everything behind the mel is the PCM entry points' path, so wherever the PCM path can produce the same input
(mel = q2a_pcm_to_mel(pcm), seek = offset_ms / 10) the comparison is exact, bit for bit. Where it cannot (frames past
n_len are zeros, not the PCM padding's value) the CPU oracle on the reference's own window is the yardstick.
All tests need an MI355X."""
import ctypes as C
import os
import subprocess
import wave

import numpy as np
import pytest

import mel_cases as mc
import oracle_py
from conftest import PKG, rel_errors

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

T, TM = mc.N_CTX, mc.TM
SENTINEL_ROWS, SENTINEL = 8, 7.0
MAIN = os.path.join(PKG, "bin", "q2a_main")
TOOL = os.path.join(PKG, "bin", "q2a_tool")
i32p = C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def engines(make_model):
    import q2a
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    cache = {}

    def get(cfg, wt, act=0):
        if (cfg, wt, act) not in cache:
            cache[(cfg, wt, act)] = q2a.Engine(make_model(cfg, wt), device=0, act=act)
        return cache[(cfg, wt, act)]

    yield get
    for e in cache.values():
        e.close()


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _pcm_batch(clips):
    stride = max(len(c) for c in clips)
    pcm = torch.zeros(len(clips), stride)
    for i, c in enumerate(clips):
        pcm[i, :len(c)] = torch.from_numpy(np.ascontiguousarray(c))
    return pcm.cuda(), stride, [len(c) for c in clips]


def _mel_batch(mels, pad=3, fill=float("nan")):
    """[B][n_mels][ld] on the device, ld = the longest n_len + pad (not a multiple of 4 for the clips used here), `fill`
    in every frame at or past a clip's n_len."""
    n_lens = [m.shape[1] for m in mels]
    ld = max(n_lens) + pad
    buf = np.full((len(mels), mels[0].shape[0], ld), fill, dtype=np.float32)
    for c, m in enumerate(mels):
        buf[c, :, :m.shape[1]] = m
    return torch.from_numpy(buf).cuda(), ld, n_lens


def _frontend_pcm(e, clips):
    pcm, stride, ns = _pcm_batch(clips)
    x = torch.full((len(clips) * T, e.info.n_audio_state), float("nan"), device="cuda")
    e.test_frontend(pcm.data_ptr(), stride, ns, x.data_ptr())
    torch.cuda.synchronize()
    return x


def _frontend_mel(e, buf_ptr, clip_stride, ld, n_lens, seek=None):
    """q2a_test_frontend_mel into a NaN buffer (every row must be written) with sentinel rows behind it (kept)."""
    rows = len(n_lens) * T
    x = torch.full((rows + SENTINEL_ROWS, e.info.n_audio_state), float("nan"), device="cuda")
    x[rows:] = SENTINEL
    e.test_frontend_mel(buf_ptr, clip_stride, ld, n_lens, x.data_ptr(), seek=seek)
    torch.cuda.synchronize()
    assert (x[rows:] == SENTINEL).all(), "rows behind X were written"
    return x[:rows]


def _encode_pcm(e, kind, clips, offsets_ms, key_len=None):
    """The PCM entry point of `kind` on device buffers -> (out, out_len, status); out starts as NaN."""
    import q2a
    pcm, stride, ns = _pcm_batch(clips)
    n = len(clips)
    out = torch.full((n,) + e.out_shape, float("nan"), device="cuda")
    if kind == q2a.ENCODE_PLAIN:
        nsa, offs, st = (np.ascontiguousarray(a, dtype=np.int32) for a in (ns, offsets_ms, np.full(n, -1)))
        rc = q2a.lib().q2a_encode_device_ex(C.c_void_p(e.h), C.c_void_p(pcm.data_ptr()), C.c_int64(stride),
                                            nsa.ctypes.data_as(i32p), offs.ctypes.data_as(i32p), n,
                                            C.c_void_p(out.data_ptr()), st.ctypes.data_as(i32p), None)
        assert rc == 0, q2a.lib().q2a_last_error()
        ol = np.zeros(n, dtype=np.int32)
    else:
        f = e.encode_device_padded if kind == q2a.ENCODE_PADDED else e.encode_device_varlen
        ol, st = f(pcm.data_ptr(), stride, ns, out.data_ptr(), offsets_ms=offsets_ms, key_len=key_len)
    torch.cuda.synchronize()
    return out, ol, st


def _encode_mel(e, kind, mels, seek=None, key_len=None):
    buf, ld, n_lens = _mel_batch(mels)
    out = torch.full((len(mels),) + e.out_shape, float("nan"), device="cuda")
    ol, st = e.encode_device_mel(buf.data_ptr(), buf.shape[1] * ld, ld, n_lens, out.data_ptr(), kind=kind, seek=seek,
                                 key_len=key_len)
    torch.cuda.synchronize()
    return out, ol, st


@pytest.fixture(scope="module")
def clips3(make_clip):
    """30 s, 17.3 s and 12 s: three n_len (6000, 4730, 4200), each with more than 1 s behind a 10.01 s offset."""
    return [make_clip(0, 480000), make_clip(2, 276800), make_clip(1, 192000)]


# ---------------------------------------------------------------- 1. kernel bits
@pytest.mark.parametrize("cfg,wt", [("tiny", "f16"), ("tiny", "f32"), ("full", "q4_k")])
def test_frontend_mel_equals_the_pcm_frontend_bits(engines, clips3, cfg, wt):
    """Three clips of different lengths in one launch, ld = the longest n_len + 3: the first block's input from
    q2a_pcm_to_mel's frames equals the PCM front end's, bit for bit (hi | mid | lo for the F16 conv kernels, hi | lo | hi
    for the all-F32 file, the 128-mel x D = 1280 conv shapes on the full-size engine with two clips). At the odd seek
    1001 (10 010 ms), where the PCM front-end hook has no offset, the whole plain encode is compared instead."""
    import q2a
    e = engines(cfg, wt)
    clips = clips3[:2] if cfg == "full" else clips3
    mels = [e.pcm_to_mel(c) for c in clips]
    assert [m.shape[1] for m in mels] == [6000, 4730, 4200][:len(clips)]
    buf, ld, n_lens = _mel_batch(mels)
    assert ld == 6003 and ld % 4 != 0
    want = _frontend_pcm(e, clips)
    got = _frontend_mel(e, buf.data_ptr(), buf.shape[1] * ld, ld, n_lens)
    assert torch.isfinite(got).all()
    assert _same_bits(got, want)
    # seek NULL is seek 0
    assert _same_bits(_frontend_mel(e, buf.data_ptr(), buf.shape[1] * ld, ld, n_lens, seek=[0] * len(clips)), want)
    for off in (0, 10010):
        pout, _, pst = _encode_pcm(e, q2a.ENCODE_PLAIN, clips, [off] * len(clips))
        mout, _, mst = _encode_mel(e, q2a.ENCODE_PLAIN, mels, seek=[off // 10] * len(clips))
        assert list(pst) == list(mst) == [q2a.CLIP_ENCODED] * len(clips)
        assert torch.isfinite(mout).all()
        assert _same_bits(mout, pout), off


def test_one_recording_three_seeks_equals_encode_device_ex(engines, make_clip):
    """clip_stride 0: three windows of one 75 s recording's mel (seeks 0, 3000 and the odd 1001) against
    q2a_encode_device_ex on the recording's PCM with pcm_stride 0."""
    import q2a
    e = engines("tiny", "f16")
    rec = make_clip(2, 75 * 16000)
    offs = [0, 30000, 10010]
    pcm = torch.from_numpy(rec).cuda()
    want = torch.full((3,) + e.out_shape, float("nan"), device="cuda")
    ns, oa, st = (np.ascontiguousarray(a, dtype=np.int32) for a in ([len(rec)] * 3, offs, [-1] * 3))
    rc = q2a.lib().q2a_encode_device_ex(C.c_void_p(e.h), C.c_void_p(pcm.data_ptr()), C.c_int64(0), ns.ctypes.data_as(i32p),
                                        oa.ctypes.data_as(i32p), 3, C.c_void_p(want.data_ptr()), st.ctypes.data_as(i32p), None)
    assert rc == 0 and list(st) == [q2a.CLIP_ENCODED] * 3
    mel = e.pcm_to_mel(rec)
    n_len = mel.shape[1]
    assert n_len == 10500
    buf = torch.from_numpy(mel).cuda()
    got = torch.full_like(want, float("nan"))
    _, mst = e.encode_device_mel(buf.data_ptr(), 0, n_len, [n_len] * 3, got.data_ptr(), seek=[o // 10 for o in offs])
    torch.cuda.synchronize()
    assert list(mst) == [q2a.CLIP_ENCODED] * 3
    assert _same_bits(got, want)
    assert not _same_bits(got[0], got[2])
    x = _frontend_mel(e, buf.data_ptr(), 0, n_len, [n_len] * 3, seek=[0, 0, 1001])
    assert _same_bits(x[:T], x[T:2 * T]) and not _same_bits(x[:T], x[2 * T:])


# ---------------------------------------------------------------- 2. zeros and bounds
def test_frames_past_n_len_are_zeros_and_never_read(engines):
    """mel_cases.EDGE_CLIPS in one launch, from a buffer that ends with the last clip's last readable float and holds NaN
    in every frame at or past n_len[c] of every row: X is finite, equal to the run on a zero-filled buffer with
    n_len = ld, and equal to the run on the explicit windows of mel_cases.mel_window (n_len 3000, seek 0)."""
    e = engines("tiny", "f16")
    M = e.info.n_mels
    rng = np.random.default_rng(11)
    n_lens, seeks = [c[0] for c in mc.EDGE_CLIPS], [c[1] for c in mc.EDGE_CLIPS]
    assert set(n_lens) == {1, 63, 64, 65, 777, 2999, 3000}
    assert {n - s for n, s in mc.EDGE_CLIPS} >= {63, 64, 65}
    mels = [rng.uniform(-1.0, 1.5, size=(M, n)).astype(np.float32) for n in n_lens]
    ld = 3003
    stride, total = mc.layout(n_lens, M, ld)
    flat = mc.poisoned(mels, n_lens, ld)
    assert flat.size == total and np.isnan(flat).sum() > 0 and np.isfinite(flat[-1])
    buf = torch.from_numpy(flat).cuda()
    got = _frontend_mel(e, buf.data_ptr(), stride, ld, n_lens, seek=seeks)
    assert torch.isfinite(got).all(), "a frame at or past n_len was read"
    zeros, zld, _ = _mel_batch(mels, pad=ld - max(n_lens), fill=0.0)   # the whole [B][M][ld], zeros behind every clip
    assert zld == ld and zeros.numel() == len(n_lens) * stride
    want = _frontend_mel(e, zeros.data_ptr(), stride, ld, [ld] * len(n_lens), seek=seeks)
    assert _same_bits(got, want)
    wins = torch.from_numpy(np.stack([mc.mel_window(m, n, s) for m, n, s in zip(mels, n_lens, seeks)])).cuda()
    ref = _frontend_mel(e, wins.data_ptr(), M * TM, TM, [TM] * len(n_lens))
    assert _same_bits(got, ref)
    # the windows differ from one another, and the all-zero window (seek behind the last frame) is the zero input's X
    assert not _same_bits(got[:T], got[T:2 * T])
    z = torch.zeros(1, M, TM, device="cuda")
    assert _same_bits(got[-T:], _frontend_mel(e, z.data_ptr(), M * TM, TM, [TM]))


# ---------------------------------------------------------------- 3. entry points, exact
@pytest.fixture(scope="module")
def batch(make_clip):
    """30 s, 7.3 s and 1.2 s, encoded from 0, 1 s and 0.1 s."""
    return [make_clip(0, 480000), make_clip(2, 116800), make_clip(1, 19200)], [0, 1000, 100], [1500, 365, 37]


@pytest.mark.parametrize("wt", ["f16", "q4_k", "q8_0"])
def test_mel_entry_points_equal_the_pcm_entry_points_bytes(engines, batch, wt):
    import q2a
    e = engines("tiny", wt)
    clips, offs, lens = batch
    mels = [e.pcm_to_mel(c) for c in clips]
    seeks = [o // 10 for o in offs]
    for kind in (q2a.ENCODE_PLAIN, q2a.ENCODE_PADDED, q2a.ENCODE_VARLEN):
        want, wol, wst = _encode_pcm(e, kind, clips, offs, key_len=lens)
        got, ol, st = _encode_mel(e, kind, mels, seek=seeks, key_len=lens)
        assert list(st) == list(wst) == [q2a.CLIP_ENCODED] * 3, kind
        assert list(ol) == list(wol), kind
        assert kind == q2a.ENCODE_PLAIN or list(ol) == [750, 182, 18]
        assert not torch.isnan(got).any(), "the whole output buffer is written"
        assert _same_bits(got, want), kind
        hout, hol, hst = e.encode_host_mel(mels, kind=kind, seek=seeks, key_len=lens,
                                           out=np.full((3,) + e.out_shape, np.nan, dtype=np.float32))
        assert list(hol) == list(ol) and list(hst) == list(st), kind
        assert np.array_equal(hout.view(np.int32), got.cpu().numpy().view(np.int32)), kind


def test_bf16_contract_plain_only(engines, batch):
    import q2a
    eb = engines("tiny", "f16", q2a.ACT_BF16)
    clips, offs, lens = batch
    mels = [eb.pcm_to_mel(c) for c in clips]
    seeks = [o // 10 for o in offs]
    want, _, _ = _encode_pcm(eb, q2a.ENCODE_PLAIN, clips, offs)
    got, _, st = _encode_mel(eb, q2a.ENCODE_PLAIN, mels, seek=seeks)
    assert list(st) == [q2a.CLIP_ENCODED] * 3 and _same_bits(got, want)
    hout, _, _ = eb.encode_host_mel(mels, seek=seeks)
    assert np.array_equal(hout.view(np.int32), want.cpu().numpy().view(np.int32))
    buf, ld, n_lens = _mel_batch(mels)
    for kind in (q2a.ENCODE_PADDED, q2a.ENCODE_VARLEN):
        out = torch.full((3,) + eb.out_shape, 7.0, device="cuda")
        with pytest.raises(q2a.Q2AError) as ei:
            eb.encode_device_mel(buf.data_ptr(), buf.shape[1] * ld, ld, n_lens, out.data_ptr(), kind=kind, key_len=lens)
        assert ei.value.rc == -6
        hout = np.full((3,) + eb.out_shape, 7.0, dtype=np.float32)
        with pytest.raises(q2a.Q2AError) as ei:
            eb.encode_host_mel(mels, kind=kind, out=hout)
        assert ei.value.rc == -6
        torch.cuda.synchronize()
        assert (out == 7.0).all() and (hout == 7.0).all()


# ---------------------------------------------------------------- 4. the reference's semantics, where the PCM path cannot go
def test_truncated_mel_matches_the_oracle_on_the_reference_window(engines, make_model, make_clip):
    """Tiny F16, the oracle's log-mel of clip 1 cut to n_len 777, seek 100: window frames 677 .. 2999 are zeros, which no
    PCM input produces. Against Oracle.encode(Oracle.mel_window(mel[:, :777], 100)) over the full output, at the
    project's bar for this comparison (max_rel < 1e-3, rel_l2 < 1e-4, test_encoder_tiny_matches_oracle_intermediate_free).
    Measured on an MI355X: max_rel 5.08e-05, rel_l2 1.59e-05."""
    import q2a
    from q2a import ggmlfile
    e = engines("tiny", "f16")
    o = oracle_py.Oracle(ggmlfile.read(make_model("tiny", "f16")))
    mel = np.ascontiguousarray(o.log_mel(make_clip(1))[:, :777])
    ref = o.encode(o.mel_window(mel, 100))
    out, _, st = e.encode_host_mel([mel], seek=[100])
    assert list(st) == [q2a.CLIP_ENCODED]
    mx, l2 = rel_errors(out[0], ref)
    print(f"mel 777 @ 100 vs oracle: max_rel {mx:.3e} rel_l2 {l2:.3e}")
    assert mx < 1e-3 and l2 < 1e-4, (mx, l2)
    # derived key lengths (NULL): out_len is q2a_mel_valid_lengths', rows from it on are zeros
    enc, n_out = q2a.mel_valid_lengths(777, 100)
    assert (enc, n_out) == (339, 169)
    explicit, _, _ = e.encode_host_mel([mel], kind=q2a.ENCODE_PADDED, seek=[100], key_len=[enc])
    for kind in (q2a.ENCODE_PADDED, q2a.ENCODE_VARLEN):
        got, ol, st = e.encode_host_mel([mel], kind=kind, seek=[100], out=np.full((1,) + e.out_shape, np.nan, dtype=np.float32))
        assert list(ol) == [n_out] and list(st) == [q2a.CLIP_ENCODED]
        assert np.isfinite(got).all() and got[0, :n_out].any() and not got[0, n_out:].any()
        assert np.array_equal(got.view(np.int32), explicit.view(np.int32))
        buf = torch.from_numpy(mel).cuda()
        dout = torch.full((1,) + e.out_shape, float("nan"), device="cuda")
        dol, _ = e.encode_device_mel(buf.data_ptr(), 0, 777, [777], dout.data_ptr(), kind=kind, seek=[100])
        torch.cuda.synchronize()
        assert list(dol) == [n_out]
        assert np.array_equal(dout.cpu().numpy().view(np.int32), got.view(np.int32))


# ---------------------------------------------------------------- 5. whisper API
class FullParams(C.Structure):
    """struct whisper_full_params (include/q2a_whisper.h)."""
    _fields_ = ([("strategy", C.c_int), ("n_threads", C.c_int), ("n_max_text_ctx", C.c_int), ("offset_ms", C.c_int),
                 ("duration_ms", C.c_int)] + [(f"flag{i}", C.c_bool) for i in range(9)] +
                [("thold_pt", C.c_float), ("thold_ptsum", C.c_float), ("max_len", C.c_int), ("split_on_word", C.c_bool),
                 ("max_tokens", C.c_int), ("debug_mode", C.c_bool), ("audio_ctx", C.c_int), ("tdrz_enable", C.c_bool),
                 ("suppress_regex", C.c_char_p), ("initial_prompt", C.c_char_p), ("prompt_tokens", C.c_void_p),
                 ("prompt_n_tokens", C.c_int), ("language", C.c_char_p), ("detect_language", C.c_bool),
                 ("suppress_blank", C.c_bool), ("suppress_non_speech_tokens", C.c_bool)] +
                [(n, C.c_float) for n in ("temperature", "max_initial_ts", "length_penalty", "temperature_inc",
                                          "entropy_thold", "logprob_thold", "no_speech_thold")] +
                [("best_of", C.c_int), ("beam_size", C.c_int), ("patience", C.c_float)] +
                [(f"cb{i}", C.c_void_p) for i in range(8)])


@pytest.fixture(scope="module")
def wlib():
    import q2a
    L = C.CDLL(os.path.join(PKG, "lib", "libq2a.so"))
    vp = C.c_void_p
    L.whisper_init_from_file.restype = vp
    L.whisper_init_from_file.argtypes = [C.c_char_p]
    L.whisper_free.argtypes = [vp]
    L.whisper_set_mel.argtypes = [vp, vp, C.c_int, C.c_int]
    L.whisper_encode.argtypes = [vp, C.c_int, C.c_int]
    L.whisper_n_len.argtypes = [vp]
    L.whisper_get_embd_enc.restype = C.POINTER(C.c_float)
    L.whisper_get_embd_enc.argtypes = [vp, i32p, i32p]
    L.whisper_full_default_params_by_ref.restype = C.POINTER(FullParams)
    L.whisper_full_default_params_by_ref.argtypes = [C.c_int]
    L.whisper_free_params.argtypes = [C.POINTER(FullParams)]
    L.whisper_full.argtypes = [vp, FullParams, vp, C.c_int]
    if os.path.realpath(q2a.LIB_PATH) != os.path.realpath(os.path.join(PKG, "lib", "libq2a.so")):
        pytest.skip("Q2A_LIB_PATH names another build than the one the drivers link")
    return L


def _embd(L, ctx, shape):
    p = L.whisper_get_embd_enc(ctx, None, None)
    return None if not p else np.ctypeslib.as_array(p, shape=shape).copy()


def test_whisper_set_mel_encode_and_full(wlib, engines, make_model, make_clip):
    import q2a
    L = wlib
    path = make_model("tiny", "f16")
    e = engines("tiny", "f16")
    M = e.info.n_mels
    clip = make_clip(1)
    mel = np.ascontiguousarray(e.pcm_to_mel(clip)[:, :777])
    pp = L.whisper_full_default_params_by_ref(0)
    params = FullParams.from_buffer_copy(pp.contents)
    L.whisper_free_params(pp)
    assert (params.n_max_text_ctx, params.language, params.best_of, params.beam_size) == (16384, b"en", 5, 5)
    ctx = L.whisper_init_from_file(path.encode())
    assert ctx
    try:
        short = np.ascontiguousarray(mel[:, :50])
        assert L.whisper_set_mel(ctx, short.ctypes.data, 50, M + 1) == -1   # wrong n_mel
        assert L.whisper_encode(ctx, 0, 1) == -1                            # nothing to encode yet
        assert L.whisper_set_mel(ctx, short.ctypes.data, 50, M) == 0
        assert L.whisper_n_len(ctx) == 50
        # the 1 s rule on n_len: 50 frames return 0 without an embedding
        assert L.whisper_full(ctx, params, None, 0) == 0
        assert _embd(L, ctx, e.out_shape) is None
        assert L.whisper_set_mel(ctx, mel.ctypes.data, 777, M) == 0
        assert L.whisper_n_len(ctx) == 777
        for seek in (0, 100, 1001):   # (1001: behind the last frame, the all-zero window)
            assert L.whisper_encode(ctx, seek, 1) == 0
            want, _, _ = e.encode_host_mel([mel], seek=[seek])
            assert np.array_equal(_embd(L, ctx, e.out_shape).view(np.int32), want[0].view(np.int32)), seek
        params.offset_ms = 1000
        assert L.whisper_full(ctx, params, None, 0) == 0
        want, _, _ = e.encode_host_mel([mel], seek=[100])
        assert np.array_equal(_embd(L, ctx, e.out_shape).view(np.int32), want[0].view(np.int32))
        params.offset_ms = 7000   # 777 < 700 + 100: too short behind the offset, the embedding stays
        assert L.whisper_full(ctx, params, None, 0) == 0
        assert np.array_equal(_embd(L, ctx, e.out_shape).view(np.int32), want[0].view(np.int32))
        # PCM on the same state afterwards: today's bytes, and whisper_encode re-encodes the PCM again
        params.offset_ms = 0
        assert L.whisper_full(ctx, params, clip.ctypes.data, len(clip)) == 0
        pcm_out, _ = e.encode_host([clip])
        assert np.array_equal(_embd(L, ctx, e.out_shape).view(np.int32), pcm_out[0].view(np.int32))
        assert L.whisper_n_len(ctx) == 1 + (len(clip) - 200) // 160
        assert L.whisper_encode(ctx, 100, 1) == 0
        pcm_off, _ = e.encode_host([clip], offset_ms=1000)
        assert np.array_equal(_embd(L, ctx, e.out_shape).view(np.int32), pcm_off[0].view(np.int32))
    finally:
        L.whisper_free(ctx)


def test_q2a_main_mel_and_tool_mel(engines, make_model, make_clip, tmp_path):
    """bin/q2a_tool mel writes q2a_pcm_to_mel's frames; bin/q2a_main -mel on that file equals the engine, -ot included."""
    import q2a
    if os.path.realpath(q2a.LIB_PATH) != os.path.realpath(os.path.join(PKG, "lib", "libq2a.so")):
        pytest.skip("Q2A_LIB_PATH names another build than the one the drivers link")
    path = make_model("tiny", "f16")
    e = engines("tiny", "f16")
    s16 = np.clip(np.round(make_clip(1, 192000) * 32767.0), -32768, 32767).astype(np.int16)
    with wave.open(str(tmp_path / "c.wav"), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(s16.tobytes())
    pcm = s16.astype(np.float32) / np.float32(32768.0)
    melf, out = tmp_path / "c.mel", tmp_path / "emb.f32"
    subprocess.run([TOOL, "mel", path, str(tmp_path / "c.wav"), str(melf)], check=True, timeout=120)
    mel = e.pcm_to_mel(pcm)
    assert np.array_equal(np.fromfile(melf, dtype=np.float32).view(np.int32), mel.reshape(-1).view(np.int32))
    for off in (0, 10010):
        r = subprocess.run([MAIN, "-m", path, "-np", "-mel", str(melf), "-ot", str(off), "-oemb", str(out)],
                           capture_output=True, text=True, timeout=120, check=True)
        emb = np.fromfile(out, dtype=np.float32).reshape(e.out_shape)
        want, _, _ = e.encode_host_mel([mel], seek=[off // 10])
        assert np.array_equal(emb.view(np.int32), want[0].view(np.int32)), off
        pcm_out, st = e.encode_host([pcm], offset_ms=off)
        assert st[0] == 0 and np.array_equal(emb.view(np.int32), pcm_out[0].view(np.int32)), off
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith(" ") and len(ln.split()) == 20]
        assert lines == ["".join(" %.3f" % x for x in want[0].reshape(-1)[:20])]


# ---------------------------------------------------------------- 6. arguments and launch structure
def test_mel_encode_arguments(engines):
    """Every bad argument returns Q2A_ERR_ARG (-4) before anything is launched: a 7.0-filled output stays."""
    import q2a
    e = engines("tiny", "f16")
    M = e.info.n_mels
    ld = 100
    buf = torch.zeros(2, M, ld, device="cuda")
    good = dict(clip_stride=M * ld, ld=ld, n_len=[100, 50], seek=[0, 10], key_len=[50, 20])
    bads = [dict(n_len=[0, 50]), dict(n_len=[101, 50]), dict(n_len=[100, -3]), dict(seek=[0, -1]), dict(clip_stride=M * ld - 1),
            dict(clip_stride=-M * ld), dict(key_len=[0, 20]), dict(key_len=[50, T + 1]), dict(kind=3), dict(kind=-1)]
    for kind in (q2a.ENCODE_PLAIN, q2a.ENCODE_PADDED, q2a.ENCODE_VARLEN):
        for bad in bads:
            if "key_len" in bad and kind == q2a.ENCODE_PLAIN:
                continue   # ignored for PLAIN (below)
            a = dict(good, kind=kind)
            a.update(bad)
            out = torch.full((2,) + e.out_shape, 7.0, device="cuda")
            with pytest.raises(q2a.Q2AError) as ei:
                e.encode_device_mel(buf.data_ptr(), a["clip_stride"], a["ld"], a["n_len"], out.data_ptr(), kind=a["kind"],
                                    seek=a["seek"], key_len=a["key_len"])
            assert ei.value.rc == -4, (kind, bad)
            x = torch.full((2 * T, e.info.n_audio_state), 7.0, device="cuda")
            if "key_len" not in bad and "kind" not in bad:
                with pytest.raises(q2a.Q2AError) as ei:
                    e.test_frontend_mel(buf.data_ptr(), a["clip_stride"], a["ld"], a["n_len"], x.data_ptr(), seek=a["seek"])
                assert ei.value.rc == -4, bad
            torch.cuda.synchronize()
            assert (out == 7.0).all() and (x == 7.0).all(), (kind, bad)
    # host variant: n_len is the array's own width, so seek, key_len and kind remain
    mels = [np.zeros((M, 100), np.float32), np.zeros((M, 50), np.float32)]
    for kw in (dict(seek=[0, -1]), dict(kind=q2a.ENCODE_PADDED, key_len=[0, 20]), dict(kind=q2a.ENCODE_VARLEN, key_len=[50, T + 1]),
               dict(kind=5)):
        hout = np.full((2,) + e.out_shape, 7.0, dtype=np.float32)
        got = e.encode_host_mel(mels, out=hout, raise_on_error=False, **kw)
        assert got[3] == -4 and (hout == 7.0).all(), kw
    # PLAIN does not read key_len
    out = torch.full((2,) + e.out_shape, float("nan"), device="cuda")
    _, st = e.encode_device_mel(buf.data_ptr(), M * ld, ld, [100, 50], out.data_ptr(), key_len=[0, T + 7])
    torch.cuda.synchronize()
    assert list(st) == [q2a.CLIP_ENCODED] * 2 and torch.isfinite(out).all()


PROF_CLASSES = ["mel", "conv1", "conv2", "ln", "gemm_qkv", "attn", "quant", "gemm_o", "gemm_fc1", "gemm_fc2", "pool"]   # Q2A_PROF_*


@pytest.mark.parametrize("wt", ["f16", "q4_k"])
def test_launches_of_a_mel_encode(engines, batch, wt):
    """By the engine's per-class profile counters: a mel encode books ONE launch under mel (the ingest kernel) and in
    every other class what the PCM encode of its kind books."""
    import q2a
    e = engines("tiny", wt)
    lib, h = q2a.lib(), C.c_void_p(e.h)
    clips, offs, lens = batch
    mels = [e.pcm_to_mel(c) for c in clips]
    buf, ld, n_lens = _mel_batch(mels)
    pcm, stride, ns = _pcm_batch(clips)
    out = torch.empty((3,) + e.out_shape, device="cuda")
    cnt = (C.c_int64 * len(PROF_CLASSES))()

    def counts(call):
        call()
        torch.cuda.synchronize()
        assert lib.q2a_profile_read(h, None, cnt, len(PROF_CLASSES), 1) == 0
        return dict(zip(PROF_CLASSES, cnt))

    pcm_calls = {q2a.ENCODE_PLAIN: lambda: e.encode_device(pcm.data_ptr(), stride, ns, out.data_ptr()),
                 q2a.ENCODE_PADDED: lambda: e.encode_device_padded(pcm.data_ptr(), stride, ns, out.data_ptr(), key_len=lens),
                 q2a.ENCODE_VARLEN: lambda: e.encode_device_varlen(pcm.data_ptr(), stride, ns, out.data_ptr(), key_len=lens)}
    assert lib.q2a_profile_read(h, None, None, 0, 1) == 0
    assert lib.q2a_profile_enable(h, 1) == 0
    try:
        for kind, pcm_call in pcm_calls.items():
            want = counts(pcm_call)
            got = counts(lambda: e.encode_device_mel(buf.data_ptr(), buf.shape[1] * ld, ld, n_lens, out.data_ptr(), kind=kind,
                                                     key_len=lens))
            assert want["mel"] == 1 and got["mel"] == 1 and got == want, kind
            assert got["conv1"] == got["conv2"] == 1 and got["attn"] == e.info.n_audio_layer
    finally:
        lib.q2a_profile_enable(h, 0)
        lib.q2a_profile_read(h, None, None, 0, 1)


# ---------------------------------------------------------------- 7. the HF names
def test_encode_features_equals_encode_device_mel(engines, make_clip):
    """input_features [3][128][3000] (torch CUDA) with a feature_attention_mask -> encode_device_mel(VARLEN) with the
    mask's key lengths; the numpy form (host entry point) gives the same bytes."""
    import q2a
    e = engines("tiny", "f16")
    assert e.info.n_mels == 128
    feats = np.stack([e.pcm_to_mel(make_clip(c, 480000))[:, :TM] for c in (0, 1, 2)])
    valid = [3000, 777, 100]
    mask = np.zeros((3, TM), dtype=np.int64)
    for c, n in enumerate(valid):
        mask[c, :n] = 1
    kl = [1500, 389, 50]
    assert list(q2a.features_key_len(valid)) == kl
    x = torch.from_numpy(feats).cuda()
    out, ol = e.encode_features(x, torch.from_numpy(mask).cuda())
    torch.cuda.synchronize()
    assert out.is_cuda and tuple(out.shape) == (3,) + e.out_shape and list(ol) == [750, 194, 25]
    want = torch.full_like(out, float("nan"))
    wol, _ = e.encode_device_mel(x.data_ptr(), 128 * TM, TM, [TM] * 3, want.data_ptr(), kind=q2a.ENCODE_VARLEN, key_len=kl)
    torch.cuda.synchronize()
    assert list(wol) == list(ol) and _same_bits(out, want)
    for c in range(3):
        assert out[c, :ol[c]].any() and not out[c, ol[c]:].any()
    hout, hol = e.encode_features(feats, mask)
    assert list(hol) == list(ol) and np.array_equal(hout.view(np.int32), out.cpu().numpy().view(np.int32))
    pout, pol = e.encode_features(x, torch.from_numpy(mask).cuda(), kind="padded")
    torch.cuda.synchronize()
    assert list(pol) == list(ol) and _same_bits(pout, out)
    # no mask: every frame valid
    fout, fol = e.encode_features(x)
    torch.cuda.synchronize()
    assert list(fol) == [750] * 3 and _same_bits(fout[0], out[0])
