"""Variable-length encode on the GPU: the packed instantiation of the attention kernel (q2a_attn.hip,
k_attn_t<true, NQB, true, true>) through q2a_test_attention_varlen / q2a_test_block_varlen, and the entry points
q2a_encode_device_varlen / q2a_encode_host_varlen. The acceptance criterion is bit identity with the padded family
(tests/test_gpu_padded.py): every comparison with it here is exact. All tests need an MI355X."""
import numpy as np
import pytest

import varlen_cases as vc
from test_gpu_padded import EDGE_LENS, _check_against_f64, _encode_padded, _qkv

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

T = 1500
# the tile edges of the key-length tests, plus the edges of the 16-row packing: one short of a block, a whole block, one
# into the next; a length whose last block ends inside the window (1481 -> 1488), the last whole block (1488), and the
# first length whose segment is cut at the window (1489 -> 1500)
LENS = EDGE_LENS + [15, 16, 17, 1481, 1488, 1489]


@pytest.fixture(scope="module")
def engines(make_model):
    import q2a
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    cache = {}

    def get(cfg, wt):
        if (cfg, wt) not in cache:
            cache[(cfg, wt)] = q2a.Engine(make_model(cfg, wt), device=0)
        return cache[(cfg, wt)]

    yield get
    for e in cache.values():
        e.close()


def _layout(lens):
    import q2a
    m, rs = q2a.varlen_rows(lens, T)
    return m, [int(r) for r in rs]


def _pack(x, lens):
    """[B*T][D] windows -> the packed [M_tot][D] rows of q2a_varlen_rows."""
    m, rs = _layout(lens)
    out = torch.cat([x[c * T:c * T + rs[c + 1] - rs[c]] for c in range(len(lens))])
    assert out.shape[0] == m
    return out.contiguous()


SENTINEL_ROWS, SENTINEL = 8, 7.0


def _attn_varlen(e, qp, kp, vp, lens):
    """The packed kernel on packed operands -> packed output; the output buffer starts as NaN (every packed row must be
    written) with sentinel rows behind M_tot (which must be kept)."""
    m = qp.shape[0]
    buf = torch.full((m + SENTINEL_ROWS, qp.shape[1]), float("nan"), device="cuda")
    buf[m:] = SENTINEL
    e.test_attention_varlen(qp.data_ptr(), kp.data_ptr(), vp.data_ptr(), len(lens), lens, buf.data_ptr())
    torch.cuda.synchronize()
    assert (buf[m:] == SENTINEL).all(), "rows behind M_tot were written"
    return buf[:m]


def _attn_len(e, q, k, v, lens):
    out = torch.full_like(q, float("nan"))
    e.test_attention_len(q.data_ptr(), k.data_ptr(), v.data_ptr(), len(lens), lens, out.data_ptr())
    torch.cuda.synchronize()
    return out


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def edge_case(engines):
    """One launch over LENS (inputs drawn as test_attention_len_matches_float64_at_tile_edges draws them) through the
    key-length kernel and, packed, through the packed kernel; shared and left unchanged."""
    e = engines("tiny", "f16")
    q, k, v = _qkv(len(LENS), 256, 0, 0.5, 1.5)
    padded = _attn_len(e, q, k, v, LENS)
    packed = _attn_varlen(e, _pack(q, LENS), _pack(k, LENS), _pack(v, LENS), LENS)
    return e, q, k, v, padded, packed


# ---------------------------------------------------------------- 1. attention bits
def test_attention_varlen_equals_the_key_length_kernel_bits(edge_case):
    e, q, k, v, padded, packed = edge_case
    assert torch.isfinite(packed).all(), "every packed row is written, rows key_len .. seg_rows-1 included"
    assert _same_bits(packed, _pack(padded, LENS))


def test_attention_varlen_one_clip_launches(edge_case):
    """One clip per launch: the 64-query grid of both kernels; the same bits as inside the batch."""
    e, q, k, v, padded, packed = edge_case
    _, rs = _layout(LENS)
    for c, L in enumerate(LENS):
        sl = slice(c * T, (c + 1) * T)
        q1, k1, v1 = (x[sl].contiguous() for x in (q, k, v))
        one = _attn_varlen(e, _pack(q1, [L]), _pack(k1, [L]), _pack(v1, [L]), [L])
        assert _same_bits(one, _pack(_attn_len(e, q1, k1, v1, [L]), [L])), f"key_len {L}"
        assert _same_bits(one, packed[rs[c]:rs[c + 1]]), f"key_len {L}: one-clip launch differs from the batch"


def test_attention_varlen_matches_float64(edge_case):
    e, q, k, v, padded, packed = edge_case
    _, rs = _layout(LENS)
    out = torch.zeros_like(q)   # back into windows: _check_against_f64 reads rows c*T .. c*T + key_len - 1
    for c in range(len(LENS)):
        out[c * T:c * T + rs[c + 1] - rs[c]] = packed[rs[c]:rs[c + 1]]
    _check_against_f64(out, q, k, v, LENS, 4)   # 2e-5 max-rel, 5e-6 rel-L2 per clip on its valid rows


# ---------------------------------------------------------------- 2. the padded queries' re-base
def test_padded_queries_rebase_the_valid_rows(engines):
    """key_len 1481: queries 1481 .. 1487 alone re-base block 92 (tests/test_varlen_cpu.py proves it on the model), which
    changes the bits of the valid rows 1472 .. 1480. The packed kernel carries those seven rows and reproduces them."""
    e = engines("tiny", "f16")
    L = [vc.KEY_LEN]
    q, k, v = (torch.from_numpy(x).cuda() for x in vc.rebase_clip())
    padded = _attn_len(e, q, k, v, L)
    # the test can fail: with the padded queries silenced the key-length kernel gives the valid rows other bits
    quiet = _attn_len(e, torch.from_numpy(vc.quiet_padding(q.cpu().numpy())).cuda(), k, v, L)
    assert torch.isfinite(padded[vc.VALID]).all() and torch.isfinite(quiet[vc.VALID]).all()
    assert not _same_bits(padded[vc.VALID], quiet[vc.VALID])
    assert _same_bits(padded[:vc.VALID.start], quiet[:vc.VALID.start]), "only block 92 may differ"
    packed = _attn_varlen(e, _pack(q, L), _pack(k, L), _pack(v, L), L)
    assert packed.shape[0] == vc.PADDED.stop == 1488
    assert _same_bits(packed[:vc.KEY_LEN], padded[:vc.KEY_LEN])
    assert _same_bits(packed, padded[:1488])


# ---------------------------------------------------------------- 3. nothing outside the segments is touched
def test_attention_varlen_never_reads_the_padding_rows_as_keys(edge_case):
    """Packed K and V rows key_len .. seg_rows-1 hold NaN in the second run. (Sentinel rows and full coverage of the
    packed rows are checked in every _attn_varlen call.)"""
    e, q, k, v, padded, clean = edge_case
    _, rs = _layout(LENS)
    kp, vp = _pack(k, LENS), _pack(v, LENS)
    poisoned = 0
    for c, L in enumerate(LENS):
        kp[rs[c] + L:rs[c + 1]] = float("nan")
        vp[rs[c] + L:rs[c + 1]] = float("nan")
        poisoned += rs[c + 1] - rs[c] - L
    assert poisoned > 0
    dirty = _attn_varlen(e, _pack(q, LENS), kp, vp, LENS)
    for c, L in enumerate(LENS):
        a, b = clean[rs[c]:rs[c] + L], dirty[rs[c]:rs[c] + L]
        assert torch.isfinite(b).all(), f"key_len {L}: a padding row was read as a key"
        assert _same_bits(a, b), f"key_len {L}"


# ---------------------------------------------------------------- 4. block bits
def _block_pair(e, D, lens, seed):
    B = len(lens)
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(B * T, D, generator=g).cuda()
    y = x.clone()
    e.test_block_len(0, y.data_ptr(), B, lens)
    m, _ = _layout(lens)
    xp = torch.cat([_pack(x, lens), torch.full((SENTINEL_ROWS, D), SENTINEL, device="cuda")])
    e.test_block_varlen(0, xp.data_ptr(), B, lens)
    torch.cuda.synchronize()
    assert (xp[m:] == SENTINEL).all(), "rows behind M_tot were written"
    return xp[:m], _pack(y, lens)


@pytest.mark.parametrize("wt", ["f16", "q4_k", "q8_0"])
def test_block_varlen_equals_the_padded_block_bits(engines, wt):
    lens = [200, 1500, 17]
    packed, want = _block_pair(engines("tiny", wt), 256, lens, 5)
    assert packed.shape[0] == 208 + 1500 + 32
    assert torch.isfinite(packed).all()
    assert _same_bits(packed, want)


def test_block_varlen_full_size_q4_k(engines):
    """D = 1280, Q4_K, 8 clips: 9 740 packed rows, not a multiple of 256 and past the row counts where the Q|K|V and fc1
    GEMMs switch to their 256-row tile regimes, while the padded block runs 12 000."""
    lens = [1500, 1500, 1500, 1500, 1500, 1200, 700, 333]
    packed, want = _block_pair(engines("full", "q4_k"), 1280, lens, 6)
    assert packed.shape[0] == 9740 and packed.shape[0] % 256 != 0
    assert torch.isfinite(packed).all()
    assert _same_bits(packed, want)


# ---------------------------------------------------------------- 5. end to end
def _encode_varlen(e, clips, key_len=None, offsets_ms=None):
    n = len(clips)
    stride = max(len(c) for c in clips)
    pcm = torch.zeros(n, stride)
    for i, c in enumerate(clips):
        pcm[i, :len(c)] = torch.from_numpy(np.ascontiguousarray(c))
    pcm = pcm.cuda()
    out = torch.full((n,) + e.out_shape, float("nan"), device="cuda")
    ol, st = e.encode_device_varlen(pcm.data_ptr(), stride, [len(c) for c in clips], out.data_ptr(), offsets_ms=offsets_ms,
                                    key_len=key_len)
    torch.cuda.synchronize()
    return out, ol, st


@pytest.fixture(scope="module")
def batch(make_clip):
    """A 30 s clip, 7.3 s, 1.2 s, and half a second (skipped)."""
    return [make_clip(0, 480000), make_clip(2, 116800), make_clip(1, 19200), make_clip(0, 160000)[:8000]]


@pytest.mark.parametrize("wt", ["f16", "q4_k", "q8_0"])
def test_varlen_encode_equals_the_padded_encode_bytes(engines, batch, wt):
    import q2a
    e = engines("tiny", wt)
    for kw in (dict(), dict(key_len=[1500, 17, 1, 9]), dict(offsets_ms=[10000, 1000, 100, 0])):
        want, wol, wst = _encode_padded(e, batch, **kw)
        got, ol, st = _encode_varlen(e, batch, **kw)
        assert list(st) == list(wst) == [q2a.CLIP_ENCODED] * 3 + [q2a.CLIP_SKIPPED], kw
        assert list(ol) == list(wol) and ol[3] == 0, kw
        assert not torch.isnan(got).any(), "the whole output buffer is written"
        assert _same_bits(got, want), kw
        hout, hol, hst = e.encode_host_varlen(batch, return_status=True, **kw)
        assert list(hol) == list(ol) and list(hst) == list(st)
        assert np.array_equal(hout.view(np.int32), got.cpu().numpy().view(np.int32)), kw
    assert list(_encode_varlen(e, batch)[1]) == [750, 182, 30, 0]


def test_varlen_encode_alone_equals_inside_the_batch(engines, batch):
    e = engines("tiny", "q4_k")
    inside, ol, _ = _encode_varlen(e, batch)
    for c in (0, 1, 2):
        alone, ol1, _ = _encode_varlen(e, [batch[c]])
        assert list(ol1) == [ol[c]]
        assert _same_bits(alone[0], inside[c]), f"clip {c}"


def test_varlen_encode_of_skipped_clips_only(engines, batch):
    import q2a
    e = engines("tiny", "f16")
    short = batch[3]
    out, ol, st = _encode_varlen(e, [short, short[:4000]])
    assert list(st) == [q2a.CLIP_SKIPPED] * 2 and list(ol) == [0, 0]
    assert _same_bits(out, torch.zeros_like(out))
    hout, hol, hst = e.encode_host_varlen([short, short[:4000]], return_status=True)
    assert list(hst) == [q2a.CLIP_SKIPPED] * 2 and list(hol) == [0, 0] and not hout.any()


# ---------------------------------------------------------------- 6. launch structure
PROF_CLASSES = ["mel", "conv1", "conv2", "ln", "gemm_qkv", "attn", "quant", "gemm_o", "gemm_fc1", "gemm_fc2", "pool"]   # Q2A_PROF_*


@pytest.mark.parametrize("wt", ["f16", "q4_k"])
def test_launches_per_entry_point(engines, batch, wt):
    """What each entry point launches, by the engine's per-class profile counters (one count per launch): the three
    families run the same front end and the same launches per layer, and differ in the pool class alone — pool (plain),
    pool + tail zeroing (padded), gather + pool (packed). A packed encode with no clip to encode launches its pool
    kernel (which writes the zeros) and nothing else."""
    import ctypes as C

    import q2a
    e = engines("tiny", wt)
    lib, h = q2a.lib(), C.c_void_p(e.h)
    L = e.info.n_audio_layer
    clips, lens = batch[:3], [1500, 500, 37]
    stride = max(len(c) for c in clips)
    pcm = torch.zeros(len(clips), stride)
    for i, c in enumerate(clips):
        pcm[i, :len(c)] = torch.from_numpy(np.ascontiguousarray(c))
    pcm = pcm.cuda()
    ns = [len(c) for c in clips]
    out = torch.empty((len(clips),) + e.out_shape, device="cuda")
    cnt = (C.c_int64 * len(PROF_CLASSES))()

    def counts(call):
        call()
        torch.cuda.synchronize()
        assert lib.q2a_profile_read(h, None, cnt, len(PROF_CLASSES), 1) == 0
        return dict(zip(PROF_CLASSES, cnt))

    def want(pool):
        w = {c: L for c in ("gemm_qkv", "attn", "gemm_o", "gemm_fc1", "gemm_fc2")}
        # Q4_K, default fc1 path: the attention output and the fc1 pre-activation each pass a Q8_K quantizer
        w.update(mel=1, conv1=1, conv2=1, ln=2 * L, quant=2 * L if wt == "q4_k" else 0, pool=pool)
        return w

    assert lib.q2a_profile_read(h, None, None, 0, 1) == 0
    assert lib.q2a_profile_enable(h, 1) == 0
    try:
        assert counts(lambda: e.encode_device(pcm.data_ptr(), stride, ns, out.data_ptr())) == want(1)
        assert counts(lambda: e.encode_device_padded(pcm.data_ptr(), stride, ns, out.data_ptr(), key_len=lens)) == want(2)
        assert counts(lambda: e.encode_device_varlen(pcm.data_ptr(), stride, ns, out.data_ptr(), key_len=lens)) == want(2)
        skipped = counts(lambda: _encode_varlen(e, [batch[3], batch[3][:4000]]))
        assert skipped == dict({c: 0 for c in PROF_CLASSES}, pool=1)
    finally:
        lib.q2a_profile_enable(h, 0)
        lib.q2a_profile_read(h, None, None, 0, 1)


# ---------------------------------------------------------------- 7. arguments
def test_varlen_encode_arguments(engines, make_model, make_clip):
    """The cases of test_padded_encode_arguments against the variable-length entry points."""
    import q2a
    e = engines("tiny", "f16")
    clip = make_clip(0, 160000)
    for bad in (0, T + 1):
        pcm = torch.from_numpy(clip).cuda()
        out = torch.full((1,) + e.out_shape, 7.0, device="cuda")
        with pytest.raises(q2a.Q2AError) as ei:
            e.encode_device_varlen(pcm.data_ptr(), len(clip), [len(clip)], out.data_ptr(), key_len=[bad])
        assert ei.value.rc == -4
        torch.cuda.synchronize()
        assert (out == 7.0).all(), "nothing may be launched"
        with pytest.raises(q2a.Q2AError) as ei:
            e.encode_host_varlen([clip], key_len=[bad])
        assert ei.value.rc == -4
        q = torch.zeros(T, 256, device="cuda")
        with pytest.raises(q2a.Q2AError) as ei:
            e.test_attention_varlen(q.data_ptr(), q.data_ptr(), q.data_ptr(), 1, [bad], out.data_ptr())
        assert ei.value.rc == -4
        with pytest.raises(q2a.Q2AError) as ei:
            e.test_block_varlen(0, q.data_ptr(), 1, [bad])
        assert ei.value.rc == -4
        torch.cuda.synchronize()
        assert (out == 7.0).all() and not q.any()
    # under 1 s of audio: skipped, no valid output rows, zeros
    out, ol, st = _encode_varlen(e, [clip, clip[:8000]])
    assert list(st) == [q2a.CLIP_ENCODED, q2a.CLIP_SKIPPED]
    assert list(ol) == [q2a.valid_lengths(160000)[1], 0]
    assert not out[1].any()
    hout, hol, hst = e.encode_host_varlen([clip, clip[:8000]], return_status=True)
    assert list(hst) == [q2a.CLIP_ENCODED, q2a.CLIP_SKIPPED] and list(hol) == list(ol)
    assert np.array_equal(hout, out.cpu().numpy())
    # the bf16 activation contract has no packed kernel
    eb = q2a.Engine(make_model("tiny", "f16"), device=0, act=q2a.ACT_BF16)
    try:
        pcm = torch.from_numpy(clip).cuda()
        out = torch.full((1,) + eb.out_shape, 7.0, device="cuda")
        with pytest.raises(q2a.Q2AError) as ei:
            eb.encode_device_varlen(pcm.data_ptr(), len(clip), [len(clip)], out.data_ptr())
        assert ei.value.rc == -6
        with pytest.raises(q2a.Q2AError) as ei:
            eb.encode_host_varlen([clip])
        assert ei.value.rc == -6
        q = torch.zeros(T, 256, device="cuda")
        with pytest.raises(q2a.Q2AError) as ei:
            eb.test_attention_varlen(q.data_ptr(), q.data_ptr(), q.data_ptr(), 1, [100], out.data_ptr())
        assert ei.value.rc == -6
        with pytest.raises(q2a.Q2AError) as ei:
            eb.test_block_varlen(0, q.data_ptr(), 1, [100])
        assert ei.value.rc == -6
        torch.cuda.synchronize()
        assert (out == 7.0).all()
    finally:
        eb.close()
