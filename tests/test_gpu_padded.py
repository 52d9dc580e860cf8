"""Padding-aware encode on the GPU: the key-length instantiation of the attention kernel (q2a_attn.hip,
k_attn_t<true, NQB, true>) through q2a_test_attention_len / q2a_test_block_len, and the padded entry points
q2a_encode_device_padded / q2a_encode_host_padded. All tests here need an MI355X."""
import numpy as np
import pytest

from conftest import rel_errors

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

T = 1500
# the lengths where the 32-key tiling can go wrong: one-tile loops (1, 2, 31, 32), two tiles (33 .. 64), three (65, 96),
# the last whole tile (1472 = 46 * 32), one key into the last tile, the full window
EDGE_LENS = [1, 2, 31, 32, 33, 63, 64, 65, 96, 1472, 1473, 1500]


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


def _qkv(B, D, seed, qs, ks):
    g = torch.Generator(device="cpu").manual_seed(seed)
    q = (torch.randn(B * T, D, generator=g) * qs).cuda()
    k = (torch.randn(B * T, D, generator=g) * ks).cuda()
    v = torch.randn(B * T, D, generator=g).cuda()
    return q, k, v


def _attn_len(e, q, k, v, B, lens):
    out = torch.full_like(q, float("nan"))   # every row must be written by the kernel
    e.test_attention_len(q.data_ptr(), k.data_ptr(), v.data_ptr(), B, lens, out.data_ptr())
    torch.cuda.synchronize()
    return out


def _attn(e, q, k, v, B):
    out = torch.empty_like(q)
    e.test_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), B, out.data_ptr())
    torch.cuda.synchronize()
    return out


def _ref_rows(q, k, v, c, L, H):
    """float64 softmax attention of clip c's queries < L with keys >= L at -inf -> [L][D] (float64, on the GPU)."""
    D = q.shape[1]
    sl = slice(c * T, (c + 1) * T)
    qh = q[sl][:L].view(L, H, 64).permute(1, 0, 2).double()
    kh = k[sl].view(T, H, 64).permute(1, 0, 2).double()
    vh = v[sl].view(T, H, 64).permute(1, 0, 2).double()
    s = qh @ kh.transpose(-1, -2)
    s.masked_fill_(torch.arange(T, device=s.device) >= L, float("-inf"))
    return (torch.softmax(s, dim=-1) @ vh).permute(1, 0, 2).reshape(L, D)


def _query_tile(B, H):
    """Queries per workgroup of the launch (q2a_attn.hip launcher): 64 when the 128-query grid would not fill the CUs."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return 64 if ((T + 127) // 128) * H * B < cus else 128


@pytest.fixture(scope="module")
def edge_case(engines):
    """The 12-clip launch at EDGE_LENS (inputs as test_attention_matches_fp32_reference) and its clean output, shared by
    the float64 comparison and the never-read check."""
    e = engines("tiny", "f16")
    B = len(EDGE_LENS)
    q, k, v = _qkv(B, 256, 0, 0.5, 1.5)
    return e, q, k, v, _attn_len(e, q, k, v, B, EDGE_LENS)


# ---------------------------------------------------------------- 1. against float64
def _check_against_f64(out, q, k, v, lens, H):
    worst = (0.0, 0.0)
    for c, L in enumerate(lens):
        ref = _ref_rows(q, k, v, c, L, H)
        got = out[c * T:c * T + L]
        assert torch.isfinite(got).all(), f"clip {c} (key_len {L})"
        mx, l2 = rel_errors(got.cpu().numpy(), ref.cpu().numpy())
        print(f"key_len {L}: max-rel {mx:.3e} rel-L2 {l2:.3e}")
        worst = (max(worst[0], mx), max(worst[1], l2))
        # the bar of test_attention_matches_fp32_reference (F32-class contract), per clip on its valid rows
        assert mx < 2e-5 and l2 < 5e-6, (c, L, mx, l2)
    return worst


def test_attention_len_matches_float64_at_tile_edges(edge_case):
    e, q, k, v, out = edge_case
    _check_against_f64(out, q, k, v, EDGE_LENS, 4)


def test_attention_len_matches_float64_full_size(engines):
    e = engines("full", "f16")
    lens = [700, 1500]
    q, k, v = _qkv(2, 1280, 0, 0.5, 1.5)
    _check_against_f64(_attn_len(e, q, k, v, 2, lens), q, k, v, lens, 20)


# ---------------------------------------------------------------- 2. full length == the unmasked kernel
@pytest.mark.parametrize("B", [1, 6])   # 1: the narrow (64-query) grid
def test_attention_len_full_length_equals_unmasked_bits(engines, B):
    e = engines("tiny", "f16")
    q, k, v = _qkv(B, 256, 11 + B, 0.5, 1.5)
    a = _attn_len(e, q, k, v, B, [T] * B)
    b = _attn(e, q, k, v, B)
    assert torch.equal(a, b)


# ---------------------------------------------------------------- 3. padded keys are never read
def test_attention_len_never_reads_padded_keys(edge_case):
    """Rows >= key_len of K and V hold NaN in the second run: data in rows a correct kernel never touches."""
    e, q, k, v, clean = edge_case
    B, H = len(EDGE_LENS), 4
    assert torch.isfinite(clean).all()   # straddling tiles' padded query rows too: finite for finite inputs
    kn, vn = k.clone(), v.clone()
    for c, L in enumerate(EDGE_LENS):
        kn[c * T + L:(c + 1) * T] = float("nan")
        vn[c * T + L:(c + 1) * T] = float("nan")
    dirty = _attn_len(e, q, kn, vn, B, EDGE_LENS)
    tile = _query_tile(B, H)
    for c, L in enumerate(EDGE_LENS):
        a, b = clean[c * T:c * T + L], dirty[c * T:c * T + L]
        assert torch.isfinite(b).all(), f"clip {c} (key_len {L}) read a padded key"
        assert torch.equal(a, b), f"clip {c} (key_len {L})"
        past = ((L + tile - 1) // tile) * tile   # first query tile wholly past the length
        for o in (clean, dirty):
            assert not o[c * T + past:(c + 1) * T].any(), f"clip {c} (key_len {L}): rows >= {past} not zero"


# ---------------------------------------------------------------- 4. batch position / grid shape, re-base path running
def test_attention_len_batch_equals_single_clip_bits(engines):
    e = engines("tiny", "f16")
    lens = [1500, 65, 700, 33, 1473, 1]
    B = len(lens)
    q, k, v = _qkv(B, 256, 7, 2.0, 2.0)   # large scores: the re-base path runs (as the narrow-grid test)
    out = _attn_len(e, q, k, v, B, lens)
    for c, L in enumerate(lens):
        sl = slice(c * T, (c + 1) * T)
        o1 = _attn_len(e, q[sl].contiguous(), k[sl].contiguous(), v[sl].contiguous(), 1, [L])
        assert torch.equal(o1[:L], out[sl][:L]), f"clip {c} (key_len {L}): batch differs from the one-clip launch"


# ---------------------------------------------------------------- 5. one block ignores the padding
@pytest.mark.parametrize("wt", ["f16", "q4_k"])
def test_block_len_ignores_padded_rows(engines, wt):
    e = engines("tiny", wt)
    D, B, L = 256, 2, 200
    g = torch.Generator(device="cpu").manual_seed(5)
    x1 = torch.randn(B * T, D, generator=g).cuda()
    x2 = x1.clone()
    x2[L:T] = torch.randn(T - L, D, generator=g).cuda()   # other finite values in clip 0's padding

    def run(x, lens):
        y = x.clone()
        if lens is None:
            e.test_block(0, y.data_ptr(), B)
        else:
            e.test_block_len(0, y.data_ptr(), B, lens)
        torch.cuda.synchronize()
        return y

    a, b = run(x1, [L, T]), run(x2, [L, T])
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    assert torch.equal(a[:L], b[:L]), "valid rows of clip 0 depend on its padding"
    assert torch.equal(a[T:], b[T:]), "clip 1 depends on clip 0"
    # the unmasked block does depend on it: this test can fail
    ua, ub = run(x1, None), run(x2, None)
    assert not torch.equal(ua[:L], ub[:L])
    assert torch.equal(ua[T:], ub[T:])


# ---------------------------------------------------------------- 6. end to end
def _encode_padded(e, clips, key_len=None, offsets_ms=None):
    n = len(clips)
    stride = max(len(c) for c in clips)
    pcm = torch.zeros(n, stride)
    for i, c in enumerate(clips):
        pcm[i, :len(c)] = torch.from_numpy(np.ascontiguousarray(c))
    pcm = pcm.cuda()
    out = torch.full((n,) + e.out_shape, float("nan"), device="cuda")
    ol, st = e.encode_device_padded(pcm.data_ptr(), stride, [len(c) for c in clips], out.data_ptr(), offsets_ms=offsets_ms,
                                    key_len=key_len)
    torch.cuda.synchronize()
    return out, ol, st


def _encode(e, clips):
    n = len(clips)
    stride = max(len(c) for c in clips)
    pcm = torch.zeros(n, stride)
    for i, c in enumerate(clips):
        pcm[i, :len(c)] = torch.from_numpy(np.ascontiguousarray(c))
    pcm = pcm.cuda()
    out = torch.full((n,) + e.out_shape, float("nan"), device="cuda")
    st = e.encode_device(pcm.data_ptr(), stride, [len(c) for c in clips], out.data_ptr())
    torch.cuda.synchronize()
    return out, st


@pytest.mark.parametrize("wt", ["f16", "q4_k"])
def test_padded_encode_ignores_audio_past_the_key_length(engines, make_clip, wt):
    """Encoder row j < 200 depends on mel frames <= 401, i.e. on samples < 64 360, through the two convolutions; with
    key_len 200 nothing later reaches it through the attention either."""
    e = engines("tiny", wt)
    a = make_clip(0, 160000).copy()
    b = a.copy()
    b[80000:] = 0.25 * make_clip(1, 160000)[80000:]
    assert np.array_equal(a[:80000], b[:80000]) and not np.array_equal(a[80000:], b[80000:])
    # the clip maximum the mel clamp uses lies in the shared part
    assert np.abs(b).argmax() < 80000 and np.abs(b[:80000]).max() > 2 * np.abs(b[80000:]).max()
    out, ol, st = _encode_padded(e, [a, b], key_len=[200, 200])
    assert list(st) == [0, 0] and list(ol) == [100, 100]
    assert torch.isfinite(out).all()
    assert torch.equal(out[0, :100], out[1, :100])
    assert not out[:, 100:].any(), "rows >= out_len must be zeros"
    un, _ = _encode(e, [a, b])
    assert not torch.equal(un[0, :100], un[1, :100]), "the unmasked encode sees the difference: this test can fail"


# ---------------------------------------------------------------- 7. a 30 s clip through the padded entry point
def test_padded_encode_of_a_full_window_equals_the_unmasked_encode(engines, make_clip):
    import q2a
    e = engines("tiny", "f16")
    full, short = make_clip(0, 480000), make_clip(2, 116800)
    un, _ = _encode(e, [full])
    out, ol, st = _encode_padded(e, [full])
    assert list(ol) == [750] and list(st) == [q2a.CLIP_ENCODED]
    assert torch.equal(out, un)
    out2, ol2, st2 = _encode_padded(e, [full, short])
    assert list(ol2) == [750, 182] == [q2a.valid_lengths(480000)[1], q2a.valid_lengths(116800)[1]]
    assert torch.equal(out2[0], un[0])
    assert torch.isfinite(out2[1]).all() and out2[1, :182].any() and not out2[1, 182:].any()
    # the host entry point: the same bits
    hout, hol = e.encode_host_padded([full, short])
    assert list(hol) == [750, 182]
    assert np.array_equal(hout, out2.cpu().numpy())


# ---------------------------------------------------------------- 8. arguments
def test_padded_encode_arguments(engines, make_model, make_clip):
    import q2a
    e = engines("tiny", "f16")
    clip = make_clip(0, 160000)
    for bad in (0, T + 1):
        pcm = torch.from_numpy(clip).cuda()
        out = torch.full((1,) + e.out_shape, 7.0, device="cuda")
        with pytest.raises(q2a.Q2AError) as ei:
            e.encode_device_padded(pcm.data_ptr(), len(clip), [len(clip)], out.data_ptr(), key_len=[bad])
        assert ei.value.rc == -4
        torch.cuda.synchronize()
        assert (out == 7.0).all(), "nothing may be launched"
        with pytest.raises(q2a.Q2AError) as ei:
            e.encode_host_padded([clip], key_len=[bad])
        assert ei.value.rc == -4
        q = torch.zeros(T, 256, device="cuda")
        with pytest.raises(q2a.Q2AError) as ei:
            e.test_attention_len(q.data_ptr(), q.data_ptr(), q.data_ptr(), 1, [bad], out.data_ptr())
        assert ei.value.rc == -4
    # under 1 s of audio: skipped, no valid output rows, zeros
    out, ol, st = _encode_padded(e, [clip, clip[:8000]])
    assert list(st) == [q2a.CLIP_ENCODED, q2a.CLIP_SKIPPED]
    assert list(ol) == [q2a.valid_lengths(160000)[1], 0]
    assert not out[1].any()
    hout, hol, hst = e.encode_host_padded([clip, clip[:8000]], return_status=True)
    assert list(hst) == [q2a.CLIP_ENCODED, q2a.CLIP_SKIPPED] and list(hol) == list(ol)
    assert np.array_equal(hout, out.cpu().numpy())
    # the bf16 activation contract has no key-length kernel
    eb = q2a.Engine(make_model("tiny", "f16"), device=0, act=q2a.ACT_BF16)
    try:
        pcm = torch.from_numpy(clip).cuda()
        out = torch.full((1,) + eb.out_shape, 7.0, device="cuda")
        with pytest.raises(q2a.Q2AError) as ei:
            eb.encode_device_padded(pcm.data_ptr(), len(clip), [len(clip)], out.data_ptr())
        assert ei.value.rc == -6
        with pytest.raises(q2a.Q2AError) as ei:
            eb.encode_host_padded([clip])
        assert ei.value.rc == -6
        torch.cuda.synchronize()
        assert (out == 7.0).all()
    finally:
        eb.close()


# ---------------------------------------------------------------- 9. composition
def test_padded_encode_is_the_composition_of_its_stages(engines, make_clip):
    import q2a
    e = engines("tiny", "f16")
    clip = make_clip(2, 116800)
    enc_len, out_len = q2a.valid_lengths(len(clip))
    assert (enc_len, out_len) == (365, 182)
    pcm = torch.from_numpy(clip).cuda()
    x = torch.empty(T, 256, device="cuda")
    e.test_frontend(pcm.data_ptr(), len(clip), [len(clip)], x.data_ptr())
    for layer in (0, 1):
        e.test_block_len(layer, x.data_ptr(), 1, [enc_len])
    staged = torch.empty((1,) + e.out_shape, device="cuda")
    e.test_pool_ln(x.data_ptr(), 1, staged.data_ptr())
    torch.cuda.synchronize()
    out, ol, _ = _encode_padded(e, [clip])
    assert list(ol) == [out_len]
    assert torch.equal(out[0, :out_len], staged[0, :out_len])
    assert not out[0, out_len:].any()
