"""Audio features in one call on the GPU: q2a_audio_features_device / _device_mel / _host / _host_mel,
Engine.audio_features and the pool kernel behind them (q2a_exact.hip, k_poolnorm_pack) through q2a_test_pool_operand.

The acceptance criterion is bit identity with the composition of the existing entry points: the packed embd_enc is
cat(out[c][:out_len[c]]) of q2a_encode_device_varlen, the features q2a_projector_apply of those rows. Every comparison
with it here is exact; the oracle comparison uses tests/test_projector.py's bars. All tests need an MI355X."""
import os
import subprocess

import numpy as np
import pytest

import operand_cases as oc
import oracle_py
from conftest import TOOL, rel_errors
from q2a import ggmlfile

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

T = 1500
SENTINEL_ROWS, SENTINEL = 8, 7.0
# the edges of the 16-row packing and of AvgPool1d(2): odd and even lengths, one short of a 16-row block, a whole one, one
# into the next, a length whose last block ends inside the window (1481), the first one cut at the window (1489), T
KEY_LENS = [1, 2, 3, 15, 16, 17, 31, 33, 365, 1481, 1489, 1500]
OUT_LENS = [0, 1, 1, 7, 8, 8, 15, 16, 182, 740, 744, 750]
SKIP_AT = 6   # the clip under 1 s, in the middle of the batch


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


@pytest.fixture(scope="module")
def projector_path(host_build, workdir):
    def make(d_in, d_out, wt):
        base = os.path.join(workdir, f"proj-{d_in}x{d_out}-f16.bin")
        if not os.path.exists(base):
            subprocess.check_call([TOOL, "gen-projector", base, str(d_in), str(d_out), "f16", "0x51A2"])
        if wt == "f16":
            return base
        path = os.path.join(workdir, f"proj-{d_in}x{d_out}-{wt}.bin")
        if not os.path.exists(path):
            subprocess.check_call([TOOL, "quantize", base, path, wt, "8"])
        return path
    return make


@pytest.fixture(scope="module")
def projectors(projector_path):
    import q2a
    cache = {}

    def get(d_in, d_out, wt):
        if (d_in, d_out, wt) not in cache:
            cache[(d_in, d_out, wt)] = q2a.Projector(projector_path(d_in, d_out, wt), device=0)
        return cache[(d_in, d_out, wt)]

    yield get
    for p in cache.values():
        p.close()


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


def _mel_batch(mels):
    n_lens = [m.shape[1] for m in mels]
    ld = max(n_lens) + 3
    buf = np.full((len(mels), mels[0].shape[0], ld), np.nan, dtype=np.float32)
    for c, m in enumerate(mels):
        buf[c, :, :m.shape[1]] = m
    return torch.from_numpy(buf).cuda(), ld, n_lens


def _composition(e, pr, clips, key_len=None, offsets_ms=None):
    """The three steps of the existing entry points: encode_device_varlen into the padded buffer, a gather of the valid
    rows, Projector.apply -> (feat or None, embd, out_len, status)."""
    pcm, stride, ns = _pcm_batch(clips)
    out = torch.full((len(clips),) + e.out_shape, float("nan"), device="cuda")
    ol, st = e.encode_device_varlen(pcm.data_ptr(), stride, ns, out.data_ptr(), offsets_ms=offsets_ms, key_len=key_len)
    embd = torch.cat([out[c, :ol[c]] for c in range(len(clips))]).contiguous()
    feat = None
    if pr is not None and embd.shape[0]:
        feat = torch.empty((embd.shape[0], pr.d_out), device="cuda")
        pr.apply(embd.data_ptr(), embd.shape[0], feat.data_ptr())
    torch.cuda.synchronize()
    return feat, embd, ol, st


def _buffers(e, pr, n_tot, feat=True, embd=True):
    """Output buffers of exactly n_tot rows (rows_cap = n_tot) that start as NaN, with sentinel rows behind them."""
    def buf(width):
        b = torch.full((n_tot + SENTINEL_ROWS, width), float("nan"), device="cuda")
        b[n_tot:] = SENTINEL
        return b
    return (buf(pr.d_out) if pr is not None and feat else None), (buf(e.info.n_audio_state) if embd else None)


def _finish(bufs, n_tot):
    torch.cuda.synchronize()
    res = []
    for b in bufs:
        if b is None:
            res.append(None)
            continue
        assert (b[n_tot:] == SENTINEL).all(), "rows behind N_tot were written"
        assert torch.isfinite(b[:n_tot]).all(), "a row below N_tot was not written"
        res.append(b[:n_tot])
    return res


def _features(e, pr, clips, n_tot, key_len=None, offsets_ms=None, feat=True, embd=True):
    """q2a_audio_features_device with rows_cap = n_tot -> (feat or None, embd or None, out_len, status)."""
    pcm, stride, ns = _pcm_batch(clips)
    fb, eb = _buffers(e, pr, n_tot, feat, embd)
    ol, st = e.audio_features_device(pcm.data_ptr(), stride, ns, fb.data_ptr() if fb is not None else 0,
                                     eb.data_ptr() if eb is not None else 0, n_tot, projector=pr if feat else None,
                                     offsets_ms=offsets_ms, key_len=key_len)
    f, m = _finish((fb, eb), n_tot)
    return f, m, ol, st


def _features_mel(e, pr, mels, n_tot, seek=None, key_len=None):
    buf, ld, n_lens = _mel_batch(mels)
    fb, eb = _buffers(e, pr, n_tot)
    ol, st = e.audio_features_device_mel(buf.data_ptr(), buf.shape[1] * ld, ld, n_lens, fb.data_ptr() if fb is not None else 0,
                                         eb.data_ptr(), n_tot, projector=pr, seek=seek, key_len=key_len)
    f, m = _finish((fb, eb), n_tot)
    return f, m, ol, st


@pytest.fixture(scope="module")
def batch13(make_clip):
    """13 clips: twelve of 30 s for KEY_LENS and, at SKIP_AT, half a second (skipped; its key length is any valid one)."""
    full = [make_clip(c, 480000) for c in range(3)]
    clips = [full[i % 3] for i in range(len(KEY_LENS))]
    clips.insert(SKIP_AT, make_clip(0, 160000)[:8000])
    lens = list(KEY_LENS)
    lens.insert(SKIP_AT, 100)
    want = list(OUT_LENS)
    want.insert(SKIP_AT, 0)
    return clips, lens, want


@pytest.fixture(scope="module")
def composed(engines, projectors, batch13):
    """The composition's results for batch13 per (model type, projector type); computed once, left unchanged."""
    cache = {}

    def get(wt, pwt):
        if (wt, pwt) not in cache:
            clips, lens, _ = batch13
            cache[(wt, pwt)] = _composition(engines("tiny", wt), projectors(256, 512, pwt), clips, key_len=lens)
        return cache[(wt, pwt)]
    return get


# ---------------------------------------------------------------- 1. bits against the composition
@pytest.mark.parametrize("wt,pwt", [("f16", "f16"), ("q4_k", "q4_k"), ("q4_k", "q6_k"), ("q8_0", "q8_0")])
def test_audio_features_equal_the_composition_bits(engines, projectors, batch13, composed, wt, pwt):
    """fp16 (mode 0), Q8_K (mode 1, Q4_K and Q6_K weights) and Q8_0 (mode 2) operands straight from the pool kernel."""
    import q2a
    clips, lens, want_ol = batch13
    e, pr = engines("tiny", wt), projectors(256, 512, pwt)
    wfeat, wembd, wol, wst = composed(wt, pwt)
    n_tot = sum(want_ol)
    assert list(wol) == want_ol and wembd.shape[0] == n_tot == q2a.packed_out_rows(want_ol_lens(lens))[0]
    feat, embd, ol, st = _features(e, pr, clips, n_tot, key_len=lens)
    assert list(ol) == want_ol and ol[SKIP_AT] == 0
    assert list(st) == list(wst) and st[SKIP_AT] == q2a.CLIP_SKIPPED
    assert _same_bits(embd, wembd)
    assert _same_bits(feat, wfeat)


def want_ol_lens(lens):
    """The key lengths as q2a_packed_out_rows wants them: 0 for the skipped clip."""
    kl = list(lens)
    kl[SKIP_AT] = 0
    return kl


# ---------------------------------------------------------------- 2. output combinations
def test_output_combinations_give_the_same_bits(engines, projectors, batch13, composed):
    clips, lens, want_ol = batch13
    e, pr = engines("tiny", "q4_k"), projectors(256, 512, "q4_k")
    wfeat, wembd, _, _ = composed("q4_k", "q4_k")
    n_tot = sum(want_ol)
    f, m, ol, _ = _features(e, pr, clips, n_tot, key_len=lens, feat=False)   # p NULL: the packed embd_enc alone
    assert f is None and _same_bits(m, wembd) and list(ol) == want_ol
    f, m, ol, _ = _features(e, pr, clips, n_tot, key_len=lens, embd=False)   # the features alone
    assert m is None and _same_bits(f, wfeat) and list(ol) == want_ol


# ---------------------------------------------------------------- 3. batch independence
def test_a_clip_alone_gives_its_rows_of_the_batch(engines, projectors, batch13, composed):
    import q2a
    clips, lens, want_ol = batch13
    e, pr = engines("tiny", "q4_k"), projectors(256, 512, "q4_k")
    wfeat, wembd, _, _ = composed("q4_k", "q4_k")
    _, start = q2a.packed_out_rows(want_ol_lens(lens))
    for L in (365, 1481, 17):
        c = lens.index(L)
        f, m, ol, _ = _features(e, pr, [clips[c]], L // 2, key_len=[L])
        assert list(ol) == [L // 2]
        sl = slice(int(start[c]), int(start[c + 1]))
        assert _same_bits(m, wembd[sl]) and _same_bits(f, wfeat[sl]), f"key_len {L}"


# ---------------------------------------------------------------- 4. mel against PCM
def test_mel_input_equals_pcm_input(engines, projectors, make_clip):
    """mel = pcm_to_mel(pcm): the log-mel entry point returns the PCM entry point's bytes, one clip from frame 1000
    against offsets_ms 10 000."""
    e, pr = engines("tiny", "q4_k"), projectors(256, 512, "q4_k")
    clips = [make_clip(0, 480000), make_clip(2, 276800), make_clip(1, 192000)]
    lens, offs = [1500, 365, 17], [0, 10000, 0]
    n_tot = sum(L // 2 for L in lens)
    f, m, ol, st = _features(e, pr, clips, n_tot, key_len=lens, offsets_ms=offs)
    mels = [e.pcm_to_mel(c) for c in clips]
    fm, mm, olm, stm = _features_mel(e, pr, mels, n_tot, seek=[o // 10 for o in offs], key_len=lens)
    assert list(olm) == list(ol) == [750, 182, 8] and list(stm) == list(st)
    assert _same_bits(mm, m) and _same_bits(fm, f)


# ---------------------------------------------------------------- 5. host against device
def test_host_entry_points_equal_the_device_ones(engines, projectors, batch13, composed):
    clips, lens, want_ol = batch13
    e, pr = engines("tiny", "q4_k"), projectors(256, 512, "q4_k")
    wfeat, wembd, wol, wst = composed("q4_k", "q4_k")
    hf, hm, hol, hst = e.audio_features_host(clips, projector=pr, key_len=lens, rows_cap=sum(want_ol))
    assert list(hol) == list(wol) and list(hst) == list(wst)
    assert np.array_equal(hm.view(np.int32), wembd.cpu().numpy().view(np.int32))
    assert np.array_equal(hf.view(np.int32), wfeat.cpu().numpy().view(np.int32))
    # log-mel: three clips, derived key lengths
    sub = [clips[0], clips[1][:276800], clips[2][:192000]]
    mels = [e.pcm_to_mel(c) for c in sub]
    n_tot = 3 * 750   # pcm_to_mel pads every clip with 30 s of frames: full windows
    df, dm, dol, dst = _features_mel(e, pr, mels, n_tot)
    hf, hm, hol, hst = e.audio_features_host_mel(mels, projector=pr)
    assert list(hol) == list(dol) == [750] * 3 and list(hst) == list(dst)
    assert np.array_equal(hm.view(np.int32), dm.cpu().numpy().view(np.int32))
    assert np.array_equal(hf.view(np.int32), df.cpu().numpy().view(np.int32))


# ---------------------------------------------------------------- 6. high-level Python
def test_engine_audio_features(engines, projectors, make_clip):
    import q2a
    e, pr = engines("tiny", "q4_k"), projectors(256, 512, "q4_k")
    L = 3000
    frames = [3000, 730, 33]
    x = np.stack([e.pcm_to_mel(make_clip(c, 480000))[:, :L] for c in range(3)])
    mask = np.zeros((3, L), dtype=np.int64)
    for c, n in enumerate(frames):
        mask[c, :n] = 1
    kl = q2a.features_key_len(frames)
    assert list(kl) == [1500, 365, 17]
    n_tot = int((kl // 2).sum())
    wf, wm, wol, _ = _features_mel(e, pr, list(x), n_tot, key_len=kl)
    xd = torch.from_numpy(x).cuda()
    feat, ol, embd = e.audio_features(xd, torch.from_numpy(mask).cuda(), projector=pr, return_embd=True)
    torch.cuda.synchronize()
    assert feat.is_cuda and tuple(feat.shape) == (n_tot, 512) and tuple(embd.shape) == (n_tot, 256)
    assert list(ol) == list(wol) == [750, 182, 8]
    assert _same_bits(feat, wf) and _same_bits(embd, wm)
    feat2, ol2 = e.audio_features(xd, torch.from_numpy(mask).cuda(), projector=pr)
    torch.cuda.synchronize()
    assert _same_bits(feat2, wf) and list(ol2) == list(ol)
    hfeat, hol, hembd = e.audio_features(x, mask, projector=pr, return_embd=True)
    assert isinstance(hfeat, np.ndarray) and hfeat.shape == (n_tot, 512) and list(hol) == list(ol)
    assert np.array_equal(hfeat.view(np.int32), wf.cpu().numpy().view(np.int32))
    assert np.array_equal(hembd.view(np.int32), wm.cpu().numpy().view(np.int32))
    # no mask: every clip has mel_valid_lengths' rows of L frames
    feat3, ol3 = e.audio_features(xd, projector=pr)
    torch.cuda.synchronize()
    assert list(ol3) == [750] * 3 and tuple(feat3.shape) == (3 * 750, 512)


# ---------------------------------------------------------------- 7, 8. full width: the 8-row form, oracle parity
def test_full_width_bits_and_oracle(engines, projectors, projector_path, make_clip):
    """D = 1280, Q4_K with a Q4_K projector 1280 -> 4096: 1057 rows, so the last 8-row workgroup holds one row. Bits
    against the composition, and feature rows 0, 17, 34, ... against the CPU oracle's ggml MUL_MAT + bias with
    tests/test_projector.py's bars."""
    e, pr = engines("full", "q4_k"), projectors(1280, 4096, "q4_k")
    clips = [make_clip(c, 480000) for c in range(3)]
    lens = [250, 365, 1500]
    n_tot = 1057
    wfeat, wembd, wol, _ = _composition(e, pr, clips, key_len=lens)
    feat, embd, ol, _ = _features(e, pr, clips, n_tot, key_len=lens)
    assert list(ol) == list(wol) == [125, 182, 750] and n_tot % 8 == 1
    assert _same_bits(embd, wembd)
    assert _same_bits(feat, wfeat)
    mf = ggmlfile.read(projector_path(1280, 4096, "q4_k"))
    w = np.ascontiguousarray(mf.t("multi_modal_projector.linear.weight").data)
    bias = mf.t("multi_modal_projector.linear.bias").as_f32().reshape(-1)
    sel = np.arange(0, n_tot, 17)
    ref = oracle_py.gemm(mf.wtype, w, embd.cpu().numpy()[sel], 4096) + bias[None, :]
    mx, l2 = rel_errors(feat.cpu().numpy()[sel], ref)
    print(f"audio features vs oracle: max-rel {mx:.3e}, rel-L2 {l2:.3e}")
    assert mx < 1e-5 and l2 < 1e-6, (mx, l2)


# ---------------------------------------------------------------- 9. the operand hook
HOOK_LENS = [2, 17, 365, 1500]


@pytest.fixture(scope="module")
def hook_rows(engines):
    """realistic_rows packed for HOOK_LENS, and test_pool_ln of the same rows placed in windows, on the valid rows."""
    import q2a
    e = engines("tiny", "f16")
    D = e.info.n_audio_state
    m_tot, rs = q2a.varlen_rows(HOOK_LENS, T)
    x = oc.realistic_rows(m_tot, D, seed=4)
    win = np.zeros((len(HOOK_LENS) * T, D), dtype=np.float32)
    for c in range(len(HOOK_LENS)):
        win[c * T:c * T + rs[c + 1] - rs[c]] = x[rs[c]:rs[c + 1]]
    wd = torch.from_numpy(win).cuda()
    out = torch.full((len(HOOK_LENS),) + e.out_shape, float("nan"), device="cuda")
    e.test_pool_ln(wd.data_ptr(), len(HOOK_LENS), out.data_ptr())
    torch.cuda.synchronize()
    want = torch.cat([out[c, :L // 2] for c, L in enumerate(HOOK_LENS)]).cpu().numpy()
    assert np.isfinite(want).all() and want.shape[0] == q2a.packed_out_rows(HOOK_LENS)[0] == 941
    return e, torch.from_numpy(x).cuda(), want


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_pool_operand_hook(hook_rows, mode):
    e, xd, want = hook_rows
    N, D = want.shape
    ld = (N + 255) // 256 * 256
    blk = {0: 0, 1: 256, 2: 32}[mode]
    nblk = D // blk if blk else 1
    embd = torch.full((N + SENTINEL_ROWS, D), oc.SENTINEL32, dtype=torch.int32, device="cuda")
    codes = torch.full((N + SENTINEL_ROWS, D), oc.SENTINEL16, dtype=torch.int16, device="cuda")
    dy = torch.full((nblk, ld), oc.SENTINEL32, dtype=torch.int32, device="cuda")
    aext = torch.full((max(D // 256, 1), ld, 16), oc.SENTINEL16, dtype=torch.int16, device="cuda")
    e.test_pool_operand(mode, xd.data_ptr(), len(HOOK_LENS), HOOK_LENS, embd_ptr=embd.data_ptr(), codes_ptr=codes.data_ptr(),
                        dy_ptr=dy.data_ptr(), aext_ptr=aext.data_ptr(), ld=ld)
    torch.cuda.synchronize()
    embd, codes = embd.cpu().numpy(), codes.cpu().numpy().view(np.uint16)
    dy, aext = dy.cpu().numpy(), aext.cpu().numpy().view(np.uint16)
    assert (embd[N:] == oc.SENTINEL32).all() and (codes[N:] == oc.SENTINEL16).all(), "rows behind N_tot were written"
    assert np.array_equal(embd[:N], want.view(np.int32)), "embd differs from test_pool_ln's rows"
    y = embd[:N].view(np.float32)
    if mode == 0:
        assert np.array_equal(codes[:N], oc.fp16_bits(y))
        assert (dy == oc.SENTINEL32).all() and (aext == oc.SENTINEL16).all()
        return
    assert (dy[:, N:] == oc.SENTINEL32).all(), "d behind row N_tot was written"
    assert (dy[:, :N] != oc.SENTINEL32).all(), "a block scale was never written"
    got = {"codes": oc.decode_codes(codes[:N]), "d": oc.decode_d(dy.view(np.float32), N)}
    if mode == 1:
        assert (aext[:, N:] == oc.SENTINEL16).all(), "block sums behind row N_tot were written"
        got["hi"], got["lo"] = oc.decode_bsum(aext, N)
        oc.check_q8k(got, y, "pool + Q8_K")
    else:
        assert (aext == oc.SENTINEL16).all()
        oc.check_q80(got, y, "pool + Q8_0")
    # the f32 rows alone (no operand): the same bits
    only = torch.full((N + SENTINEL_ROWS, D), oc.SENTINEL32, dtype=torch.int32, device="cuda")
    e.test_pool_operand(mode, xd.data_ptr(), len(HOOK_LENS), HOOK_LENS, embd_ptr=only.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(only.cpu().numpy(), embd)


# ---------------------------------------------------------------- launch structure
PROF_CLASSES = ["mel", "conv1", "conv2", "ln", "gemm_qkv", "attn", "quant", "gemm_o", "gemm_fc1", "gemm_fc2", "pool"]   # Q2A_PROF_*


def test_launches_of_the_audio_feature_call(engines, projectors, batch13):
    """By the engine's per-class profile counters (one count per launch): the variable-length encode's launches, with
    the gather and ONE pool launch in the pool class (the projector's GEMM is in no class); a batch without a valid row
    launches nothing at all."""
    import ctypes as C

    import q2a
    e, pr = engines("tiny", "q4_k"), projectors(256, 512, "q4_k")
    clips, lens, want_ol = batch13
    lib, h = q2a.lib(), C.c_void_p(e.h)
    L = e.info.n_audio_layer
    cnt = (C.c_int64 * len(PROF_CLASSES))()

    def counts(call):
        call()
        torch.cuda.synchronize()
        assert lib.q2a_profile_read(h, None, cnt, len(PROF_CLASSES), 1) == 0
        return dict(zip(PROF_CLASSES, cnt))

    want = {c: L for c in ("gemm_qkv", "attn", "gemm_o", "gemm_fc1", "gemm_fc2")}
    want.update(mel=1, conv1=1, conv2=1, ln=2 * L, quant=2 * L, pool=2)
    assert lib.q2a_profile_read(h, None, None, 0, 1) == 0
    assert lib.q2a_profile_enable(h, 1) == 0
    try:
        assert counts(lambda: _features(e, pr, clips, sum(want_ol), key_len=lens)) == want
        short = clips[SKIP_AT]
        assert counts(lambda: _features(e, pr, [short, short[:4000]], 0)) == {c: 0 for c in PROF_CLASSES}
        # every key length 1: rows in the packed stream, none in the output
        assert counts(lambda: _features(e, pr, clips[:2], 0, key_len=[1, 1])) == {c: 0 for c in PROF_CLASSES}
    finally:
        lib.q2a_profile_enable(h, 0)
        lib.q2a_profile_read(h, None, None, 0, 1)


# ---------------------------------------------------------------- 10. errors: nothing is launched or written
def test_audio_features_arguments(engines, projectors, make_clip):
    import q2a
    e, pr = engines("tiny", "f16"), projectors(256, 512, "f16")
    clip = make_clip(0, 160000)
    pcm = torch.from_numpy(clip).cuda()
    n_tot = q2a.valid_lengths(len(clip))[1]
    feat = torch.full((n_tot, 512), 7.0, device="cuda")
    embd = torch.full((n_tot, 256), 7.0, device="cuda")

    def call(eng=e, p=pr, f=feat, m=embd, cap=n_tot, kl=None, clips=None):
        x, stride, ns = (pcm, len(clip), [len(clip)]) if clips is None else _pcm_batch(clips)
        return eng.audio_features_device(x.data_ptr(), stride, ns, f.data_ptr() if f is not None else 0,
                                         m.data_ptr() if m is not None else 0, cap, projector=p, key_len=kl)

    def untouched():
        torch.cuda.synchronize()
        return bool((feat == 7.0).all() and (embd == 7.0).all())

    wrong = projectors(512, 512, "f16")   # d_in is not n_audio_state
    for kw in (dict(cap=n_tot - 1), dict(p=wrong), dict(f=None), dict(p=None, f=None, m=None), dict(p=None),
               dict(kl=[0]), dict(kl=[T + 1])):
        with pytest.raises(q2a.Q2AError) as ei:
            call(**kw)
        assert ei.value.rc == -4, kw
        assert untouched(), kw
    with pytest.raises(q2a.Q2AError) as ei:
        e.audio_features_host([clip], projector=pr, rows_cap=n_tot - 1)
    assert ei.value.rc == -4
    # the bf16 activation contract has no packed kernel
    with pytest.raises(q2a.Q2AError) as ei:
        call(eng=engines("tiny", "f16", q2a.ACT_BF16))
    assert ei.value.rc == -6 and untouched()
    # skipped clips only: Q2A_OK, no rows, nothing written
    ol, st = call(clips=[clip[:8000], clip[:4000]], kl=None)
    assert list(ol) == [0, 0] and list(st) == [q2a.CLIP_SKIPPED] * 2 and untouched()
    # and the call itself works with these buffers
    ol, st = call()
    torch.cuda.synchronize()
    assert list(ol) == [n_tot] and torch.isfinite(feat).all() and torch.isfinite(embd).all() and not (embd == 7.0).all()
