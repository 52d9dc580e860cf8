"""inputs_embeds on the device: the row map derived from input_ids (q2a_test_audio_token_rows), the text-row gather
(q2a_test_embed_gather), and the calls that do both around the projector GEMM's row-map epilogue
(q2a_inputs_embeds_device / _device_mel, q2a_projector_apply_ids, Engine.inputs_embeds).

Every comparison is exact, on integer views. The map is compared with the host twin (itself held against
numpy.flatnonzero in tests/test_audio_token_rows_cpu.py); the gather is a byte copy of table[ids]; the audio rows are the
existing f32 audio_features cast by torch on the CPU, as in tests/test_gpu_features_to.py, and bit for bit what
Projector.apply_to stores given the explicit map. Every destination starts as that file's sentinel pattern with guard
rows and ld > d_out, so everything that must stay untouched is compared too. All tests need an MI355X."""
import os
import subprocess

import numpy as np
import pytest

from conftest import TOOL

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

S16, S32 = 0x5A5A, 0x5A5A5A5A   # the sentinel bit patterns of tests/test_gpu_features_to.py
ERR_ARG, ERR_UNSUPPORTED = -4, -6
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
AUDIO = 151646
FILL = -7
D_OUT = 256
CHUNK = 2048                    # the compaction's tokens per workgroup (csrc/q2a_internal.h, Q2A_IDS_CHUNK)


def _dt(name):
    import q2a
    return {"bf16": q2a.DT_BF16, "f16": q2a.DT_F16, "f32": q2a.DT_F32}[name]


def _ibits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _sentinel(rows, ld, dtype):
    if dtype == torch.float32:
        return torch.full((rows, ld), S32, dtype=torch.int32, device="cuda").view(torch.float32)
    return torch.full((rows, ld), S16, dtype=torch.int16, device="cuda").view(dtype)


def _sent_value(dtype):
    return S32 if dtype == torch.float32 else S16


def _want_buffer(like, rows):
    """The expected integer image of a destination: the sentinel everywhere, then rows = [(row indices, [k][d_out] CPU
    tensor of the destination's dtype), ...] written into columns 0 .. d_out-1, in order."""
    want = torch.full_like(_ibits(like.cpu()), _sent_value(like.dtype))
    for idx, vals in rows:
        idx = torch.as_tensor(np.asarray(idx, dtype=np.int64))
        if len(idx):
            want[idx, :vals.shape[1]] = _ibits(vals)
    return want


def _assert_same(dst, want, what):
    got = _ibits(dst.cpu())
    if not torch.equal(got, want):
        bad = got != want
        r, c = [int(v[0]) for v in torch.nonzero(bad, as_tuple=True)]
        raise AssertionError(f"{what}: {int(bad.sum())} elements differ, first at row {r} column {c}: "
                             f"got {int(got[r, c]) & 0xFFFFFFFF:#x}, want {int(want[r, c]) & 0xFFFFFFFF:#x}")


# ---------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def projectors(host_build, workdir):
    import q2a
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    cache = {}

    def get(wt, d_in=256, d_out=D_OUT):
        if (wt, d_in, d_out) not in cache:
            base = os.path.join(workdir, f"proj-{d_in}x{d_out}-f16.bin")
            if not os.path.exists(base):
                subprocess.check_call([TOOL, "gen-projector", base, str(d_in), str(d_out), "f16", "0x51A2"])
            path = base
            if wt != "f16":
                path = os.path.join(workdir, f"proj-{d_in}x{d_out}-{wt}.bin")
                if not os.path.exists(path):
                    subprocess.check_call([TOOL, "quantize", base, path, wt, "8"])
            cache[(wt, d_in, d_out)] = q2a.Projector(path, device=0)
        return cache[(wt, d_in, d_out)]

    yield get
    for p in cache.values():
        p.close()


@pytest.fixture(scope="module")
def engines(make_model):
    import q2a
    cache = {}

    def get(wt, act=0):
        if (wt, act) not in cache:
            cache[(wt, act)] = q2a.Engine(make_model("tiny", wt), device=0, act=act)
        return cache[(wt, act)]

    yield get
    for e in cache.values():
        e.close()


# ---------------------------------------------------------------- 1. the compaction alone
N_TOKENS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 70001]
PATTERNS = ["none", "all", "first", "last", "edges", "bernoulli"]


def _pattern_ids(n, pattern, np_dtype):
    """n text ids in 0 .. 999 with the audio id where the pattern says. int64 text ids also get high words set, a few
    of them over the audio id's own low word: those must not match."""
    rng = np.random.default_rng(1000 + n)
    ids = rng.integers(0, 1000, size=n).astype(np_dtype)
    if np_dtype == np.int64:
        decoy = rng.random(n) < 0.05
        ids[decoy] = AUDIO + (rng.integers(1, 1 << 30, size=int(decoy.sum())) << 32) * rng.choice([-1, 1], size=int(decoy.sum()))
    hit = np.zeros(n, dtype=bool)
    if pattern == "all":
        hit[:] = True
    elif pattern == "first":
        hit[0] = True
    elif pattern == "last":
        hit[-1] = True
    elif pattern == "edges":      # every multiple of 64 (hence of every power-of-two chunk up to 4096) and its neighbours
        e = np.arange(0, n + 64, 64)
        for d in (-1, 0, 1):
            p = e + d
            hit[p[(p >= 0) & (p < n)]] = True
    elif pattern == "bernoulli":
        hit = rng.random(n) < 0.3
    else:
        assert pattern == "none"
    ids[hit] = AUDIO
    return ids


@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("n", N_TOKENS)
def test_compaction_against_the_host_twin(projectors, n, width):
    import q2a
    pr = projectors("f16")
    np_dtype = np.int32 if width == 4 else np.int64
    assert CHUNK in (64, 256, 1024, 2048, 4096)
    for pattern in PATTERNS:
        ids = _pattern_ids(n, pattern, np_dtype)
        count, _ = q2a.audio_token_rows(ids, AUDIO)
        assert count == int((ids == AUDIO).sum())
        if width == 8 and n >= 255 and pattern != "all":   # some ids carry the audio id's low word under another high word
            assert int(((ids & 0xFFFFFFFF) == AUDIO).sum()) > count
        ids_dev = torch.from_numpy(ids).cuda()
        for n_feat in sorted({0, max(count - 1, 0), count, count + 1, count + 300}):
            _, want = q2a.audio_token_rows(ids, AUDIO, map_cap=n_feat)
            got = torch.full((n_feat + 4,), FILL, dtype=torch.int32, device="cuda")
            report = torch.full((4,), FILL, dtype=torch.int32, device="cuda")
            pr.test_audio_token_rows(ids_dev.data_ptr(), width, n, AUDIO, n_feat, got.data_ptr(), report.data_ptr())
            torch.cuda.synchronize()
            got = got.cpu().numpy()
            what = (n, width, pattern, n_feat)
            assert np.array_equal(got[:n_feat], want), what
            assert np.all(got[n_feat:] == FILL), what           # the words behind n_feat stay untouched
            if n_feat > count:
                assert np.all(got[count:n_feat] == -1), what    # the -1 tail
            assert report.cpu().tolist() == [count, n_feat, 0, int(count != n_feat)], what


def test_compaction_arguments(projectors):
    import q2a
    pr = projectors("f16")
    ids = torch.zeros(64, dtype=torch.int64, device="cuda")
    got = torch.full((8,), FILL, dtype=torch.int32, device="cuda")
    report = torch.full((4,), FILL, dtype=torch.int32, device="cuda")
    good = dict(ids_ptr=ids.data_ptr(), ids_width=8, n_tokens=64, audio_token_id=AUDIO, n_feat=8, row_map_ptr=got.data_ptr(),
                report_ptr=report.data_ptr())
    for kw in (dict(ids_width=2), dict(n_tokens=0), dict(n_tokens=(1 << 24) + 1), dict(ids_ptr=0), dict(ids_ptr=ids.data_ptr() + 4),
               dict(n_feat=-1), dict(row_map_ptr=0), dict(report_ptr=0)):
        with pytest.raises(q2a.Q2AError) as ei:
            pr.test_audio_token_rows(**dict(good, **kw))
        assert ei.value.rc == ERR_ARG, kw
    torch.cuda.synchronize()
    assert bool((got == FILL).all()) and bool((report == FILL).all())


# ---------------------------------------------------------------- 2. the gather alone
def _table(vocab, ld, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((vocab, ld), generator=g).to(dtype)


@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_gather_alone(dt, width):
    import q2a
    dtype = DTYPES[dt]
    vocab, d_out, table_ld, ld, n, guard = 301, D_OUT, D_OUT + 8, D_OUT + 64, 1237, 3
    audio = 7                      # inside the table's range: its row must still not be copied
    rng = np.random.default_rng(31 + width)
    ids = rng.integers(0, vocab, size=n).astype(np.int32 if width == 4 else np.int64)
    ids[rng.random(n) < 0.2] = audio
    bad_at = [0, 5, 64, 700, n - 1]
    ids[bad_at] = [-1, vocab, vocab + 1000, np.iinfo(ids.dtype).min, np.iinfo(ids.dtype).max]
    if width == 8:
        ids[9] = 3 + (1 << 32)     # a valid low word under a high word: outside the table
        ids[10] = audio + (1 << 32)   # the audio id's low word: not the audio id, and outside the table
        bad_at += [9, 10]
    ids[[1, 2]] = [0, vocab - 1]
    table = _table(vocab, table_ld, dtype, 77)
    tab_dev = table.cuda()
    dst = _sentinel(n + guard, ld, dtype)
    report = torch.full((4,), FILL, dtype=torch.int32, device="cuda")
    ids_dev = torch.from_numpy(ids).cuda()
    src = q2a.embeds_src(ids_dev.data_ptr(), width, n, audio, tab_dev.data_ptr(), vocab, table_ld, report.data_ptr())
    q2a.test_embed_gather(src, q2a.feat_dst(dst.data_ptr(), ld, n, _dt(dt)), d_out)
    torch.cuda.synchronize()
    text = np.flatnonzero((ids != audio) & (ids >= 0) & (ids < vocab))
    assert len(text) + len(bad_at) + int((ids == audio).sum()) == n
    want = _want_buffer(dst, [(text, table[torch.from_numpy(ids[text].astype(np.int64)), :d_out])])
    _assert_same(dst, want, f"gather {dt} width {width}")
    assert report.cpu().tolist() == [0, 0, len(bad_at), 2]
    # no bad id: the counter and the flag stay 0
    ids_ok = torch.from_numpy(np.where((ids >= 0) & (ids < vocab), ids, 1).astype(ids.dtype)).cuda()
    src = q2a.embeds_src(ids_ok.data_ptr(), width, n, audio, tab_dev.data_ptr(), vocab, table_ld, report.data_ptr())
    q2a.test_embed_gather(src, q2a.feat_dst(dst.data_ptr(), ld, n, _dt(dt)), d_out)
    torch.cuda.synchronize()
    assert report.cpu().tolist() == [0, 0, 0, 0]


# ---------------------------------------------------------------- 3. the whole call
FRAMES = [3000, 500, 74, 1]          # valid mel frames per clip -> key lengths 1500, 250, 37, 1
KEY_LENS = [1500, 250, 37, 1]
OUT_LENS = [750, 125, 18, 0]
N_FEAT = sum(OUT_LENS)               # 893
SEQ, N_SEQ = 320, 3
N_TOK = SEQ * N_SEQ                  # 960 = 893 audio + 67 text positions
VOCAB, TABLE_LD, LD, GUARD = 300, D_OUT + 8, D_OUT + 64, 3


def _layout_ids(np_dtype=np.int64):
    """input_ids [N_SEQ][SEQ] flat: clip 0's 750 audio tokens at 0 .. 750 with a text token at 5 (a split run, crossing
    two sequence ends), ten text tokens, clip 1's 125 at 761 .. 885, 56 text tokens, clip 2's 18 at the very end — clips
    1 and 2 lie in the last sequence, audio tokens sit at flat positions 0 and n - 1."""
    rng = np.random.default_rng(3)
    ids = rng.integers(0, VOCAB, size=N_TOK).astype(np_dtype)
    hit = np.zeros(N_TOK, dtype=bool)
    hit[0:751] = True
    hit[5] = False
    hit[761:886] = True
    hit[N_TOK - 18:] = True
    assert hit.sum() == N_FEAT and hit[0] and hit[-1] and 761 // SEQ == (N_TOK - 1) // SEQ == 2
    ids[hit] = AUDIO
    return ids


@pytest.fixture(scope="module")
def mel4(engines, make_clip):
    """input_features [4][n_mels][3000] on the device and the mask of FRAMES; computed once, left unchanged."""
    e = engines("f16")
    L = 3000
    x = np.stack([e.pcm_to_mel(make_clip(c % 3, 480000))[:, :L] for c in range(4)])
    mask = np.zeros((4, L), dtype=np.int64)
    for c, n in enumerate(FRAMES):
        mask[c, :n] = 1
    return torch.from_numpy(x).cuda(), torch.from_numpy(mask).cuda()


@pytest.fixture(scope="module")
def f32_features(engines, projectors, mel4):
    """The existing packed f32 audio_features per (engine type, projector type), on the CPU; computed once."""
    cache = {}

    def get(ewt, pwt):
        if (ewt, pwt) not in cache:
            feat, ol = engines(ewt).audio_features(mel4[0], mel4[1], projector=projectors(pwt))
            torch.cuda.synchronize()
            assert list(ol) == OUT_LENS and feat.shape == (N_FEAT, D_OUT) and feat.dtype == torch.float32
            cache[(ewt, pwt)] = feat.cpu()
        return cache[(ewt, pwt)]
    return get


def _mel_call(e, pr, mel4, dst, src, key_len=KEY_LENS, **kw):
    x = mel4[0]
    B, M, L = x.shape
    return e.inputs_embeds_device_mel(x.data_ptr(), M * L, L, [L] * B, dst, src, pr, key_len=key_len, **kw)


WHOLE = [(ewt, pwt, dt) for ewt in ("f16", "q4_k") for pwt in ("f16", "q4_k") for dt in ("bf16", "f16", "f32")]


@pytest.mark.parametrize("ewt,pwt,dt", WHOLE, ids=["-".join(c) for c in WHOLE])
def test_whole_call(engines, projectors, mel4, f32_features, ewt, pwt, dt):
    import q2a
    e, pr = engines(ewt), projectors(pwt)
    dtype = DTYPES[dt]
    width = 8 if dt != "f16" else 4
    ids = _layout_ids(np.int64 if width == 8 else np.int32)
    table = _table(VOCAB, TABLE_LD, dtype, 5)
    tab_dev, ids_dev = table.cuda(), torch.from_numpy(ids).cuda()
    dst = _sentinel(N_TOK + GUARD, LD, dtype)
    report = torch.full((4,), FILL, dtype=torch.int32, device="cuda")
    src = q2a.embeds_src(ids_dev.data_ptr(), width, N_TOK, AUDIO, tab_dev.data_ptr(), VOCAB, TABLE_LD, report.data_ptr())
    fd = q2a.feat_dst(dst.data_ptr(), LD, N_TOK, _dt(dt))
    ol, st = _mel_call(e, pr, mel4, fd, src)
    torch.cuda.synchronize()
    assert list(ol) == OUT_LENS and list(st) == [q2a.CLIP_ENCODED] * 4
    assert report.cpu().tolist() == [N_FEAT, N_FEAT, 0, 0]
    # table[ids] with the audio positions overwritten by the f32 features cast on the CPU; sentinel everywhere else
    audio_at, text_at = np.flatnonzero(ids == AUDIO), np.flatnonzero(ids != AUDIO)
    want = _want_buffer(dst, [(text_at, table[torch.from_numpy(ids[text_at].astype(np.int64)), :D_OUT]),
                              (audio_at, f32_features(ewt, pwt).to(dtype))])
    _assert_same(dst, want, f"inputs_embeds {ewt} {pwt} {dt}")
    # bit for bit the existing pieces: the packed embd_enc of audio_features_device_mel_to through Projector.apply_to with
    # the explicit map, over a torch gather of the text rows
    x = mel4[0]
    B, M, L = x.shape
    embd = torch.empty((N_FEAT, e.info.n_audio_state), device="cuda")
    scratch = _sentinel(N_FEAT, D_OUT, dtype)
    e.audio_features_device_mel_to(x.data_ptr(), M * L, L, [L] * B, q2a.feat_dst(scratch.data_ptr(), D_OUT, N_FEAT, _dt(dt)), pr,
                                   embd_ptr=embd.data_ptr(), embd_rows_cap=N_FEAT, key_len=KEY_LENS)
    ref = _sentinel(N_TOK + GUARD, LD, dtype)
    ref[torch.from_numpy(text_at).cuda(), :D_OUT] = tab_dev[torch.from_numpy(ids[text_at].astype(np.int64)).cuda(), :D_OUT]
    row_map = torch.from_numpy(audio_at.astype(np.int32)).cuda()
    pr.apply_to(embd.data_ptr(), N_FEAT, q2a.feat_dst(ref.data_ptr(), LD, N_TOK, _dt(dt)), row_map.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(_ibits(dst), _ibits(ref)), "not the bits of apply_to with the explicit map"
    # and Projector.apply_ids on those rows: the same buffer once more
    dst2 = _sentinel(N_TOK + GUARD, LD, dtype)
    report.fill_(FILL)
    pr.apply_ids(embd.data_ptr(), N_FEAT, q2a.feat_dst(dst2.data_ptr(), LD, N_TOK, _dt(dt)), src)
    torch.cuda.synchronize()
    assert torch.equal(_ibits(dst2), _ibits(ref)) and report.cpu().tolist() == [N_FEAT, N_FEAT, 0, 0]


def test_without_a_table_and_without_a_report(engines, projectors, mel4, f32_features):
    """embed_table NULL: the text rows keep the sentinel; report_dev NULL: the call needs none."""
    import q2a
    e, pr = engines("q4_k"), projectors("q4_k")
    ids = _layout_ids()
    ids_dev = torch.from_numpy(ids).cuda()
    dst = _sentinel(N_TOK + GUARD, LD, torch.bfloat16)
    src = q2a.embeds_src(ids_dev.data_ptr(), 8, N_TOK, AUDIO)
    ol, _ = _mel_call(e, pr, mel4, q2a.feat_dst(dst.data_ptr(), LD, N_TOK, q2a.DT_BF16), src)
    torch.cuda.synchronize()
    assert list(ol) == OUT_LENS
    _assert_same(dst, _want_buffer(dst, [(np.flatnonzero(ids == AUDIO), f32_features("q4_k", "q4_k").to(torch.bfloat16))]), "no table")


# ---------------------------------------------------------------- 4. PCM against mel
def test_pcm_entry_point_equals_the_mel_entry_point(engines, projectors, make_clip):
    import q2a
    e, pr = engines("q4_k"), projectors("q4_k")
    clips = [make_clip(0, 480000), make_clip(1, 160000)]
    kl = [365, 33]
    n_feat = sum(k // 2 for k in kl)
    n_tok = n_feat + 9
    ids = np.random.default_rng(8).integers(0, VOCAB, size=n_tok).astype(np.int64)
    ids[np.random.default_rng(9).permutation(n_tok)[:n_feat]] = AUDIO
    table = _table(VOCAB, TABLE_LD, torch.bfloat16, 6).cuda()
    ids_dev = torch.from_numpy(ids).cuda()
    outs = []
    for kind in ("pcm", "mel"):
        dst = _sentinel(n_tok + GUARD, LD, torch.bfloat16)
        report = torch.full((4,), FILL, dtype=torch.int32, device="cuda")
        src = q2a.embeds_src(ids_dev.data_ptr(), 8, n_tok, AUDIO, table.data_ptr(), VOCAB, TABLE_LD, report.data_ptr())
        fd = q2a.feat_dst(dst.data_ptr(), LD, n_tok, q2a.DT_BF16)
        if kind == "pcm":
            stride = max(len(c) for c in clips)
            pcm = torch.zeros(len(clips), stride)
            for i, c in enumerate(clips):
                pcm[i, :len(c)] = torch.from_numpy(np.ascontiguousarray(c))
            pcm = pcm.cuda()
            ol, st = e.inputs_embeds_device(pcm.data_ptr(), stride, [len(c) for c in clips], fd, src, pr, key_len=kl)
        else:
            mels = [e.pcm_to_mel(c) for c in clips]
            ld = max(m.shape[1] for m in mels)
            mel = np.zeros((len(clips), mels[0].shape[0], ld), dtype=np.float32)
            for i, m in enumerate(mels):
                mel[i, :, :m.shape[1]] = m
            md = torch.from_numpy(mel).cuda()
            ol, st = e.inputs_embeds_device_mel(md.data_ptr(), mel.shape[1] * ld, ld, [m.shape[1] for m in mels], fd, src, pr,
                                                key_len=kl)
        torch.cuda.synchronize()
        assert list(ol) == [k // 2 for k in kl] and report.cpu().tolist() == [n_feat, n_feat, 0, 0]
        outs.append(_ibits(dst.cpu()))
    assert torch.equal(outs[0], outs[1])
    assert bool((outs[0][torch.from_numpy(np.flatnonzero(ids == AUDIO)), :D_OUT] != S16).any())


# ---------------------------------------------------------------- 5. count mismatch
@pytest.mark.parametrize("kind", ["one-too-few", "one-too-many"])
def test_count_mismatch(engines, projectors, mel4, f32_features, kind):
    import q2a
    e, pr = engines("q4_k"), projectors("q4_k")
    ids = _layout_ids()
    if kind == "one-too-few":
        ids[400] = 11                       # an audio token of clip 0 turned into text: the last feature row is dropped
    else:
        ids[755] = AUDIO                    # one more, between clips 0 and 1: the last audio position gets no row
    audio_at = np.flatnonzero(ids == AUDIO)
    found = len(audio_at)
    assert found == N_FEAT + (-1 if kind == "one-too-few" else 1)
    placed = min(found, N_FEAT)
    table = _table(VOCAB, TABLE_LD, torch.bfloat16, 5)
    tab_dev, ids_dev = table.cuda(), torch.from_numpy(ids).cuda()
    dst = _sentinel(N_TOK + GUARD, LD, torch.bfloat16)
    report = torch.full((4,), FILL, dtype=torch.int32, device="cuda")
    src = q2a.embeds_src(ids_dev.data_ptr(), 8, N_TOK, AUDIO, tab_dev.data_ptr(), VOCAB, TABLE_LD, report.data_ptr())
    ol, _ = _mel_call(e, pr, mel4, q2a.feat_dst(dst.data_ptr(), LD, N_TOK, q2a.DT_BF16), src)
    torch.cuda.synchronize()
    assert list(ol) == OUT_LENS
    assert report.cpu().tolist() == [found, N_FEAT, 0, 1]
    # the first min(found, rows) pairs are placed; a further audio position keeps the sentinel; text rows are text
    text_at = np.flatnonzero(ids != AUDIO)
    want = _want_buffer(dst, [(text_at, table[torch.from_numpy(ids[text_at]), :D_OUT]),
                              (audio_at[:placed], f32_features("q4_k", "q4_k")[:placed].to(torch.bfloat16))])
    _assert_same(dst, want, kind)
    # Engine.inputs_embeds: check=True raises, check=False hands the report back without reading it
    ids2 = ids_dev.view(N_SEQ, SEQ)
    tab = tab_dev[:, :D_OUT]                 # rows strided by TABLE_LD
    with pytest.raises(ValueError, match="audio tokens"):
        e.inputs_embeds(mel4[0], mel4[1], ids2, AUDIO, pr, embed_tokens=tab)
    out, ol, rep = e.inputs_embeds(mel4[0], mel4[1], ids2, AUDIO, pr, embed_tokens=tab, check=False)
    torch.cuda.synchronize()
    assert rep.cpu().tolist() == [found, N_FEAT, 0, 1] and out.shape == (N_SEQ, SEQ, D_OUT) and out.dtype == torch.bfloat16


def test_python_inputs_embeds(engines, projectors, mel4, f32_features):
    import q2a
    e, pr = engines("f16"), projectors("q4_k")
    ids = _layout_ids()
    table = _table(VOCAB, D_OUT, torch.float16, 12)
    tab_dev = table.cuda()
    ids_dev = torch.from_numpy(ids).cuda().view(N_SEQ, SEQ)
    out, ol, rep = e.inputs_embeds(mel4[0], mel4[1], ids_dev, AUDIO, pr, embed_tokens=tab_dev)
    torch.cuda.synchronize()
    assert out.shape == (N_SEQ, SEQ, D_OUT) and out.dtype == torch.float16 and list(ol) == OUT_LENS
    assert rep.cpu().tolist() == [N_FEAT, N_FEAT, 0, 0]
    want = table[torch.from_numpy(np.where(ids == AUDIO, 0, ids))].clone()
    want[torch.from_numpy(np.flatnonzero(ids == AUDIO))] = f32_features("f16", "q4_k").to(torch.float16)
    assert torch.equal(_ibits(out.cpu().view(N_TOK, D_OUT)), _ibits(want))
    # int32 ids into a caller's buffer; a bad text id raises under check=True
    mine = _sentinel(N_TOK, D_OUT, torch.float16).view(N_SEQ, SEQ, D_OUT)
    out2, _, _ = e.inputs_embeds(mel4[0], mel4[1], ids_dev.to(torch.int32), AUDIO, pr, embed_tokens=tab_dev, out=mine)
    torch.cuda.synchronize()
    assert out2 is mine and torch.equal(_ibits(mine.cpu().view(N_TOK, D_OUT)), _ibits(want))
    bad = ids_dev.clone()
    bad[0, 5] = VOCAB
    with pytest.raises(ValueError, match="outside the embedding table"):
        e.inputs_embeds(mel4[0], mel4[1], bad, AUDIO, pr, embed_tokens=tab_dev)
    for kw in (dict(embed_tokens=tab_dev.to(torch.bfloat16), out=mine), dict(embed_tokens=tab_dev[:, :128]),
               dict(out=mine[:, :, :128]), dict(out=mine.view(N_TOK, D_OUT))):
        with pytest.raises(ValueError):
            e.inputs_embeds(mel4[0], mel4[1], ids_dev, AUDIO, pr, **kw)


# ---------------------------------------------------------------- 6. no valid audio row
PROF_CLASSES = ["mel", "conv1", "conv2", "ln", "gemm_qkv", "attn", "quant", "gemm_o", "gemm_fc1", "gemm_fc2", "pool"]   # Q2A_PROF_*


@pytest.mark.parametrize("n_audio", [0, 3])
def test_no_valid_audio_row(engines, projectors, mel4, n_audio):
    """Every key length 1: no feature row, no encoder kernel; the text rows are still gathered and the report is
    [count, 0, 0, count != 0]. By the profile counters (pool class: the compaction's two kernels are booked as one
    entry, the gather as another) nothing else is launched."""
    import ctypes as C

    import q2a
    e, pr = engines("q4_k"), projectors("q4_k")
    n_tok = 700
    ids = np.random.default_rng(4).integers(0, VOCAB, size=n_tok).astype(np.int64)
    ids[[0, 300, n_tok - 1][:n_audio]] = AUDIO
    table = _table(VOCAB, TABLE_LD, torch.bfloat16, 5)
    tab_dev, ids_dev = table.cuda(), torch.from_numpy(ids).cuda()
    dst = _sentinel(n_tok + GUARD, LD, torch.bfloat16)
    report = torch.full((4,), FILL, dtype=torch.int32, device="cuda")
    src = q2a.embeds_src(ids_dev.data_ptr(), 8, n_tok, AUDIO, tab_dev.data_ptr(), VOCAB, TABLE_LD, report.data_ptr())
    lib, h = q2a.lib(), C.c_void_p(e.h)
    cnt = (C.c_int64 * len(PROF_CLASSES))()
    assert lib.q2a_profile_read(h, None, None, 0, 1) == 0
    assert lib.q2a_profile_enable(h, 1) == 0
    try:
        ol, st = _mel_call(e, pr, mel4, q2a.feat_dst(dst.data_ptr(), LD, n_tok, q2a.DT_BF16), src, key_len=[1, 1, 1, 1])
        torch.cuda.synchronize()
        assert lib.q2a_profile_read(h, None, cnt, len(PROF_CLASSES), 1) == 0
    finally:
        lib.q2a_profile_enable(h, 0)
        lib.q2a_profile_read(h, None, None, 0, 1)
    assert dict(zip(PROF_CLASSES, cnt)) == dict({c: 0 for c in PROF_CLASSES}, pool=2)
    assert list(ol) == [0, 0, 0, 0]
    assert report.cpu().tolist() == [n_audio, 0, 0, int(n_audio != 0)]
    text_at = np.flatnonzero(ids != AUDIO)
    _assert_same(dst, _want_buffer(dst, [(text_at, table[torch.from_numpy(ids[text_at]), :D_OUT])]), "no valid audio row")


# ---------------------------------------------------------------- 7. errors: nothing is launched or written
def test_arguments(engines, projectors, mel4):
    import q2a
    e, pr = engines("f16"), projectors("f16")
    ids = _layout_ids()
    ids_dev = torch.from_numpy(ids).cuda()
    tab_dev = _table(VOCAB, TABLE_LD, torch.bfloat16, 5).cuda()
    dst = _sentinel(N_TOK + GUARD, LD, torch.bfloat16)
    report = torch.full((4,), FILL, dtype=torch.int32, device="cuda")
    embd = torch.full((N_FEAT, 256), S32, dtype=torch.int32, device="cuda").view(torch.float32)
    good_dst = dict(base=dst.data_ptr(), ld=LD, n_rows=N_TOK, dtype=q2a.DT_BF16)
    good_src = dict(ids_ptr=ids_dev.data_ptr(), ids_width=8, n_tokens=N_TOK, audio_token_id=AUDIO, table_ptr=tab_dev.data_ptr(),
                    vocab=VOCAB, table_ld=TABLE_LD, report_ptr=report.data_ptr())

    def call(eng=e, p=pr, d=None, s=None, no_src=False, no_dst=False, reserved=0, cap=N_FEAT):
        d, s = dict(good_dst, **(d or {})), dict(good_src, **(s or {}))
        fd = None if no_dst else q2a.feat_dst(d["base"], d["ld"], d["n_rows"], d["dtype"])
        sr = None if no_src else q2a.embeds_src(**s)
        if sr is not None:
            sr.reserved = reserved
        return _mel_call(eng, p, mel4, fd, sr, embd_ptr=embd.data_ptr(), embd_rows_cap=cap)

    def untouched():
        torch.cuda.synchronize()
        return bool((_ibits(dst) == S16).all() and (report == FILL).all() and (_ibits(embd) == S32).all())

    cases = {
        "no src": dict(no_src=True),
        "no dst": dict(no_dst=True),
        "no projector": dict(p=None),
        "ids_width 2": dict(s=dict(ids_width=2)),
        "reserved set": dict(reserved=1),
        "no input_ids": dict(s=dict(ids_ptr=0)),
        "misaligned input_ids": dict(s=dict(ids_ptr=ids_dev.data_ptr() + 4)),
        "n_tokens 0": dict(s=dict(n_tokens=0), d=dict(n_rows=0)),
        "n_tokens above 2^24": dict(s=dict(n_tokens=(1 << 24) + 1), d=dict(n_rows=(1 << 24) + 1)),
        "n_tokens != n_rows": dict(s=dict(n_tokens=N_TOK - 1)),
        "a misaligned table": dict(s=dict(table_ptr=tab_dev.data_ptr() + 2)),
        "table_ld < d_out": dict(s=dict(table_ld=D_OUT - 8)),
        "table_ld * 2 bytes not a multiple of 16": dict(s=dict(table_ld=D_OUT + 4)),
        "vocab 0": dict(s=dict(vocab=0)),
        "a misaligned base": dict(d=dict(base=dst.data_ptr() + 2)),
        "ld < d_out": dict(d=dict(ld=D_OUT - 8)),
        "a bad dtype": dict(d=dict(dtype=3)),
        "embd_rows_cap below N_tot": dict(cap=N_FEAT - 1),
    }
    for why, kw in cases.items():
        with pytest.raises(q2a.Q2AError) as ei:
            call(**kw)
        assert ei.value.rc == ERR_ARG, why
        assert untouched(), why
    # Projector.apply_ids makes the same checks of src
    x = torch.zeros((4, 256), device="cuda")
    for why, s in (("ids_width", dict(ids_width=3)), ("n_tokens", dict(n_tokens=N_TOK + 1)), ("table", dict(table_ld=D_OUT + 4))):
        with pytest.raises(q2a.Q2AError) as ei:
            pr.apply_ids(x.data_ptr(), 4, q2a.feat_dst(dst.data_ptr(), LD, N_TOK, q2a.DT_BF16), q2a.embeds_src(**dict(good_src, **s)))
        assert ei.value.rc == ERR_ARG and untouched(), why
    # the bf16 activation contract has no packed kernel
    with pytest.raises(q2a.Q2AError) as ei:
        call(eng=engines("f16", q2a.ACT_BF16))
    assert ei.value.rc == ERR_UNSUPPORTED and untouched()
    # and the call itself works with these buffers
    ol, _ = call()
    torch.cuda.synchronize()
    assert list(ol) == OUT_LENS and report.cpu().tolist() == [N_FEAT, N_FEAT, 0, 0]
    assert not bool((_ibits(dst[:N_TOK, :D_OUT]) == S16).all(dim=1).any()) and not bool((_ibits(embd) == S32).all())


# ---------------------------------------------------------------- 8. the projector's regime
def test_projector_regime_is_unchanged_by_src(projectors):
    """q2a_projector_regime answers for the row count alone; a call with src runs that GEMM: on a 256 -> 4096 projector
    at a row count of the 128-tile regime, apply_ids stores the bits of apply_to with the explicit map."""
    import q2a
    pr = projectors("q4_k", 256, 4096)
    M, n_tok = 1003, 1100
    before = pr.regime(M)
    assert before == q2a.REGIME_128
    rng = np.random.default_rng(21)
    ids = rng.integers(0, VOCAB, size=n_tok).astype(np.int64)
    ids[np.sort(rng.permutation(n_tok)[:M])] = AUDIO
    ids_dev = torch.from_numpy(ids).cuda()
    x = torch.randn((M, 256), device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    got, ref = _sentinel(n_tok + GUARD, 4096, torch.bfloat16), _sentinel(n_tok + GUARD, 4096, torch.bfloat16)
    report = torch.full((4,), FILL, dtype=torch.int32, device="cuda")
    pr.apply_ids(x.data_ptr(), M, q2a.feat_dst(got.data_ptr(), 4096, n_tok, q2a.DT_BF16),
                 q2a.embeds_src(ids_dev.data_ptr(), 8, n_tok, AUDIO, report_ptr=report.data_ptr()))
    assert pr.regime(M) == before
    rm = torch.from_numpy(np.flatnonzero(ids == AUDIO).astype(np.int32)).cuda()
    pr.apply_to(x.data_ptr(), M, q2a.feat_dst(ref.data_ptr(), 4096, n_tok, q2a.DT_BF16), rm.data_ptr())
    torch.cuda.synchronize()
    assert report.cpu().tolist() == [M, M, 0, 0]
    assert torch.equal(_ibits(got), _ibits(ref)) and not bool((_ibits(got[rm.long()]) == S16).all(dim=1).any())
