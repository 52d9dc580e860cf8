"""Audio features as f32 / fp16 / bf16 stored in place into the consumer's rows: the GEMM epilogue Q2A_EPI_STORE_ROWS
through Projector.apply_to, the engine entry points q2a_audio_features_device_to / _device_mel_to and
Engine.audio_features(out=...).

Every comparison is exact, on int16 / int32 views. The comparison data is the existing f32 path on the same inputs
(Projector.apply, q2a_audio_features_device), cast by torch on the CPU: the new epilogue stores the f32 call's value
rounded once more to nearest even, so nothing is left out and no tolerance is needed. Every destination starts as a
sentinel pattern, so rows and columns that must stay untouched are compared too. All tests need an MI355X."""
import os
import subprocess

import numpy as np
import pytest

from conftest import TOOL

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

T = 1500
S16, S32 = 0x5A5A, 0x5A5A5A5A   # sentinel bit patterns (bf16 / fp16 / f32: large finite values no projection produces)
ERR_ARG, ERR_UNSUPPORTED = -4, -6
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}


def _dt(name):
    import q2a
    return {"bf16": q2a.DT_BF16, "f16": q2a.DT_F16, "f32": q2a.DT_F32}[name]


def _ibits(t):
    """The integer view of a tensor's elements (int16 for the 16-bit types, int32 for f32)."""
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _sentinel(rows, ld, dtype):
    """[rows][ld] of the sentinel pattern, on the device."""
    if dtype == torch.float32:
        return torch.full((rows, ld), S32, dtype=torch.int32, device="cuda").view(torch.float32)
    return torch.full((rows, ld), S16, dtype=torch.int16, device="cuda").view(dtype)


def _sent_value(dtype):
    return S32 if dtype == torch.float32 else S16


def _check_dest(dst, want_rows, row_of, d_out, what, n_rows=None):
    """dst (device; n_rows rows, default all of it, then guard rows) holds want_rows[m] (CPU, already cast) at row
    row_of[m] for every m with row_of[m] in 0 .. n_rows-1, columns 0 .. d_out-1, and the sentinel everywhere else, guard
    rows included — compared on integer views, whole buffer."""
    got = _ibits(dst.cpu())
    n_rows = got.shape[0] if n_rows is None else n_rows
    want = torch.full_like(got, _sent_value(dst.dtype))
    row_of = np.asarray(row_of, dtype=np.int64)
    ok = (row_of >= 0) & (row_of < n_rows)
    want[torch.from_numpy(row_of[ok]), :d_out] = _ibits(want_rows)[torch.from_numpy(np.flatnonzero(ok))]
    if not torch.equal(got, want):
        bad = (got != want)
        r, c = [int(v[0]) for v in torch.nonzero(bad, as_tuple=True)]
        raise AssertionError(f"{what}: {int(bad.sum())} elements differ, first at row {r} column {c}: "
                             f"got {int(got[r, c]) & 0xFFFFFFFF:#x}, want {int(want[r, c]) & 0xFFFFFFFF:#x}")


# ---------------------------------------------------------------- fixtures
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
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    cache = {}

    def get(d_in, d_out, wt):
        if (d_in, d_out, wt) not in cache:
            cache[(d_in, d_out, wt)] = q2a.Projector(projector_path(d_in, d_out, wt), device=0)
        return cache[(d_in, d_out, wt)]

    yield get
    for p in cache.values():
        p.close()


@pytest.fixture(scope="module")
def engines(make_model):
    import q2a
    cache = {}

    def get(cfg, wt, act=0):
        if (cfg, wt, act) not in cache:
            cache[(cfg, wt, act)] = q2a.Engine(make_model(cfg, wt), device=0, act=act)
        return cache[(cfg, wt, act)]

    yield get
    for e in cache.values():
        e.close()


@pytest.fixture(scope="module")
def applied(projectors):
    """(x on the device, Projector.apply's f32 result on the CPU) per (d_in, weight type, M): random f32 rows of scale 1
    through the existing f32 path; computed once, left unchanged."""
    cache = {}

    def get(d_in, wt, M):
        if (d_in, wt, M) not in cache:
            pr = projectors(d_in, 4096, wt)
            g = torch.Generator(device="cuda").manual_seed(1000 * d_in + M)
            x = torch.randn((M, d_in), device="cuda", generator=g)
            y = torch.empty((M, pr.d_out), device="cuda")
            pr.apply(x.data_ptr(), M, y.data_ptr())
            torch.cuda.synchronize()
            cache[(d_in, wt, M)] = (x, y.cpu())
        return cache[(d_in, wt, M)]
    return get


# ---------------------------------------------------------------- 1. the epilogue in every regime
def cdiv(a, b):
    return -(-a // b)


def expected_regime(wt, M, N, K):
    """q2a_gemm.hip's narrow_tiles / wide_tiles / pipe8_ok restated for a projector's STORE_F GEMM."""
    import q2a
    if wt == "q6_k":
        return q2a.REGIME_FIXED
    wide = cdiv(M, 256) * (N // 256) >= 512 and N % 256 == 0
    narrow = cdiv(M, 128) * (N // 128) < 256
    nk = K // 64
    if wide:
        if wt == "f16":
            return q2a.REGIME_PIPE8 if nk % 2 == 0 else q2a.REGIME_256
        if wt == "q4_k":
            return q2a.REGIME_PIPE8 if nk % 4 == 0 else q2a.REGIME_128x256
        return q2a.REGIME_128x256
    return q2a.REGIME_NARROW if narrow else q2a.REGIME_128


# (weight type, d_in, M, regime name): every M has a partial last tile
REGIME_CASES = [
    ("f16", 256, 203, "NARROW"), ("f16", 256, 1003, "128"), ("f16", 256, 8003, "PIPE8"), ("f16", 320, 8003, "256"),
    ("q4_k", 256, 203, "NARROW"), ("q4_k", 256, 1003, "128"), ("q4_k", 256, 8003, "PIPE8"),
    ("q8_0", 256, 203, "NARROW"), ("q8_0", 256, 1003, "128"), ("q8_0", 256, 8003, "128x256"),
    ("q6_k", 256, 1003, "FIXED"),
]
F32_CASES = [("f16", 256, 1003, "128"), ("q4_k", 256, 1003, "128"), ("q8_0", 256, 1003, "128"), ("q6_k", 256, 1003, "FIXED")]
EPI_CASES = [c + (d,) for c in REGIME_CASES for d in ("bf16", "f16")] + [c + ("f32",) for c in F32_CASES]


@pytest.mark.parametrize("wt,d_in,M,regime,dt", EPI_CASES, ids=["-".join(map(str, c)) for c in EPI_CASES])
def test_epilogue_per_regime(projectors, applied, wt, d_in, M, regime, dt):
    import q2a
    pr = projectors(d_in, 4096, wt)
    want_regime = getattr(q2a, "REGIME_" + regime)
    assert expected_regime(wt, M, pr.d_out, d_in) == want_regime, "the case no longer lies in its regime"
    assert pr.regime(M) == want_regime
    assert M % 64 != 0 and M % 128 != 0 and M % 256 != 0
    x, y32 = applied(d_in, wt, M)
    dtype = DTYPES[dt]
    guard = 5   # rows behind n_rows: the destination holds exactly M rows
    dst = _sentinel(M + guard, pr.d_out, dtype)
    pr.apply_to(x.data_ptr(), M, q2a.feat_dst(dst.data_ptr(), pr.d_out, M, _dt(dt)))
    torch.cuda.synchronize()
    _check_dest(dst, y32.to(dtype), np.arange(M), pr.d_out, f"{wt} {regime} {dt}")


# ---------------------------------------------------------------- 2. the row map
MAP_M = 1003


def _map_case(kind, M):
    """(row_map or None, n_rows, ld) of a row-map case, on the q4_k 256 -> 4096 projector."""
    rng = np.random.default_rng(17)
    if kind == "identity":
        return None, M, 4096
    if kind == "permutation":
        n_rows = M + 37
        return rng.permutation(n_rows)[:M].astype(np.int32), n_rows, 4096
    if kind == "wide-ld":
        n_rows = M + 37
        return rng.permutation(n_rows)[:M].astype(np.int32), n_rows, 4096 + 128
    assert kind == "out-of-range"
    n_rows = M + 37
    rm = rng.permutation(n_rows)[:M].astype(np.int32)
    # rows that must be dropped, in the first tile, at a tile edge, in the middle and in the partial last tile
    for m, v in ((0, -1), (7, n_rows), (127, -1), (128, n_rows), (500, -2 ** 31), (501, 2 ** 31 - 1), (999, n_rows + 5),
                 (M - 1, -1)):
        rm[m] = v
    return rm, n_rows, 4096


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("kind", ["identity", "permutation", "wide-ld", "out-of-range"])
def test_row_map(projectors, applied, kind, dt):
    import q2a
    pr = projectors(256, 4096, "q4_k")
    x, y32 = applied(256, "q4_k", MAP_M)
    rm, n_rows, ld = _map_case(kind, MAP_M)
    dtype = DTYPES[dt]
    guard = 5
    dst = _sentinel(n_rows + guard, ld, dtype)
    rmd = torch.from_numpy(rm).cuda() if rm is not None else None
    pr.apply_to(x.data_ptr(), MAP_M, q2a.feat_dst(dst.data_ptr(), ld, n_rows, _dt(dt)), rmd.data_ptr() if rmd is not None else 0)
    torch.cuda.synchronize()
    row_of = rm if rm is not None else np.arange(MAP_M)
    if kind == "out-of-range":
        assert ((row_of < 0) | (row_of >= n_rows)).sum() == 8
    _check_dest(dst, y32.to(dtype), row_of, pr.d_out, f"row map {kind} {dt}", n_rows=n_rows)


def test_apply_to_arguments(projectors, applied):
    import q2a
    pr = projectors(256, 4096, "q4_k")
    x, _ = applied(256, "q4_k", MAP_M)
    dst = _sentinel(MAP_M + 1, 4096, torch.bfloat16)
    base = dst.data_ptr()
    for d in (q2a.feat_dst(base + 2, 4096, MAP_M, q2a.DT_BF16), q2a.feat_dst(0, 4096, MAP_M, q2a.DT_BF16),
              q2a.feat_dst(base, 4095, MAP_M, q2a.DT_BF16), q2a.feat_dst(base, 4096 + 4, MAP_M, q2a.DT_BF16),
              q2a.feat_dst(base, 4096, MAP_M, 3), q2a.feat_dst(base, 4096, MAP_M - 1, q2a.DT_BF16),
              q2a.feat_dst(base, 4096, -1, q2a.DT_BF16)):
        with pytest.raises(q2a.Q2AError) as ei:
            pr.apply_to(x.data_ptr(), MAP_M, d)
        assert ei.value.rc == ERR_ARG
    torch.cuda.synchronize()
    assert bool((_ibits(dst) == S16).all())


# ---------------------------------------------------------------- 3. the engine path
# the 13-clip batch of tests/test_gpu_audio_features.py, rebuilt here: the edges of the 16-row packing and of
# AvgPool1d(2), key length 1 (no output row) and, in the middle, a clip under 1 s that is skipped
KEY_LENS = [1, 2, 3, 15, 16, 17, 31, 33, 365, 1481, 1489, 1500]
OUT_LENS = [0, 1, 1, 7, 8, 8, 15, 16, 182, 740, 744, 750]
SKIP_AT = 6
GAP = 3
ENGINE_TYPES = ["f16", "q4_k", "q8_0"]


def _pcm_batch(clips):
    stride = max(len(c) for c in clips)
    pcm = torch.zeros(len(clips), stride)
    for i, c in enumerate(clips):
        pcm[i, :len(c)] = torch.from_numpy(np.ascontiguousarray(c))
    return pcm.cuda(), stride, [len(c) for c in clips]


@pytest.fixture(scope="module")
def batch13(make_clip):
    full = [make_clip(c, 480000) for c in range(3)]
    clips = [full[i % 3] for i in range(len(KEY_LENS))]
    clips.insert(SKIP_AT, make_clip(0, 160000)[:8000])
    lens = list(KEY_LENS)
    lens.insert(SKIP_AT, 100)
    want = list(OUT_LENS)
    want.insert(SKIP_AT, 0)
    return _pcm_batch(clips), lens, want


@pytest.fixture(scope="module")
def f32_features(engines, projectors, batch13):
    """q2a_audio_features_device (the f32 call) on batch13 per weight type -> (feat, embd on the CPU, out_len, status);
    computed once, left unchanged."""
    cache = {}

    def get(wt):
        if wt not in cache:
            (pcm, stride, ns), lens, want = batch13
            e, pr = engines("tiny", wt), projectors(256, 512, wt)
            n_tot = sum(want)
            feat = torch.full((n_tot, pr.d_out), float("nan"), device="cuda")
            embd = torch.full((n_tot, e.info.n_audio_state), float("nan"), device="cuda")
            ol, st = e.audio_features_device(pcm.data_ptr(), stride, ns, feat.data_ptr(), embd.data_ptr(), n_tot, projector=pr,
                                             key_len=lens)
            torch.cuda.synchronize()
            assert list(ol) == want and torch.isfinite(feat).all()
            cache[wt] = (feat.cpu(), embd.cpu(), list(ol), list(st))
        return cache[wt]
    return get


def _reverse_rows(out_len, first=2, tail=4):
    """clip_row in reverse clip order with GAP-row gaps: the last clip first -> (clip_row, n_rows)."""
    starts, at = [0] * len(out_len), first
    for c in reversed(range(len(out_len))):
        starts[c] = at
        at += out_len[c] + (GAP if out_len[c] else 0)
    return starts, at + tail


@pytest.mark.parametrize("wt", ENGINE_TYPES)
def test_engine_places_the_rows(engines, projectors, batch13, f32_features, wt):
    import q2a
    (pcm, stride, ns), lens, want = batch13
    e, pr = engines("tiny", wt), projectors(256, 512, wt)
    wfeat, wembd, wol, wst = f32_features(wt)
    n_tot = sum(want)
    clip_row, n_rows = _reverse_rows(want)
    clip_row[0], clip_row[SKIP_AT] = -5, 10 ** 9   # clips without rows: their entries are ignored
    ld = pr.d_out + 64
    dst = _sentinel(n_rows + 3, ld, torch.bfloat16)
    embd = torch.full((n_tot + 2, e.info.n_audio_state), S32, dtype=torch.int32, device="cuda").view(torch.float32)
    ol, st = e.audio_features_device_to(pcm.data_ptr(), stride, ns, q2a.feat_dst(dst.data_ptr(), ld, n_rows, q2a.DT_BF16), pr,
                                        clip_rows=clip_row, embd_ptr=embd.data_ptr(), embd_rows_cap=n_tot, key_len=lens)
    torch.cuda.synchronize()
    assert list(ol) == wol == want and list(st) == wst and st[SKIP_AT] == q2a.CLIP_SKIPPED
    n, row_of = q2a.feat_rows(want, clip_row, n_rows)
    assert n == n_tot
    # every placed row is the f32 call's row cast to bf16; the gaps, the rows before the first and behind the last range,
    # the columns past d_out and the rows behind n_rows keep the sentinel
    _check_dest(dst, wfeat.to(torch.bfloat16), row_of, pr.d_out, f"engine {wt}")
    got_embd = _ibits(embd.cpu())
    assert torch.equal(got_embd[:n_tot], _ibits(wembd)), "embd is no longer the packed f32 rows"
    assert bool((got_embd[n_tot:] == S32).all())


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
def test_engine_packed_without_clip_row(engines, projectors, batch13, f32_features, dt):
    """clip_row = NULL: the packed layout of the f32 call, in every element type; no embd."""
    import q2a
    (pcm, stride, ns), lens, want = batch13
    e, pr = engines("tiny", "q4_k"), projectors(256, 512, "q4_k")
    wfeat, _, wol, wst = f32_features("q4_k")
    n_tot = sum(want)
    dtype = DTYPES[dt]
    dst = _sentinel(n_tot + 4, pr.d_out, dtype)
    ol, st = e.audio_features_device_to(pcm.data_ptr(), stride, ns, q2a.feat_dst(dst.data_ptr(), pr.d_out, n_tot, _dt(dt)), pr,
                                        key_len=lens)
    torch.cuda.synchronize()
    assert list(ol) == wol and list(st) == wst
    _check_dest(dst, wfeat.to(dtype), np.arange(n_tot), pr.d_out, f"packed {dt}")


def test_engine_mel_entry_point(engines, projectors, make_clip):
    """One clip from frame 1000 through q2a_audio_features_device_mel_to against q2a_audio_features_device_mel."""
    import q2a
    e, pr = engines("tiny", "q4_k"), projectors(256, 512, "q4_k")
    mel = e.pcm_to_mel(make_clip(2, 276800))
    n_len = mel.shape[1]
    kl = [365]
    assert kl[0] <= q2a.mel_valid_lengths(n_len, 1000)[0]
    n_tot = kl[0] // 2
    md = torch.from_numpy(np.ascontiguousarray(mel)).cuda()
    wfeat = torch.full((n_tot, pr.d_out), float("nan"), device="cuda")
    wol, wst = e.audio_features_device_mel(md.data_ptr(), 0, n_len, [n_len], wfeat.data_ptr(), 0, n_tot, projector=pr,
                                           seek=[1000], key_len=kl)
    n_rows = n_tot + 20
    dst = _sentinel(n_rows, pr.d_out, torch.bfloat16)
    ol, st = e.audio_features_device_mel_to(md.data_ptr(), 0, n_len, [n_len], q2a.feat_dst(dst.data_ptr(), pr.d_out, n_rows, q2a.DT_BF16),
                                            pr, clip_rows=[11], seek=[1000], key_len=kl)
    torch.cuda.synchronize()
    assert list(ol) == list(wol) == [n_tot] and list(st) == list(wst) and n_tot > 0
    _check_dest(dst, wfeat.cpu().to(torch.bfloat16), 11 + np.arange(n_tot), pr.d_out, "mel entry point")


# ---------------------------------------------------------------- 4. Python: straight into inputs_embeds
def test_audio_features_into_inputs_embeds(engines, projectors, make_clip):
    import q2a
    e, pr = engines("tiny", "q4_k"), projectors(256, 512, "q4_k")
    L = 3000
    frames = [3000, 730, 33]
    x = np.stack([e.pcm_to_mel(make_clip(c, 480000))[:, :L] for c in range(3)])
    mask = np.zeros((3, L), dtype=np.int64)
    for c, n in enumerate(frames):
        mask[c, :n] = 1
    xd, md = torch.from_numpy(x).cuda(), torch.from_numpy(mask).cuda()
    wfeat, wol = e.audio_features(xd, md, projector=pr)            # the packed f32 features, as before
    torch.cuda.synchronize()
    assert list(wol) == [750, 182, 8] and wfeat.dtype == torch.float32
    # two sequences: clip 0 in the first, clips 1 and 2 in the second, the last run touching the sequence's end
    AUDIO, S = 151646, 1000
    ids = np.full((2, S), 11, dtype=np.int64)
    ids[0, 100:850] = AUDIO
    ids[1, 5:187] = AUDIO
    ids[1, S - 8:] = AUDIO
    starts, lens = q2a.audio_token_runs(ids, AUDIO)
    assert list(lens) == list(wol)
    inputs_embeds = _sentinel(2 * S, pr.d_out, torch.bfloat16).view(2, S, pr.d_out)
    out, ol = e.audio_features(xd, md, projector=pr, out=inputs_embeds, clip_rows=starts)
    torch.cuda.synchronize()
    assert out is inputs_embeds and list(ol) == list(wol)
    # the audio positions equal the cast features, in order; every text position is untouched
    _check_dest(inputs_embeds.view(2 * S, pr.d_out), wfeat.cpu().to(torch.bfloat16), np.flatnonzero(ids.reshape(-1) == AUDIO),
                pr.d_out, "inputs_embeds")
    # return_embd still hands back the packed f32 embd_enc; a float16 [rows][d_out] destination, packed
    _, _, wembd = e.audio_features(xd, md, projector=pr, return_embd=True)
    rows16 = _sentinel(sum(wol) + 3, pr.d_out, torch.float16)
    out2, ol2, embd = e.audio_features(xd, md, projector=pr, return_embd=True, out=rows16)
    torch.cuda.synchronize()
    assert out2 is rows16 and list(ol2) == list(wol) and torch.equal(_ibits(embd), _ibits(wembd))
    _check_dest(rows16, wfeat.cpu().to(torch.float16), np.arange(sum(wol)), pr.d_out, "float16 rows")
    with pytest.raises(ValueError):
        e.audio_features(xd, md, projector=pr, out=inputs_embeds[:, :, :256])     # not contiguous, wrong width
    with pytest.raises(ValueError):
        e.audio_features(xd, md, projector=pr, clip_rows=starts)                  # clip_rows without out
    with pytest.raises(ValueError):
        e.audio_features(xd, md, out=inputs_embeds, return_embd=True)             # out without a projector


# ---------------------------------------------------------------- 5. arguments: nothing is launched or written
def test_engine_arguments(engines, projectors, make_clip):
    import q2a
    e, pr = engines("tiny", "f16"), projectors(256, 512, "f16")
    clips = [make_clip(0, 160000), make_clip(1, 160000)]
    pcm, stride, ns = _pcm_batch(clips)
    per = q2a.valid_lengths(160000)[1]
    n_rows = 2 * per + 8
    dst = _sentinel(n_rows + 1, 512, torch.bfloat16)
    embd = torch.full((2 * per, 256), S32, dtype=torch.int32, device="cuda").view(torch.float32)
    base = dst.data_ptr()
    good = dict(base=base, ld=512, n_rows=n_rows, dtype=q2a.DT_BF16)

    def call(eng=e, p=pr, rows=(0, per + 4), cap=2 * per, **kw):
        d = dict(good, **kw)
        fd = q2a.feat_dst(d["base"], d["ld"], d["n_rows"], d["dtype"]) if d["base"] is not None else None
        return eng.audio_features_device_to(pcm.data_ptr(), stride, ns, fd, p, clip_rows=rows, embd_ptr=embd.data_ptr(),
                                            embd_rows_cap=cap)

    def untouched():
        torch.cuda.synchronize()
        return bool((_ibits(dst) == S16).all() and (_ibits(embd) == S32).all())

    cases = {
        "a misaligned base": dict(base=base + 2),
        "ld < d_out": dict(ld=504),
        "ld * 2 bytes not a multiple of 16": dict(ld=516),
        "a bad dtype": dict(dtype=3),
        "a range past n_rows": dict(rows=(0, n_rows - per + 1)),
        "a negative start": dict(rows=(-1, per + 4)),
        "overlapping ranges": dict(rows=(0, per - 1)),
        "packed rows past n_rows": dict(rows=None, n_rows=2 * per - 1),
        "dst without a projector": dict(p=None),
        "no dst": dict(base=None),
        "embd_rows_cap below N_tot": dict(cap=2 * per - 1),
    }
    for why, kw in cases.items():
        with pytest.raises(q2a.Q2AError) as ei:
            call(**kw)
        assert ei.value.rc == ERR_ARG, why
        assert untouched(), why
    # the bf16 activation contract has no packed kernel
    with pytest.raises(q2a.Q2AError) as ei:
        call(eng=engines("tiny", "f16", q2a.ACT_BF16))
    assert ei.value.rc == ERR_UNSUPPORTED and untouched()
    # and the call itself works with these buffers
    ol, st = call()
    torch.cuda.synchronize()
    assert list(ol) == [per, per]
    got = _ibits(dst.cpu())
    assert bool((got[:per] != S16).any()) and bool((got[per:per + 4] == S16).all()) and bool((got[2 * per + 4:] == S16).all())
    assert not bool((_ibits(embd) == S32).all())


# ---------------------------------------------------------------- 6. launch structure
PROF_CLASSES = ["mel", "conv1", "conv2", "ln", "gemm_qkv", "attn", "quant", "gemm_o", "gemm_fc1", "gemm_fc2", "pool"]   # Q2A_PROF_*


def test_launches_of_the_to_call(engines, projectors, batch13):
    """By the engine's per-class profile counters (one count per launch; the projector's GEMM is in no class): the _to
    call launches what the f32 call launches, plus the one map kernel (pool class) when clip_row is given."""
    import ctypes as C

    import q2a
    e, pr = engines("tiny", "q4_k"), projectors(256, 512, "q4_k")
    (pcm, stride, ns), lens, want = batch13
    n_tot = sum(want)
    lib, h = q2a.lib(), C.c_void_p(e.h)
    cnt = (C.c_int64 * len(PROF_CLASSES))()
    feat = torch.empty((n_tot, pr.d_out), device="cuda")
    clip_row, n_rows = _reverse_rows(want)
    dst = _sentinel(n_rows, pr.d_out, torch.bfloat16)
    fd = q2a.feat_dst(dst.data_ptr(), pr.d_out, n_rows, q2a.DT_BF16)

    def counts(call):
        call()
        torch.cuda.synchronize()
        assert lib.q2a_profile_read(h, None, cnt, len(PROF_CLASSES), 1) == 0
        return dict(zip(PROF_CLASSES, cnt))

    assert lib.q2a_profile_read(h, None, None, 0, 1) == 0
    assert lib.q2a_profile_enable(h, 1) == 0
    try:
        base = counts(lambda: e.audio_features_device(pcm.data_ptr(), stride, ns, feat.data_ptr(), 0, n_tot, projector=pr, key_len=lens))
        assert base["pool"] == 2 and base["mel"] == 1
        packed = counts(lambda: e.audio_features_device_to(pcm.data_ptr(), stride, ns, fd, pr, key_len=lens))
        assert packed == base
        placed = counts(lambda: e.audio_features_device_to(pcm.data_ptr(), stride, ns, fd, pr, clip_rows=clip_row, key_len=lens))
        assert placed == dict(base, pool=base["pool"] + 1)
        # no valid row at all: nothing is launched, the map kernel included
        none = counts(lambda: e.audio_features_device_to(pcm.data_ptr(), stride, ns[:2], fd, pr, clip_rows=[0, 0], key_len=[1, 1]))
        assert none == {c: 0 for c in PROF_CLASSES}
    finally:
        lib.q2a_profile_enable(h, 0)
        lib.q2a_profile_read(h, None, None, 0, 1)
