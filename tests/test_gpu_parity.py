"""Parity of the HIP path (lib/libq2a.so through its C ABI) against the CPU oracle and the reference's golden
vectors. All tests here need an MI355X."""
import numpy as np
import pytest

from conftest import full_ref_samples, rel_errors, tiny_ref_rows
import oracle_py
from q2a import ggmlfile

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


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


def _tensor_raw(mf, name):
    return np.ascontiguousarray(mf.t(name).data)


# ---------------------------------------------------------------- mel frontend
@pytest.mark.parametrize("clip", [0, 2, 3])
def test_mel_matches_oracle(engines, make_model, make_clip, golden, clip):
    meta, g = golden
    e = engines("tiny", "f16")
    pcm = make_clip(clip)
    mel = e.pcm_to_mel(pcm)
    orc = oracle_py.Oracle(ggmlfile.read(make_model("tiny", "f16"))).log_mel(pcm)
    assert mel.shape == orc.shape
    diff = np.abs(mel - orc)
    # same FFT recursion / op order as the reference; only double log10 ulps could differ
    assert diff.max() <= 1e-6, diff.max()
    assert (diff == 0).mean() > 0.999
    assert np.array_equal(mel.reshape(-1)[g[f"mel{clip}_idx"]] == g[f"mel{clip}_val"],
                          np.ones(len(g[f"mel{clip}_idx"]), bool)) or np.abs(
        mel.reshape(-1)[g[f"mel{clip}_idx"]] - g[f"mel{clip}_val"]).max() <= 1e-6


# ---------------------------------------------------------------- weight GEMMs (ggml activation conversion)
@pytest.mark.parametrize("wt", ["f16", "q4_k", "q8_0", "q4_0"])
@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_linear_matches_oracle(engines, make_model, wt, which):
    e = engines("tiny", wt)
    mf = ggmlfile.read(make_model("tiny", wt))
    D, F = 256, 1024
    K = F if which == 3 else D
    names = {0: ["self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight"],
             1: ["self_attn.out_proj.weight"], 2: ["fc1.weight"], 3: ["fc2.weight"]}[which]
    w = np.concatenate([_tensor_raw(mf, f"layers.1.{n}") for n in names])
    N = {0: 3 * D, 1: D, 2: F, 3: D}[which]
    M = 1500 + 37   # ragged row tail
    rng = np.random.default_rng(which)
    x = (rng.standard_normal((M, K)) * (1.0 if which != 3 else 0.3)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    yd = torch.empty((M, N), dtype=torch.float32, device="cuda")
    e.test_linear(1, which, xd.data_ptr(), M, yd.data_ptr())
    torch.cuda.synchronize()
    y = yd.cpu().numpy()
    ref = oracle_py.gemm(mf.wtype, w, x, N)
    mx, l2 = rel_errors(y, ref)
    # identical integer / fp16-exact products; only fp32 summation order differs
    assert mx < 1e-5 and l2 < 1e-6, (mx, l2)


# ---------------------------------------------------------------- attention vs a plain PyTorch fp32 reference
@pytest.mark.parametrize("cfg,D,H,B", [("tiny", 256, 4, 2), ("full", 1280, 20, 1)])
def test_attention_matches_fp32_reference(engines, cfg, D, H, B):
    e = engines(cfg, "f16")
    T = 1500
    g = torch.Generator(device="cpu").manual_seed(0)
    q = (torch.randn(B * T, D, generator=g) * 0.5).cuda()
    k = (torch.randn(B * T, D, generator=g) * 1.5).cuda()
    v = torch.randn(B * T, D, generator=g).cuda()
    out = torch.empty_like(q)
    e.test_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), B, out.data_ptr())
    torch.cuda.synchronize()
    qh = q.view(B, T, H, 64).permute(0, 2, 1, 3).double()
    kh = k.view(B, T, H, 64).permute(0, 2, 1, 3).double()
    vh = v.view(B, T, H, 64).permute(0, 2, 1, 3).double()
    p = torch.softmax(qh @ kh.transpose(-1, -2), dim=-1)
    ref = (p @ vh).permute(0, 2, 1, 3).reshape(B * T, D).float()
    mx, l2 = rel_errors(out.cpu().numpy(), ref.cpu().numpy())
    # F32-class contract: QK^T from hi/lo fp16 splits of Q and K (3 MFMA terms), P = Ph + Pl and
    # V = Vh + Vl into the P.V MFMA (3 terms), fp32 accumulation. Measured 1.3e-6 max-rel / 5.7e-7 rel-L2 (tiny); the bar
    # is ~10x that, so a P or V that falls back to one fp16 term (2^-11 per element: ~2e-4 rel-L2) fails it
    assert mx < 2e-5 and l2 < 5e-6, (mx, l2)


@pytest.mark.parametrize("cfg,D,H,B", [("tiny", 256, 4, 6), ("full", 1280, 20, 2)])
def test_attention_narrow_grid_gives_the_same_bits(engines, cfg, D, H, B):
    """One clip launches 16 queries per wave (its 128-query grid would leave CUs idle), a batch 32 (q2a_attn.hip
    launcher): every clip of the batch must equal that clip run alone, bit for bit (the lazy re-base is decided per
    16-query block, so a block's arithmetic does not depend on its wave-mates)."""
    e = engines(cfg, "f16")
    T = 1500
    g = torch.Generator(device="cpu").manual_seed(7)
    q = (torch.randn(B * T, D, generator=g) * 2.0).cuda()   # large scores: the re-base path runs
    k = (torch.randn(B * T, D, generator=g) * 2.0).cuda()
    v = torch.randn(B * T, D, generator=g).cuda()
    out = torch.empty_like(q)
    e.test_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), B, out.data_ptr())
    torch.cuda.synchronize()
    for b in (0, B - 1):
        sl = slice(b * T, (b + 1) * T)
        qs, ks, vs = q[sl].contiguous(), k[sl].contiguous(), v[sl].contiguous()
        o1 = torch.empty_like(qs)
        e.test_attention(qs.data_ptr(), ks.data_ptr(), vs.data_ptr(), 1, o1.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(o1, out[sl]), f"clip {b}: batched attention differs from the one-clip launch"


def test_attention_propagates_nan(engines):
    """q2a_attn.o is built with -fno-honor-nans (Makefile: the max reductions need no sNaN canonicalisation). A
    non-finite upstream value must still surface: a NaN in one query row makes that row's output NaN (its scores, hence
    its probabilities, are NaN whatever the max reduction returns), a NaN in one key row poisons its head for every query;
    rows and heads that never touch the poison stay finite and equal to the clean run (to rounding: a wave-wide lazy
    re-base may take another branch)."""
    e = engines("tiny", "f16")
    T, D, H, B = 1500, 256, 4, 1
    g = torch.Generator(device="cpu").manual_seed(3)
    q0 = (torch.randn(B * T, D, generator=g) * 0.5).cuda()
    k0 = (torch.randn(B * T, D, generator=g) * 1.5).cuda()
    v0 = torch.randn(B * T, D, generator=g).cuda()

    def run(q, k, v):
        out = torch.empty_like(q)
        torch.cuda.synchronize()   # q / k / v were written on torch's stream; the engine runs on its own
        e.test_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), B, out.data_ptr())
        torch.cuda.synchronize()
        return out.cpu()

    clean = run(q0, k0, v0)
    assert torch.isfinite(clean).all()
    q = q0.clone()
    q[700, 64:128] = float("nan")            # query 700, head 1
    o = run(q, k0, v0)
    assert torch.isnan(o[700, 64:128]).all()
    keep = torch.ones(T, dtype=torch.bool)
    keep[700] = False
    same = lambda a, b: bool(torch.isfinite(a).all()) and torch.allclose(a, b, rtol=1e-5, atol=1e-6)  # noqa: E731
    assert same(o[keep], clean[keep]) and same(o[700, :64], clean[700, :64])
    k = k0.clone()
    k[123, 128:192] = float("nan")           # key 123, head 2
    o = run(q0, k, v0)
    assert torch.isnan(o[:, 128:192]).all()
    assert same(o[:, :128], clean[:, :128]) and same(o[:, 192:], clean[:, 192:])


# ---------------------------------------------------------------- end to end, tiny model
def _encode(e, clips):
    out, st = e.encode_host(clips)
    return out, st


def _tiny_avg(out, g, xc, wt, clips):
    """The engine's statistics on the golden's sampled rows, averaged over the fixture's clips (batch order = clips)."""
    st = [rel_errors(out[i][g["rows_stride5"]], tiny_ref_rows(g, xc, wt, c)) for i, c in enumerate(clips)]
    return float(np.mean([x[0] for x in st])), float(np.mean([x[1] for x in st]))


def test_encoder_tiny_f16_vs_reference(engines, make_clip, golden, xclips, tiny_avg_bar):
    """Tiny F16 model against the reference (golden AVX2 build) over the fixture's clips: the clip-averaged statistics
    within the widest clip-averaged disagreement between two reference builds (tiny_avg_bar, x1.0) — the tiny model is
    not saturated by re-quantization chaos, so this is where an implementation's own rounding shows (the fp16 P.V of
    round 2 sat at 1.8x this bar); clip 0 on the whole output within the north-star 1e-3."""
    _, g = golden
    e = engines("tiny", "f16")
    bar = tiny_avg_bar("f16")
    out, st = _encode(e, [make_clip(c, 480000) for c in bar["clips"]])
    assert list(st) == [0] * len(bar["clips"])
    mx, l2 = _tiny_avg(out, g, xclips, "f16", bar["clips"])
    assert mx <= bar["max_rel"] and l2 <= bar["rel_l2"], (mx, l2, bar)
    mx0, l20 = rel_errors(out[0], g["tiny_f16_c0"])
    assert mx0 < 1e-3 and l20 < 1e-4, (mx0, l20)   # north-star 1e-3


@pytest.mark.parametrize("wt", ["q4_k", "q8_0", "q4_0"])
def test_encoder_tiny_quantized_vs_reference(engines, make_clip, golden, xclips, tiny_avg_bar, wt):
    """Tiny quantized models: activation re-quantization makes single int8 flips unavoidable, for the reference's
    own builds too; the bar is their widest clip-averaged disagreement on the golden's sampled rows (x1.0)."""
    _, g = golden
    e = engines("tiny", wt)
    bar = tiny_avg_bar(wt)
    out, st = _encode(e, [make_clip(c, 480000) for c in bar["clips"]])
    mx, l2 = _tiny_avg(out, g, xclips, wt, bar["clips"])
    assert mx <= bar["max_rel"] and l2 <= bar["rel_l2"], (mx, l2, bar)


def test_batch_equals_single_and_edge_clips(engines, make_clip, golden):
    """Ragged batch: two 30 s clips, a 7.3 s clip and a 41 s clip in one batch must equal the clips encoded
    alone, bit for bit (no cross-clip state), and match the reference outputs for each length."""
    _, g = golden
    e = engines("tiny", "f16")
    clips = [make_clip(c) for c in (0, 1, 2, 3)]
    outb, st = _encode(e, clips)
    assert list(st) == [0, 0, 0, 0]
    for i, c in enumerate((0, 1, 2, 3)):
        single, _ = _encode(e, [clips[i]])
        assert np.array_equal(single[0], outb[i]), f"clip {c} differs between batch and single"
        ref = g["tiny_f16_c0"][g["rows_stride5"]] if c == 0 else g[f"tiny_f16_c{c}_rows"]
        mx, l2 = rel_errors(outb[i][g["rows_stride5"]], ref)
        assert mx < 1e-3 and l2 < 1e-4, (c, mx, l2)


def test_short_audio_is_skipped_like_reference(engines, make_clip):
    """< 1 s after the offset: the reference returns 0 without encoding (qwen2-whisper.cpp:2359-2365)."""
    e = engines("tiny", "f16")
    sentinel = np.full((2,) + e.out_shape, 7.0, dtype=np.float32)
    out, st = e.encode_host([make_clip(5, 12000), make_clip(0)], out=sentinel.copy())
    assert st[0] == 1 and st[1] == 0
    assert np.all(out[0] == 7.0)
    assert not np.all(out[1] == 7.0)


def test_host_call_failure_reports_failed_clips(engines, make_clip):
    """q2a_encode_host_ex on 40 clips (two chunks of 20) whose clip 30 carries a negative window offset: the second
    chunk fails, so no clip's output reaches the caller and every status is Q2A_CLIP_FAILED (2) — none reads as a
    stale ENCODED — and the caller's buffer is untouched. A negative sample count fails before any copy, the same way.
    The engine stays usable afterwards."""
    import q2a
    e = engines("tiny", "f16")
    clip = make_clip(0)
    clips = [clip] * 40
    offs = [0] * 40
    offs[30] = -100
    sentinel = np.full((40,) + e.out_shape, 7.0, dtype=np.float32)
    out, st, rc = e.encode_host(clips, out=sentinel.copy(), offsets_ms=offs, raise_on_error=False)
    assert rc == -4, rc
    assert list(st) == [q2a.CLIP_FAILED] * 40
    assert np.all(out == 7.0)
    bad = [clip] * 3
    ns_bad = np.array([len(clip), -5, len(clip)], dtype=np.int32)
    st2 = np.full(3, -1, dtype=np.int32)
    ptrs = (q2a.C.c_void_p * 3)(*[c.ctypes.data for c in bad])
    i32p = q2a.C.POINTER(q2a.C.c_int32)
    rc2 = q2a.lib().q2a_encode_host(e.h, ptrs, ns_bad.ctypes.data_as(i32p), 3, 0, q2a.C.c_void_p(out.ctypes.data),
                                    st2.ctypes.data_as(i32p))
    assert rc2 == -4 and list(st2) == [q2a.CLIP_FAILED] * 3
    out2, st3 = e.encode_host([clip, clip], offsets_ms=[0, 0])
    assert list(st3) == [q2a.CLIP_ENCODED] * 2 and np.array_equal(out2[0], out2[1])


def test_invalid_arguments_rejected(engines, make_clip):
    """Argument errors come back as Q2A_ERR_ARG (-4, include/q2a_encoder.h) before any launch — an empty batch, a
    negative sample count, a clip longer than its PCM row, a negative offset, a zero reservation — and leave the
    engine usable: the next valid call is bit-identical to one made before the errors."""
    import q2a
    e = engines("tiny", "f16")
    clip = make_clip(0)
    ref, st = e.encode_host([clip])
    assert list(st) == [0]
    pcm = torch.from_numpy(clip).cuda()
    out = torch.empty((1,) + e.out_shape, dtype=torch.float32, device="cuda")
    bad = [
        lambda: e.encode_host([]),
        lambda: e.encode_device(pcm.data_ptr(), pcm.numel(), [-1], out.data_ptr()),
        lambda: e.encode_device(pcm.data_ptr(), pcm.numel(), [pcm.numel() + 1], out.data_ptr()),
        lambda: e.encode_device(pcm.data_ptr(), pcm.numel(), [pcm.numel()], out.data_ptr(), offset_ms=-10),
        lambda: e.encode_device(pcm.data_ptr(), pcm.numel(), [pcm.numel()], 0),
        lambda: e.reserve(0),
    ]
    for call in bad:
        with pytest.raises(q2a.Q2AError, match=r"q2a error -4"):
            call()
    torch.cuda.synchronize()
    again, st = e.encode_host([clip])
    assert list(st) == [0]
    assert np.array_equal(again, ref)
    st = e.encode_device(pcm.data_ptr(), pcm.numel(), [pcm.numel()], out.data_ptr())
    torch.cuda.synchronize()
    assert list(st) == [0]
    assert np.array_equal(out.cpu().numpy(), ref)


@pytest.mark.parametrize("compact", [False, True])
def test_device_blob_path_matches_file_path(engines, make_model, make_clip, compact):
    """The multi-GPU path (pack on host -> device copy (RCCL broadcast) -> open on the device blob) must give
    bit-identical outputs to opening the file — also from the compact transport blob, which the open expands on the
    GPU."""
    import q2a
    path = make_model("tiny", "q4_k")
    blob = q2a.pack_model(path, compact=compact)
    dev = torch.frombuffer(blob, dtype=torch.uint8).cuda()
    e2 = q2a.Engine(device=0, device_blob=dev.data_ptr(), blob_size=len(blob))
    del dev   # a compact blob was expanded into an engine-owned copy; a device-layout blob must stay alive
    clip = make_clip(0)
    a, _ = engines("tiny", "q4_k").encode_host([clip])
    if not compact:
        dev = torch.frombuffer(blob, dtype=torch.uint8).cuda()
        e2.close()
        e2 = q2a.Engine(device=0, device_blob=dev.data_ptr(), blob_size=len(blob))
    b, _ = e2.encode_host([clip])
    e2.close()
    assert np.array_equal(a, b)


@pytest.mark.parametrize("cfg,wt,act", [("tiny", "q4_k", 0), ("tiny", "q8_0", 0), ("tiny", "q4_0", 0), ("tiny", "f16", 0),
                                        ("tiny", "f32", 0), ("tiny", "q4_k", 1), ("tiny", "q8_0", 1),
                                        ("full", "q4_k", 0), ("full", "q8_0", 1)])
def test_compact_blob_expands_to_the_host_pack_bytes(make_model, cfg, wt, act):
    """q2a_expand_blob (the GPU expansion behind opening a compact blob: Q4_K sc*q operands, block-major d / dmin /
    beta / gamma / min operands, Q8_0 / Q4_0 codes, F32 hi|lo splits, bf16 dequantization) reproduces the host
    packer's device layout byte for byte, for every weight type and both activation contracts. Full size Q4_K: the
    transport blob is <= 0.4 GB against the 1.40 GB it expands to."""
    import q2a
    path = make_model(cfg, wt)
    full = q2a.pack_model(path, act)
    comp = q2a.pack_model(path, act, compact=True)
    dev_bytes, tr_bytes = q2a.blob_device_size(comp)
    assert dev_bytes == len(full) and tr_bytes == len(comp)
    if (cfg, wt, act) == ("full", "q4_k", 0):
        assert len(comp) <= 0.4e9 and len(full) > 1.3e9
    cd = torch.frombuffer(comp, dtype=torch.uint8).cuda()
    out = torch.full((len(full),), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    q2a.expand_blob(cd.data_ptr(), len(comp), out.data_ptr(), len(full), 0)
    torch.cuda.synchronize()
    want = torch.frombuffer(full, dtype=torch.uint8).cuda()
    eq = out == want
    assert bool(eq.all()), f"{int((~eq).sum())} bytes differ, first at {int((~eq).nonzero()[0])}"


def test_encoder_tiny_matches_oracle_intermediate_free(engines, make_model, make_clip):
    """Oracle (CPU restatement) on a second clip, full output compared."""
    e = engines("tiny", "f16")
    mf = ggmlfile.read(make_model("tiny", "f16"))
    o = oracle_py.Oracle(mf)
    pcm = make_clip(1)
    ref = o.encode(o.mel_window(o.log_mel(pcm)))
    out, _ = _encode(e, [pcm])
    mx, l2 = rel_errors(out[0], ref)
    assert mx < 1e-3 and l2 < 1e-4, (mx, l2)


# ---------------------------------------------------------------- full size (L=32, D=1280, H=20)
def _full_size_check(outs, g, xc, wt, bar):
    """Full-size outputs of the fixture's clips (bar["clips"], in that order) against the reference's golden samples:
    the clip-averaged statistics within the widest clip-averaged disagreement between two reference builds
    (xbuild_avg_bar, x1.0); F16 also within the north-star 1e-3 on every clip. Clip 0's row norms within
    20x the cross-build row-norm spread (a secondary statistic; the element-wise bars are the contract)."""
    idx = g[f"full_{wt}_c0_idx"]
    st = [rel_errors(o.reshape(-1)[idx], full_ref_samples(g, xc, wt, c)) for o, c in zip(outs, bar["clips"])]
    mxs, l2s = float(np.mean([x[0] for x in st])), float(np.mean([x[1] for x in st]))
    assert mxs <= bar["max_rel"] and l2s <= bar["rel_l2"], (wt, mxs, l2s, st, bar)
    if wt == "f16":
        assert all(x[0] < 1e-3 and x[1] < 1e-3 for x in st), st
    rn = np.linalg.norm(outs[0].astype(np.float64), axis=1)
    rnerr = np.abs(rn - g[f"full_{wt}_c0_rownorm"]).max() / g[f"full_{wt}_c0_rownorm"].max()
    assert rnerr < 20 * bar["rownorm_rel"], (wt, rnerr, bar)


@pytest.mark.parametrize("wt", ["f16", "q4_k", "q8_0"])
def test_encoder_full_size_vs_reference_samples(engines, make_clip, golden, xclips, xbuild_avg_bar, xbuild_bar, wt):
    _, g = golden
    e = engines("full", wt)
    bar = dict(xbuild_avg_bar(wt), rownorm_rel=xbuild_bar(wt)["rownorm_rel"])
    out, st = _encode(e, [make_clip(c, 480000) for c in bar["clips"]])
    assert list(st) == [0] * len(bar["clips"])
    _full_size_check(list(out), g, xclips, wt, bar)


# ---------------------------------------------------------------- big-tile GEMM configuration (256-wide tiles)
@pytest.mark.parametrize("wt", ["f16", "q4_k", "q8_0"])
@pytest.mark.parametrize("which", [0, 2])
def test_linear_big_tiles_match_oracle(engines, make_model, wt, which):
    """M large enough that the launcher picks the 256-wide tile / 8-wave kernels (the batched-serving shapes)."""
    e = engines("tiny", wt)
    mf = ggmlfile.read(make_model("tiny", wt))
    D, F = 256, 1024
    names = {0: ["self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight"],
             2: ["fc1.weight"]}[which]
    w = np.concatenate([_tensor_raw(mf, f"layers.0.{n}") for n in names])
    N = {0: 3 * D, 2: F}[which]
    M = 45000 + 17
    x = np.random.default_rng(100 + which).standard_normal((M, D)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    yd = torch.empty((M, N), dtype=torch.float32, device="cuda")
    e.test_linear(0, which, xd.data_ptr(), M, yd.data_ptr())
    torch.cuda.synchronize()
    ref = oracle_py.gemm(mf.wtype, w, x, N)
    mx, l2 = rel_errors(yd.cpu().numpy(), ref)
    assert mx < 1e-5 and l2 < 1e-6, (mx, l2)


@pytest.mark.parametrize("wt", ["f16", "q4_k"])
@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_linear_full_size_bench_shape_matches_oracle(engines, make_model, wt, which):
    """The bench's GEMM shapes exactly: full-size weights (K = 1 280 or 5 120: five / twenty Q4_K blocks, so the
    block recurrence runs between blocks, which the tiny model's single block never does), M = 96 000 rows in ONE
    launch: the single 8-phase 256x256 grid. (Q2A_EPI_STORE_F never takes the two-launch partial-round tail — that is
    for RESID, PRE_H and GELU_H, run by tests/test_gpu_gemm_epilogues.py::test_partial_round_tail.) Checked against the
    C oracle on 384 sampled rows, including the rows around 91 648, where fc2's RESID launch of this M has its seam on 256 CUs."""
    e = engines("full", wt)
    mf = ggmlfile.read(make_model("full", wt))
    D, F = 1280, 5120
    K = F if which == 3 else D
    names = {0: ["self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight"],
             1: ["self_attn.out_proj.weight"], 2: ["fc1.weight"], 3: ["fc2.weight"]}[which]
    w = np.concatenate([_tensor_raw(mf, f"layers.7.{n}") for n in names])
    N = {0: 3 * D, 1: D, 2: F, 3: D}[which]
    M = 96000
    g = torch.Generator(device="cuda").manual_seed(200 + which)
    xd = torch.randn((M, K), device="cuda", generator=g) * (1.0 if which != 3 else 0.3)
    yd = torch.empty((M, N), dtype=torch.float32, device="cuda")
    # no synchronisation: with stream NULL the engine's work is ordered after torch's default stream (x) and before
    # what torch queues there next (the row gather below) — include/q2a_encoder.h
    e.test_linear(7, which, xd.data_ptr(), M, yd.data_ptr())
    rows = np.unique(np.concatenate([np.random.default_rng(which).choice(M, 352, replace=False),
                                     [0, 255, 256, 91647, 91648, 95999 - 1, 95999] + list(range(91640, 91664))]))
    ri = torch.from_numpy(rows).cuda()
    x = xd[ri].cpu().numpy()
    y = yd[ri].cpu().numpy()
    del xd, yd
    ref = oracle_py.gemm(mf.wtype, w, x, N)
    mx, l2 = rel_errors(y, ref)
    assert mx < 1e-5 and l2 < 1e-6, (mx, l2)


@pytest.mark.parametrize("wt", ["f16", "q4_k"])
def test_encoder_bench_batch_64_is_batch_invariant(engines, make_clip, golden, xclips, xbuild_avg_bar, xbuild_bar, wt):
    """The bench's own batch (64 full-size clips, the 8-phase 256x256 kernels): clip 0 at positions 0 and 63 with 62
    different clips between them. Both copies must be bit-identical, equal to clip 0 encoded ALONE (small-tile
    kernels) bit for bit — a clip's embedding does not depend on what it is batched with — and match the reference."""
    _, g = golden
    e = engines("full", wt)
    c0 = make_clip(0)
    clips = [c0] + [make_clip(100 + i, 480000) for i in range(62)] + [c0]
    # ONE device call over all 64 clips, as bench.py times it (q2a_encode_host chunks its batch into 32-clip pieces):
    # every GEMM is one launch with M = 96 000 rows, so the 8-phase grids and fc2's partial-round tail on 128x128 tiles
    # (launch_pipe8, only at this M) are what runs; the single-clip encode below runs the small tiles and no tail
    pcm = torch.from_numpy(np.stack(clips).astype(np.float32)).cuda()
    outd = torch.empty((64,) + e.out_shape, dtype=torch.float32, device="cuda")
    st = e.encode_device(pcm.data_ptr(), pcm.shape[1], [pcm.shape[1]] * 64, outd.data_ptr())
    torch.cuda.synchronize()
    out = outd.cpu().numpy()
    del pcm, outd
    assert list(st) == [0] * 64
    assert np.array_equal(out[0], out[63])
    single, _ = e.encode_host([c0])
    assert np.array_equal(single[0], out[0]), "batch-of-64 output differs from the single-clip encode"
    bar = dict(xbuild_avg_bar(wt), rownorm_rel=xbuild_bar(wt)["rownorm_rel"])
    pos = {0: 0, **{100 + i: 1 + i for i in range(62)}}   # batch position of each clip id
    _full_size_check([out[pos[c]] for c in bar["clips"]], g, xclips, wt, bar)


# ---------------------------------------------------------------- one encoder block at batched (wide-tile) shapes
# bars: 3x the rel-L2 measured in round 3 (profiles/r03zt_parity_log.jsonl: f16 6.5e-6, q4_k 6.5e-5, q8_0 4.2e-5). The
# quantized residual is Q8_K / Q8_0 code flips where the engine's and the oracle's fp32 sums round differently; F16
# has no re-quantization, so its bar is an order of magnitude tighter
@pytest.mark.parametrize("wt,tol_l2", [("f16", 2e-5), ("q4_k", 2e-4), ("q8_0", 1.3e-4)])
def test_block_batched_matches_oracle_layer0(engines, make_model, make_clip, wt, tol_l2):
    """Layer 0 on 30 copies of the oracle's layer-0 input (M = 45 000 rows: wide tiles, and for Q4_K the fused
    fc1 + GELU + Q8_K epilogue) against the oracle's own layer-0 output; the two ends of the batch bit-identical."""
    e = engines("tiny", wt)
    mf = ggmlfile.read(make_model("tiny", wt))
    o = oracle_py.Oracle(mf)
    _, dumps = o.encode(o.mel_window(o.log_mel(make_clip(0))), dump=True)
    x0 = dumps["conv_out"]
    B = 30
    x = torch.from_numpy(np.tile(x0, (B, 1))).cuda()
    e.test_block(0, x.data_ptr(), B)
    torch.cuda.synchronize()
    out = x.cpu().numpy().reshape(B, 1500, -1)
    assert np.array_equal(out[0], out[B - 1])
    mx, l2 = rel_errors(out[0], dumps["x2"])
    assert l2 < tol_l2, (mx, l2)


# ---------------------------------------------------------------- deferred GELU (Q4_K fc1 -> Q8_K quantizer)
@pytest.mark.parametrize("n_clips", [1, 30])
def test_deferred_gelu_equals_epilogue_gelu(make_model, make_clip, n_clips):
    """Q4_K fc1 writes its fp16 pre-activation (Q2A_EPI_PRE_H) and the Q8_K quantizer applies the GELU table; the
    codes, hence every output bit, must equal the GELU-epilogue + quantizer path (q2a_test_fc1_path 1) and, at the
    8-phase batch shapes, the fused GELU + Q8_K fc1 epilogue (path 2)."""
    import q2a
    path = make_model("tiny", "q4_k")
    clips = [make_clip(0)] * n_clips
    engines = [q2a.Engine(path, device=0) for _ in range(3)]
    try:
        outs = []
        for k, e in enumerate(engines):
            e.test_fc1_path(k)
            outs.append(e.encode_host(clips)[0])
        assert np.array_equal(outs[0], outs[1])
        assert np.array_equal(outs[0], outs[2])
    finally:
        for e in engines:
            e.close()


def test_null_stream_is_ordered_with_the_default_stream(engines):
    """include/q2a_encoder.h: a NULL stream runs on the engine's own stream ORDERED as if issued on stream 0. The input
    comes out of a chain of torch kernels still queued on the default stream when the call is made, and the output is
    consumed by a torch kernel queued right after it — no synchronisation anywhere; the result must equal the same
    call made on fully drained inputs (ADVICE/VERDICT r04: the round-4 race at the bench shape)."""
    e = engines("full", "f16")
    M, K, N = 96000, 1280, 5120
    g = torch.Generator(device="cuda").manual_seed(77)
    base = torch.randn((M, K), device="cuda", generator=g)
    torch.cuda.synchronize()
    ref = torch.empty((M, N), dtype=torch.float32, device="cuda")
    e.test_linear(3, 2, base.data_ptr(), M, ref.data_ptr())
    torch.cuda.synchronize()
    ref_sum = ref.double().sum().item()
    for _ in range(3):
        x = base * 0.5
        for _ in range(20):   # ~20 more launches queued on stream 0 ahead of the engine's reads
            x = x * 1.0 + 0.0
        x = x * 2.0
        y = torch.full((M, N), float("nan"), dtype=torch.float32, device="cuda")
        e.test_linear(3, 2, x.data_ptr(), M, y.data_ptr())
        got = torch.equal(y, ref)      # queued on stream 0 behind the engine's work
        assert got and y.double().sum().item() == ref_sum
