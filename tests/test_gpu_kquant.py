"""Q5_K and Q6_K model files on the GPU (lib/libq2a.so through its C ABI). Q5_K runs the Q4_K kernels on a Q4_K-layout
blob (5-bit codes, sc*q <= 1953); Q6_K runs its own GEMM block mode (Q2A_BLK_Q6K, csrc/q2a_internal.h). The references:
the integer contract of ggml's vec_dot in float64 (tests/kquant_cases.py), the reference's own outputs and cross-build
disagreement (tests/golden/golden_kq.*, make_golden_kq.py). All tests need an MI355X."""
import os
import subprocess
import time

import numpy as np
import pytest

import kquant_cases as kc
from conftest import GOLDEN_DIR, TOOL, _avg_bar, rel_errors
from q2a import ggmlfile

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

D, F = kc.D, kc.F
TYPES = ["q5_k", "q6_k"]


@pytest.fixture(scope="module")
def golden_kq():
    return kc.load_golden_kq(GOLDEN_DIR)


@pytest.fixture(scope="module")
def kq_model(make_model, workdir, golden_kq):
    """kq_model(cfg, wt): the tiny / full model (conftest make_model), or cfg "tinyext": the hand-made rows of
    tests/kquant_cases.py quantized by bin/q2a_tool; SHA-256 checked against the reference-quantized files."""
    meta, _ = golden_kq

    def make(cfg, wt):
        if cfg != "tinyext":
            path = make_model(cfg, wt)
        else:
            ext = os.path.join(workdir, "tinyext-f16.bin")
            if not os.path.exists(ext):
                kc.write_ext_model(make_model("tiny", "f16"), ext)
            path = os.path.join(workdir, f"tinyext-{wt}.bin")
            if not os.path.exists(path):
                subprocess.check_call([TOOL, "quantize", ext, path, wt, "8"])
        from conftest import _sha
        assert _sha(path) == meta["models"][f"{cfg}-{wt}"]["sha256"], f"quantizer drift for {cfg}-{wt}"
        return path

    return make


@pytest.fixture(scope="module")
def engines(kq_model):
    import q2a
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    cache = {}

    def get(cfg, wt, act=0):
        if (cfg, wt, act) not in cache:
            cache[(cfg, wt, act)] = q2a.Engine(kq_model(cfg, wt), device=0, act=act)
        return cache[(cfg, wt, act)]

    yield get
    for e in cache.values():
        e.close()


def _linear(e, layer, which, xd, M, N):
    yd = torch.empty((M, N), dtype=torch.float32, device="cuda")
    e.test_linear(layer, which, xd.data_ptr(), M, yd.data_ptr())
    torch.cuda.synchronize()
    return yd


def _nk(which):
    return {0: 3 * D, 1: D, 2: F, 3: D}[which], (F if which == 3 else D)


# ---------------------------------------------------------------- 1. one linear against the integer contract
@pytest.mark.parametrize("wt", TYPES)
@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_linear_matches_the_integer_contract(engines, kq_model, wt, which):
    """M = 1537 (ragged tail; Q5_K on the narrow 64x128 tiles, Q6_K on its 128x128 tile). fc2 (K = 1024) is where blocks
    1..3 run: Q5_K's block-ratio recurrence, Q6_K's per-block acc += (dx*dy)*blkI. Bar: the one-linear bar of every
    weight type, 1e-5 max-rel / 1e-6 rel-L2 (identical integer products; only the fp32 summation order differs)."""
    e = engines("tiny", wt)
    mf = ggmlfile.read(kq_model("tiny", wt))
    N, K = _nk(which)
    M = 1537
    x = (np.random.default_rng(which).standard_normal((M, K)) * (1.0 if which != 3 else 0.3)).astype(np.float32)
    y = _linear(e, 1, which, torch.from_numpy(x).cuda(), M, N).cpu().numpy()
    ref = kc.kq_linear_ref(kc.matrix_tensors(mf, 1, which), x)
    mx, l2 = rel_errors(y, ref)
    print(f"linear {wt} which={which}: max-rel {mx:.3e} rel-L2 {l2:.3e}")
    assert mx < 1e-5 and l2 < 1e-6, (mx, l2)


# ---------------------------------------------------------------- 2. the same at wide tiles (Q5_K; Q6_K has one regime)
@pytest.mark.parametrize("which,M", [(2, 45017), (3, 131089)])
def test_q5k_linear_wide_tiles(engines, kq_model, which, M):
    """fc1 at M = 45 017 (the 8-phase 256x256 kernel, one Q4_K-layout block) and fc2 at M = 131 089: N = 256, so
    ceil(M / 256) * (N / 256) = 513 >= 512 is the smallest M that puts a 4-block K on the 8-phase kernel and its partial
    last round. The float64 contract is evaluated on sampled rows (tile edges, the ragged tail, 600 random rows)."""
    e = engines("tiny", "q5_k")
    mf = ggmlfile.read(kq_model("tiny", "q5_k"))
    N, K = _nk(which)
    g = torch.Generator(device="cuda").manual_seed(300 + which)
    xd = torch.randn((M, K), device="cuda", generator=g) * (1.0 if which != 3 else 0.3)
    yd = _linear(e, 0, which, xd, M, N)
    last_tile = (M - 1) // 256 * 256
    rows = np.unique(np.concatenate([np.random.default_rng(which).choice(M, 600, replace=False),
                                     [0, 255, 256, 511, last_tile - 1], np.arange(last_tile, M)]))
    ri = torch.from_numpy(rows).cuda()
    x, y = xd[ri].cpu().numpy(), yd[ri].cpu().numpy()
    ref = kc.kq_linear_ref(kc.matrix_tensors(mf, 0, which), x)
    mx, l2 = rel_errors(y, ref)
    print(f"wide q5_k which={which} M={M}: max-rel {mx:.3e} rel-L2 {l2:.3e}")
    assert mx < 1e-5 and l2 < 1e-6, (mx, l2)


# ---------------------------------------------------------------- 3. the end codes, block sums past 2^24
@pytest.mark.parametrize("wt", TYPES)
@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_linear_extremes(engines, kq_model, wt, which):
    """Test 1 on the hand-made rows (kquant_cases: zeroed blocks, a lone outlier, constant rows at the end codes — the CPU
    test asserts Q5_K q = 31 with sc = 63 and Q6_K sc = -128 with q = 0 and q = 63 occur there) against activations of
    one sign at full scale: row 0 all 1.0 (every Q8_K code -127), the rest uniform in [0.9, 1]. The constant weight rows
    then reach |I_b| = 256 * 128 * 32 * 127 = 133 169 152 (2^26.99) for Q6_K — its f32 block sum blkI is past 2^24, where
    it is no longer ggml's exact integer sumi — and 256 * 63 * 31 * 127 = 63 495 936 (2^25.9) for Q5_K. Same bar, against
    the float64 value."""
    e = engines("tinyext", wt)
    mf = ggmlfile.read(kq_model("tinyext", wt))
    N, K = _nk(which)
    M = 1537
    x = np.random.default_rng(50 + which).uniform(0.9, 1.0, (M, K)).astype(np.float32)
    x[0] = 1.0
    y = _linear(e, 0, which, torch.from_numpy(x).cuda(), M, N).cpu().numpy()
    ref, imax, mag = kc.kq_linear_ref(kc.matrix_tensors(mf, 0, which), x, return_int=True)
    assert imax == 256 * 127 * (128 * 32 if wt == "q6_k" else 63 * 31), imax   # the type's largest possible |I_b|
    assert imax > 2 ** 24
    mx, l2 = rel_errors(y, ref)
    print(f"extremes {wt} which={which}: |I_b| max {imax:.0f} max-rel {mx:.3e} rel-L2 {l2:.3e}")
    assert mx < 1e-5 and l2 < 1e-6, (mx, l2)
    # the hand-made rows one by one (the large constant rows hide the others in the whole-matrix statistic): each
    # within 1e-5 of the magnitude of the terms it sums. With one-sign activations the alternating row and Q5_K's
    # d*sc*q - dmin*m split cancel almost completely, and an fp32 sum's error scales with the terms, not with the result
    # (ggml's own f32 accumulation is no different); a zeroed row has no terms and must come out as exactly 0
    for r in range(kc.EXT_ROWS):
        d = np.abs(y[:, r] - ref[:, r]).max()
        assert d <= 1e-5 * mag[:, r].max(), (r, d, mag[:, r].max())


# ---------------------------------------------------------------- 4. device expand of the compact blob
@pytest.mark.parametrize("cfg,wt,act", [("tiny", "q5_k", 0), ("tiny", "q6_k", 0), ("tinyext", "q5_k", 0),
                                        ("tinyext", "q6_k", 0), ("tiny", "q5_k", 1), ("tiny", "q6_k", 1)])
def test_compact_blob_expands_to_the_host_pack_bytes(kq_model, cfg, wt, act):
    """q2a_expand_blob reproduces the host packer's device layout byte for byte: Q5_K's sc*q operands with the fifth bit
    from qh and the Q4_K block arrays, Q6_K's q - 32 operands, d and the sub-block-major scales; the hand-made rows add
    the d = 0 blocks; act 1 the bf16 dequantization."""
    import q2a
    path = kq_model(cfg, wt)
    full = q2a.pack_model(path, act)
    comp = q2a.pack_model(path, act, compact=True)
    assert q2a.blob_device_size(comp) == (len(full), len(comp))
    cd = torch.frombuffer(comp, dtype=torch.uint8).cuda()
    out = torch.full((len(full),), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    q2a.expand_blob(cd.data_ptr(), len(comp), out.data_ptr(), len(full), 0)
    torch.cuda.synchronize()
    eq = out == torch.frombuffer(full, dtype=torch.uint8).cuda()
    assert bool(eq.all()), f"{int((~eq).sum())} bytes differ, first at {int((~eq).nonzero()[0])}"


# ---------------------------------------------------------------- 5. tiny encoder against the reference
def _kq_bar(meta, prefix, clips, keys):
    entries = [meta[prefix]] + [meta[f"{prefix}_clip{c}"] for c in clips[1:]]
    return _avg_bar(entries, keys)


@pytest.mark.parametrize("wt", TYPES)
def test_encoder_tiny_vs_reference(engines, make_clip, golden, golden_kq, wt):
    """Clips 0 and 101..104, the statistics on rows_stride5 averaged over the clips, within the fixture's widest
    clip-averaged pair of reference builds x1.0 (tiny_avg_bar's rule, from golden_kq.json)."""
    meta, kq = golden_kq
    rows = golden[1]["rows_stride5"]
    clips = [0, 101, 102, 103, 104]
    bar = _kq_bar(meta, f"tiny_{wt}", clips, {"max_rel": "rows_max_rel", "rel_l2": "rows_rel_l2"})
    e = engines("tiny", wt)
    assert e.info.wtype == kc.WT_TYPE[wt] and e.info.act == 0   # q2a_get_info reports the file's type
    out, st = e.encode_host([make_clip(c, 480000) for c in clips])
    assert list(st) == [0] * len(clips)
    s = [rel_errors(out[i][rows], kq[f"tiny_{wt}_c{c}_rows"]) for i, c in enumerate(clips)]
    mx, l2 = float(np.mean([x[0] for x in s])), float(np.mean([x[1] for x in s]))
    print(f"tiny {wt}: max-rel {mx:.3e} (bar {bar['max_rel']:.3e}) rel-L2 {l2:.3e} (bar {bar['rel_l2']:.3e})")
    assert mx <= bar["max_rel"] and l2 <= bar["rel_l2"], (mx, l2, bar)


# ---------------------------------------------------------------- 6. batch and entry-point invariance (Q6_K bytes)
def test_q6k_clip_does_not_depend_on_its_batch(engines, make_clip):
    e = engines("tiny", "q6_k")
    c0 = make_clip(0)
    alone, _ = e.encode_host([c0])
    batch, st = e.encode_host([c0, make_clip(101, 480000), c0])
    assert list(st) == [0, 0, 0]
    assert np.array_equal(alone[0].view(np.uint32), batch[0].view(np.uint32))
    assert np.array_equal(alone[0].view(np.uint32), batch[2].view(np.uint32))


def test_q6k_varlen_equals_padded(engines, make_clip):
    e = engines("tiny", "q6_k")
    clips = [make_clip(c, 480000) for c in (0, 101, 102)]
    kl = [1500, 250, 33]
    want, wol = e.encode_host_padded(clips, key_len=kl)
    got, ol = e.encode_host_varlen(clips, key_len=kl)
    assert list(ol) == list(wol) == [750, 125, 16]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("wt", TYPES)
def test_group_of_one_equals_engine(engines, kq_model, make_clip, wt):
    """The blob broadcast plus the device expand (q2a_group_*, N = 1 on a one-GPU box) against the engine."""
    import q2a
    clips = [make_clip(c, 480000) for c in (0, 101)]
    ref, _ = engines("tiny", wt).encode_host(clips)
    g = q2a.Group(kq_model("tiny", wt), devices=[0])
    out, st = g.encode_host(clips)
    g.close()
    assert list(st) == [0, 0]
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))


def test_q6k_group_of_two_devices(engines, kq_model, make_clip):
    import q2a
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    clips = [make_clip(c, 480000) for c in (0, 101, 102)]
    ref, _ = engines("tiny", "q6_k").encode_host(clips)
    g = q2a.Group(kq_model("tiny", "q6_k"), devices=[0, 1])
    out, st = g.encode_host(clips)
    g.close()
    assert list(st) == [0, 0, 0]
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("wt", TYPES)
def test_q2a_main_encodes_a_quantized_file(engines, kq_model, make_clip, tmp_path, wt):
    """`q2a_tool quantize ... q5_k|q6_k` followed by bin/q2a_main (whisper_full through the reference-named API, where
    nothing is type-specific): the dumped embedding equals the engine's."""
    import wave
    import q2a
    from conftest import PKG
    if os.path.realpath(q2a.LIB_PATH) != os.path.realpath(os.path.join(PKG, "lib", "libq2a.so")):
        pytest.skip("Q2A_LIB_PATH names another build than the one the driver links")
    pcm = make_clip(0, 480000)
    s16 = np.clip(np.round(pcm * 32767.0), -32768, 32767).astype(np.int16)
    f = tmp_path / "c0.wav"
    with wave.open(str(f), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(s16.tobytes())
    dump = tmp_path / "emb.f32"
    subprocess.run([os.path.join(PKG, "bin", "q2a_main"), "-m", kq_model("tiny", wt), "-np", "-oemb", str(dump), str(f)],
                   check=True, timeout=120, capture_output=True)
    got = np.fromfile(dump, dtype=np.uint32)
    want, st = engines("tiny", wt).encode_host([s16.astype(np.float32) / 32768.0])
    assert list(st) == [0] and got.size == 750 * D
    assert np.array_equal(got, want.reshape(-1).view(np.uint32))


# ---------------------------------------------------------------- 7. the bf16 contract on a Q6_K file
@pytest.mark.parametrize("which", [0, 3])
def test_q6k_bf16_linear_matches_emulation(engines, kq_model, which):
    """Q2A_ACT_BF16: the weights are dequantize_row_q6_K's values rounded to bf16 at pack time (ggmlfile as_f32), the
    activations bf16; products exact, fp32 sums. Against the float64 emulation of tests/test_gpu_bf16_act.py, its bar."""
    import q2a
    e = engines("tiny", "q6_k", q2a.ACT_BF16)
    mf = ggmlfile.read(kq_model("tiny", "q6_k"))
    bf = lambda t: t.to(torch.bfloat16).to(t.dtype)  # noqa: E731
    w = torch.cat([bf(torch.from_numpy(t.as_f32().reshape(-1, t.ne[0]))).double() for t in kc.matrix_tensors(mf, 1, which)]).cuda()
    N, K = w.shape
    M = 1507
    x = torch.from_numpy(np.random.default_rng(7 + which).standard_normal((M, K)).astype(np.float32)).cuda()
    y = _linear(e, 1, which, x, M, N)
    ref = bf(x).double() @ w.T
    mx, l2 = rel_errors(y.cpu().numpy(), ref.cpu().numpy())
    print(f"bf16 q6_k which={which}: max-rel {mx:.3e} rel-L2 {l2:.3e}")
    assert mx < 1e-5 and l2 < 1e-6, (mx, l2)


# ---------------------------------------------------------------- 8. projector
@pytest.mark.parametrize("wt", TYPES)
@pytest.mark.parametrize("rows", [33, 1537])
def test_projector_matches_the_integer_contract(host_build, workdir, wt, rows):
    import q2a
    d_in, d_out = 768, 384
    base = os.path.join(workdir, "projector-768x384-f16.bin")
    if not os.path.exists(base):
        subprocess.check_call([TOOL, "gen-projector", base, str(d_in), str(d_out), "f16", "0x51A2"])
    path = os.path.join(workdir, f"projector-768x384-{wt}.bin")
    if not os.path.exists(path):
        subprocess.check_call([TOOL, "quantize", base, path, wt, "8"])
    mf = ggmlfile.read(path)
    wten = mf.t("multi_modal_projector.linear.weight")
    assert wten.type == kc.WT_TYPE[wt]
    bias = mf.t("multi_modal_projector.linear.bias").as_f32().reshape(-1).astype(np.float64)
    pr = q2a.Projector(path, device=0)
    try:
        assert (pr.d_in, pr.d_out, pr.wtype) == (d_in, d_out, kc.WT_TYPE[wt])
        x = np.random.default_rng(rows).standard_normal((rows, d_in)).astype(np.float32)
        xd = torch.from_numpy(x).cuda()
        yd = torch.empty((rows, d_out), dtype=torch.float32, device="cuda")
        pr.apply(xd.data_ptr(), rows, yd.data_ptr())
        torch.cuda.synchronize()
        ref = kc.kq_linear_ref([wten], x) + bias[None, :]
        mx, l2 = rel_errors(yd.cpu().numpy(), ref)
        print(f"projector {wt} rows={rows}: max-rel {mx:.3e} rel-L2 {l2:.3e}")
        assert mx < 1e-5, (mx, l2)
    finally:
        pr.close()


# ---------------------------------------------------------------- 9. full size
@pytest.mark.slow
@pytest.mark.parametrize("wt", TYPES)
def test_encoder_full_size_vs_reference_samples(kq_model, make_clip, golden_kq, wt):
    """Clip 0 inside a batch with clips 101 and 102; the sampled values against the fixture, the clip-averaged
    statistics within the widest clip-averaged pair of reference builds x1.0 (xbuild_avg_bar's rule)."""
    import q2a
    meta, kq = golden_kq
    clips = [0, 101, 102]
    bar = _kq_bar(meta, wt, clips, {"max_rel": "sampled_max_rel", "rel_l2": "sampled_rel_l2"})
    t0 = time.time()
    path = kq_model("full", wt)
    t1 = time.time()
    e = q2a.Engine(path, device=0)
    try:
        out, st = e.encode_host([make_clip(c, 480000) for c in clips])
    finally:
        e.close()
    assert list(st) == [0, 0, 0]
    idx = kq["full_idx"]
    s = [rel_errors(out[i].reshape(-1)[idx], kq[f"full_{wt}_c{c}_val"]) for i, c in enumerate(clips)]
    mx, l2 = float(np.mean([x[0] for x in s])), float(np.mean([x[1] for x in s]))
    print(f"full {wt}: model file {t1 - t0:.1f} s, open + encode {time.time() - t1:.1f} s; max-rel {mx:.3e} "
          f"(bar {bar['max_rel']:.3e}) rel-L2 {l2:.3e} (bar {bar['rel_l2']:.3e})")
    assert mx <= bar["max_rel"] and l2 <= bar["rel_l2"], (mx, l2, s, bar)
