"""Q2_K and Q3_K model files on the GPU: both run the Q4_K kernels on a Q4_K-layout blob, Q2_K against
the Q8_K operand whose min part is the sixteen raw 16-sums. References: ggml's vec_dot in float64 (tests/k23_cases.py),
the reference's outputs and cross-build spread (tests/golden/golden_k23.*). All tests need an MI355X."""
import os
import subprocess

import numpy as np
import pytest

import k23_cases as k23
import kquant_cases as kc
from conftest import GOLDEN_DIR, TOOL, _avg_bar, _sha, rel_errors
from q2a import ggmlfile

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
D, F = kc.D, kc.F
NK = {0: (3 * D, D), 1: (D, D), 2: (F, D), 3: (D, F)}


@pytest.fixture(scope="module")
def golden_k23():
    return k23.load_golden_k23(GOLDEN_DIR)


@pytest.fixture(scope="module")
def model(make_model, workdir, golden_k23):
    """model(cfg, wt): tiny, or "tinyext" (kquant_cases' hand-made rows), quantized by bin/q2a_tool; the SHA-256 is the
    reference-quantized file's."""
    def make(cfg, wt):
        path = make_model(cfg, wt) if cfg == "tiny" else os.path.join(workdir, f"tinyext-{wt}.bin")
        if not os.path.exists(path):
            ext = os.path.join(workdir, "tinyext-f16.bin")
            kc.write_ext_model(make_model("tiny", "f16"), ext)
            subprocess.check_call([TOOL, "quantize", ext, path, wt, "8"])
        assert _sha(path) == golden_k23[0]["models"][f"{cfg}-{wt}"]["sha256"], f"quantizer drift for {cfg}-{wt}"
        return path
    return make


@pytest.fixture(scope="module")
def engines(model):
    import q2a
    cache = {}

    def get(cfg, wt, act=0):
        if (cfg, wt, act) not in cache:
            cache[(cfg, wt, act)] = q2a.Engine(model(cfg, wt), device=0, act=act)
        return cache[(cfg, wt, act)]
    yield get
    for e in cache.values():
        e.close()


def _linear(e, layer, which, xd):
    yd = torch.empty((xd.shape[0], NK[which][0]), dtype=torch.float32, device="cuda")
    e.test_linear(layer, which, xd.data_ptr(), xd.shape[0], yd.data_ptr())
    torch.cuda.synchronize()
    return yd


@pytest.mark.parametrize("wt", k23.TYPES)
@pytest.mark.parametrize("which,M", [(0, 1537), (1, 1537), (2, 1537), (3, 1537), (2, 45017), (3, 131089)])
def test_linear_matches_the_integer_contract(engines, model, wt, which, M):
    """M = 1537: ragged tail, narrow tiles; the two large M are test_q5k_linear_wide_tiles' (8-phase kernel, fc2 with its
    partial last round), checked on sampled rows. fc2 (K = 1024) runs blocks 1..3 and the block-ratio recurrence. Bar: the
    one-linear bar of every weight type."""
    e, mf = engines("tiny", wt), ggmlfile.read(model("tiny", wt))
    assert e.info.wtype == k23.WT_TYPE[wt]
    g = torch.Generator(device="cuda").manual_seed(300 + which)
    xd = torch.randn((M, NK[which][1]), device="cuda", generator=g) * (1.0 if which != 3 else 0.3)
    yd = _linear(e, 1, which, xd)
    last = (M - 1) // 256 * 256
    rows = np.arange(M) if M < 4096 else np.unique(np.concatenate(
        [np.random.default_rng(which).choice(M, 600, replace=False), [0, 255, 256, 511, last - 1], np.arange(last, M)]))
    ri = torch.from_numpy(rows).cuda()
    ref, _ = k23.k23_linear_ref(kc.matrix_tensors(mf, 1, which), xd[ri].cpu().numpy())
    mx, l2 = rel_errors(yd[ri].cpu().numpy(), ref)
    print(f"linear {wt} which={which} M={M}: max-rel {mx:.3e} rel-L2 {l2:.3e}")
    assert mx < 1e-5 and l2 < 1e-6, (mx, l2)


@pytest.mark.parametrize("wt", k23.TYPES)
@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_linear_extremes(engines, model, wt, which):
    """The hand-made rows (d = 0 beside dmin != 0, q = 3 with sc = 15; negative d, (sc - 32)(q - 4) = 128) against
    one-sign full-scale activations, test_linear_extremes' rule: the bar, and each hand-made row within 1e-5 of the
    magnitude of the terms it sums."""
    e, mf = engines("tinyext", wt), ggmlfile.read(model("tinyext", wt))
    x = np.random.default_rng(50 + which).uniform(0.9, 1.0, (1537, NK[which][1])).astype(np.float32)
    x[0] = 1.0
    y = _linear(e, 0, which, torch.from_numpy(x).cuda()).cpu().numpy()
    ref, mag = k23.k23_linear_ref(kc.matrix_tensors(mf, 0, which), x)
    mx, l2 = rel_errors(y, ref)
    print(f"extremes {wt} which={which}: max-rel {mx:.3e} rel-L2 {l2:.3e}")
    assert mx < 1e-5 and l2 < 1e-6, (mx, l2)
    for r in range(kc.EXT_ROWS):
        d = np.abs(y[:, r] - ref[:, r]).max()
        assert d <= 1e-5 * mag[:, r].max(), (r, d, mag[:, r].max())


LN, QF32, QH16, GELU = 0, 1, 2, 3


@pytest.mark.parametrize("M", [1, 7, 8, 9, 1537])
@pytest.mark.parametrize("producer,K", [(LN, 256), (LN, 1280), (QF32, 256), (QF32, 1280), (QF32, 4096), (QH16, 1024), (GELU, 1024)])
def test_raw_16_sum_operand(engines, producer, K, M):
    """Mode 5 against mode 1 of the same kernel family: codes and d bit for bit, aext = the integer 16-sums of the codes.
    K = 1280 takes the 8-rows-per-workgroup kernels (rows 7, 8, 9 straddle a group), 4096 the segmented rows."""
    e = engines("tiny", "q2_k")
    rng = np.random.default_rng(K + M)
    x = (rng.standard_normal((M, K)) * 3).astype(np.float32)
    if M * K > 256:
        x[0, :256] = 0                                    # an all-zero block beside live ones
    xd = torch.from_numpy(x).cuda() if producer in (LN, QF32) else torch.from_numpy(x).cuda().half()
    gb = [torch.from_numpy(rng.standard_normal(K).astype(np.float32)).cuda() for _ in range(2)] if producer == LN else None
    got = {}
    for mode in (1, 5):
        out = torch.zeros((M, K), dtype=torch.float16, device="cuda")
        dy = torch.zeros((K // 256, M), dtype=torch.float32, device="cuda")
        ae = torch.zeros((K // 256, M, 16), dtype=torch.float16, device="cuda")
        e.test_operand(producer, mode, xd.data_ptr(), M, K, out.data_ptr(), dy.data_ptr(), ae.data_ptr(), ld=M,
                       g_ptr=gb[0].data_ptr() if gb else 0, b_ptr=gb[1].data_ptr() if gb else 0)
        torch.cuda.synchronize()
        got[mode] = (out.cpu(), dy.cpu(), ae.cpu())
    assert torch.equal(got[1][0].view(torch.int16), got[5][0].view(torch.int16))
    assert torch.equal(got[1][1].view(torch.int32), got[5][1].view(torch.int32))
    sums = got[5][0].double().view(M, K // 256, 16, 16).sum(-1).permute(1, 0, 2)
    assert torch.equal(got[5][2].double(), sums)
    assert sums.abs().max() > 0


@pytest.mark.parametrize("cfg,wt,act", [(c, w, a) for c in ("tiny", "tinyext") for w in k23.TYPES for a in (0, 1)])
def test_compact_blob_expands_to_the_host_pack_bytes(model, cfg, wt, act):
    import q2a
    path = model(cfg, wt)
    full, comp = q2a.pack_model(path, act), q2a.pack_model(path, act, compact=True)
    assert q2a.blob_device_size(comp) == (len(full), len(comp))
    cd = torch.frombuffer(comp, dtype=torch.uint8).cuda()
    out = torch.full((len(full),), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    q2a.expand_blob(cd.data_ptr(), len(comp), out.data_ptr(), len(full), 0)
    torch.cuda.synchronize()
    eq = out == torch.frombuffer(full, dtype=torch.uint8).cuda()
    assert bool(eq.all()), f"{int((~eq).sum())} bytes differ, first at {int((~eq).nonzero()[0])}"


@pytest.mark.parametrize("wt", k23.TYPES)
def test_encoder_tiny_vs_reference(engines, make_clip, golden, golden_k23, wt):
    """Clips 0 and 101..104 on rows_stride5, clip-averaged, within the fixture's widest clip-averaged pair of reference
    builds x1.0 (tiny_avg_bar's rule)."""
    meta, arr = golden_k23
    rows, clips = golden[1]["rows_stride5"], [0, 101, 102, 103, 104]
    bar = _avg_bar([meta[f"tiny_{wt}"]] + [meta[f"tiny_{wt}_clip{c}"] for c in clips[1:]],
                   {"max_rel": "rows_max_rel", "rel_l2": "rows_rel_l2"})
    out, st = engines("tiny", wt).encode_host([make_clip(c, 480000) for c in clips])
    assert list(st) == [0] * len(clips)
    s = [rel_errors(out[i][rows], arr[f"tiny_{wt}_c{c}_rows"]) for i, c in enumerate(clips)]
    mx, l2 = float(np.mean([x[0] for x in s])), float(np.mean([x[1] for x in s]))
    print(f"tiny {wt}: max-rel {mx:.3e} (bar {bar['max_rel']:.3e}) rel-L2 {l2:.3e} (bar {bar['rel_l2']:.3e})")
    assert mx <= bar["max_rel"] and l2 <= bar["rel_l2"], (mx, l2, bar)


def test_q2k_batch_independence_and_varlen(engines, make_clip):
    e = engines("tiny", "q2_k")
    clips = [make_clip(c, 480000) for c in (0, 101, 102)]
    alone, _ = e.encode_host([clips[0]])
    batch, st = e.encode_host([clips[0], clips[1], clips[0]])
    assert list(st) == [0, 0, 0]
    assert np.array_equal(alone[0].view(np.uint32), batch[0].view(np.uint32))
    assert np.array_equal(alone[0].view(np.uint32), batch[2].view(np.uint32))
    kl = [1500, 250, 33]
    want, wol = e.encode_host_padded(clips, key_len=kl)
    got, ol = e.encode_host_varlen(clips, key_len=kl)
    assert list(ol) == list(wol) == [750, 125, 16]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("wt", k23.TYPES)
def test_embedding_gather(wt, dt):
    """float32(the float64 formula of dequantize_row_q2_K / _q3_K) cast once to the destination type, bit for bit, at the
    row count and column widths of test_gpu_embed_qtable (n_cols 256 and 512: padded rows; 4096: whole passes)."""
    import ctypes as C
    import q2a
    t, dtype = k23.WT_TYPE[wt], {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[dt]
    fn = getattr(q2a._host(), "q2a_quantize_row_" + wt.replace("k", "K"))
    fn.argtypes, fn.restype = [C.c_void_p, C.c_void_p, C.c_int64], None
    for n_cols, width in ((256, 4), (512, 8), (4096, 4)):
        rs = ggmlfile.row_size(t, n_cols)
        rng = np.random.default_rng(n_cols)
        x = (rng.standard_normal((281, n_cols)) * (10.0 ** (np.arange(281) % 3 * 3 - 4))[:, None]).astype(np.float32)
        rows = np.zeros((281 + 8, rs), dtype=np.uint8)
        for i in range(281):
            fn(x[i].ctypes.data_as(C.c_void_p), rows[i].ctypes.data_as(C.c_void_p), n_cols)
        end = rows[281:].reshape(8, n_cols // 256, rs // (n_cols // 256))   # end codes: all bits / no bits, d and dmin rotating
        end[:4], end[4:] = 0xFF, 0x00
        for v in range(8):
            for b in range(n_cols // 256):
                end[v, b, -4 if wt == "q2_k" else -2:] = np.array([[0x7BFF, 0x0001, 0x0000, 0xB266][(v + b + i) % 4] for i in range(2)],
                                                                  dtype="<u2").view(np.uint8)[:4 if wt == "q2_k" else 2]
        v = ggmlfile.Tensor("t", t, (n_cols, len(rows)), rows.reshape(-1)).kq()
        d, shape = v["d"].astype(np.float64)[..., None, None], (len(rows), n_cols // 256, 16, 16)
        if wt == "q2_k":
            y = d * v["sc"][..., None] * v["q"].reshape(shape) - (v["dmin"].astype(np.float64)[..., None] * v["m"])[..., None]
        else:
            y = d * (v["sc"] - 32)[..., None] * (v["q"].reshape(shape) - 4)
        vals = torch.from_numpy(y.reshape(len(rows), n_cols).astype(np.float32))
        qt = q2a.QuantTable.from_host(rows, t, n_cols)
        n, audio = 1237, 7
        ids = rng.integers(0, len(rows), size=n).astype(np.int32 if width == 4 else np.int64)
        ids[rng.random(n) < 0.2] = audio
        ids[20:28] = np.arange(281, 289)
        dst = torch.zeros((n, n_cols + 64), dtype=dtype, device="cuda")
        report = torch.zeros(4, dtype=torch.int32, device="cuda")
        ids_dev = torch.from_numpy(ids).cuda()
        src = q2a.embeds_src(ids_dev.data_ptr(), width, n, audio, report_ptr=report.data_ptr())
        q2a.test_embed_gather_q(src, qt, q2a.feat_dst(dst.data_ptr(), n_cols + 64, n, {"f32": q2a.DT_F32, "f16": q2a.DT_F16, "bf16": q2a.DT_BF16}[dt]), n_cols)
        torch.cuda.synchronize()
        text = np.flatnonzero(ids != audio)
        want = vals[torch.from_numpy(ids[text].astype(np.int64))].to(dtype)
        got = dst.cpu()[torch.from_numpy(text), :n_cols]
        ib = torch.int32 if dt == "f32" else torch.int16
        assert torch.equal(got.view(ib), want.view(ib)), (wt, dt, n_cols)
        assert not bool(dst.cpu()[:, n_cols:].any()) and report.cpu().tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("wt", k23.TYPES)
def test_bf16_linear_matches_emulation(engines, model, wt):
    """Q2A_ACT_BF16 on fc2: dequantize_row_* values rounded to bf16 at pack time, bf16 activations, fp32 sums; against the
    float64 emulation at tests/test_gpu_bf16_act.py's bar."""
    import q2a
    e, mf = engines("tiny", wt, q2a.ACT_BF16), ggmlfile.read(model("tiny", wt))
    bf = lambda t: t.to(torch.bfloat16).to(t.dtype)  # noqa: E731
    w = torch.cat([bf(torch.from_numpy(t.as_f32().reshape(-1, t.ne[0]))).double() for t in kc.matrix_tensors(mf, 1, 3)]).cuda()
    x = torch.from_numpy(np.random.default_rng(7).standard_normal((1507, F)).astype(np.float32)).cuda()
    y = _linear(e, 1, 3, x)
    mx, l2 = rel_errors(y.cpu().numpy(), (bf(x).double() @ w.T).cpu().numpy())
    print(f"bf16 {wt}: max-rel {mx:.3e} rel-L2 {l2:.3e}")
    assert mx < 1e-5 and l2 < 1e-6, (mx, l2)
