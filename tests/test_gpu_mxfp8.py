"""The MXFP8 activation contract (Q2A_ACT_MXFP8) on the GPU, tiny Q8_0 model (D = 256, F = 1024: 2 and
8 K-steps): the operand kernels bit for bit against the numpy rule (tests/mxfp8_cases.py), one linear and one block
against float64 emulations of the contract, the encode against the golden Q8_0 rows, and the refusals."""
import ctypes as C
import os
import subprocess
import wave
from contextlib import closing

import numpy as np
import pytest

import q2a
from conftest import PKG, rel_errors
from mxfp8_cases import mx_quant, mx_value
from q2a import ggmlfile
from test_gpu_bf16_act import D_TINY, H_TINY, bf, block_emulation, dequant, gelu_lut, layer_norm, vec

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def eng(make_model):
    e = q2a.Engine(make_model("tiny", "q8_0"), device=0, act=q2a.ACT_MXFP8)
    yield e
    e.close()


def mxq(t: torch.Tensor) -> torch.Tensor:   # the value of the MX quantisation of t along its last axis, float64
    return torch.from_numpy(mx_value(*mx_quant(t.double().cpu().numpy()))).to(t.device)


w_mx = lambda mf, name: mxq(torch.from_numpy(dequant(mf.t(name))).float()).cuda()   # noqa: E731


@pytest.mark.parametrize("K", [256, 1024])
@pytest.mark.parametrize("M", [1, 17, 300])
@pytest.mark.parametrize("form", ["bf16_rows", "ln"])
def test_operand_matches_rule(eng, form, M, K):
    """A zero row, one huge element, values straddling the powers of two. bf16 rows: every byte equal. LN: the row in float64
    rounded to f32; the kernel's f32 chain ((x - mean) * scale) * g + b (four roundings, f32 mean and scale) is within 8 ulps
    of its larger term, delta = 2^-21 (|y - b| + |b|): a code may differ only where moving the reference by delta changes it,
    and the reference's share of such elements stays under 0.1 % (measured <= 9.1e-5; no mismatch, 6.5e-6 on another draw)."""
    rng = np.random.default_rng(M * K)
    x = rng.standard_normal((M, K)).astype(np.float32)
    x[0], x[M // 2, 5] = 0.0, (50.0 if form == "ln" else 3.0e30)   # (LN: a finite variance)
    x[-1, ::7] = np.float32(2.0) ** (np.arange(len(x[-1, ::7])) % 24 - 12) * np.float32(1 - 2.0 ** -8)
    x[-1, 3::7] = np.float32(2.0) ** (np.arange(len(x[-1, 3::7])) % 24 - 12)
    g, b = rng.standard_normal(K).astype(np.float32), rng.standard_normal(K).astype(np.float32)
    xd, gd, bd = (torch.from_numpy(a).cuda() for a in (x, g, b))
    out, sc = (torch.full((M, n), 0xAA, dtype=torch.uint8, device="cuda") for n in (K, K // 32))
    if form == "ln":
        eng.test_operand(q2a.OPERAND_LN, 6, xd.data_ptr(), M, K, out.data_ptr(), dy_ptr=sc.data_ptr(), g_ptr=gd.data_ptr(), b_ptr=bd.data_ptr())
        y = layer_norm(xd.double(), gd.double(), bd.double()).float().cpu().numpy()
        delta = (np.abs(y.astype(np.float64) - b) + np.abs(b)) * 2.0 ** -21
    else:
        xb = xd.to(torch.bfloat16)
        eng.test_operand(q2a.OPERAND_QUANT_H16, 6, xb.data_ptr(), M, K, out.data_ptr(), dy_ptr=sc.data_ptr())
        y, delta = xb.float().cpu().numpy(), 0.0
    (want8, wantsc), (up8, upsc), (dn8, dnsc) = mx_quant(y), mx_quant(y + delta), mx_quant(y - delta)
    near_blk = (upsc != wantsc) | (dnsc != wantsc)
    near = (up8 != want8) | (dn8 != want8) | np.repeat(near_blk, 32, axis=1)
    got8, gotsc = out.cpu().numpy(), sc.cpu().numpy()
    assert near.mean() <= 1e-3, near.mean()
    assert not ((got8 != want8) & ~near).any() and not ((gotsc != wantsc) & ~near_blk).any()


# One linear against the exact sum of the MX values. Target: the bf16-linear bar (1e-5 max-rel of the largest |y|, 1e-6
# rel-L2). What is left is the scaled MFMA's undocumented summation inside a K-step, measured over the 16 cases at max-rel
# 1.3e-5 .. 3.2e-5, rel-L2 1.15e-5 .. 1.6e-5 in both tile forms: above a third of the target, so 3x the worst
LINEAR_BAR = (3 * 3.2e-5, 3 * 1.6e-5)
BLOCK_BAR = 3 * 1.55e-3    # 3x the measured kernel-to-emulation rel-L2 (1.545e-3 at 1, 30 and 44 clips; the emulations' gap 1.32e-2)
ENCODE_BAR = 3 * 1.38e-2   # 3x the measured rel-L2 against the golden reference Q8_0 rows (max-rel 1.9e-2; bf16: 2.1e-3 / 1.5e-3)


@pytest.mark.parametrize("M", [1, 129, 1500 + 7, 45000 + 17])   # small tile, row guard, partial last round, wide tile
@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_mxfp8_linear_matches_emulation(eng, make_model, which, M):
    mf = ggmlfile.read(make_model("tiny", "q8_0"))
    names = {0: ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"], 1: ["self_attn.out_proj"], 2: ["fc1"], 3: ["fc2"]}[which]
    w = torch.cat([w_mx(mf, f"layers.1.{n}.weight") for n in names])
    (N, K), u = w.shape, min(M, 256)   # u distinct rows (the emulation's quantiser runs on these), repeated to M
    xu = torch.from_numpy(np.random.default_rng(7 + which).standard_normal((u, K)).astype(np.float32)).cuda()
    idx = torch.arange(M, device="cuda") % u
    x = xu[idx].contiguous()
    y = torch.empty((M, N), dtype=torch.float32, device="cuda")
    eng.test_linear(1, which, x.data_ptr(), M, y.data_ptr())   # (on the default stream: y.cpu() waits for it)
    mx, l2 = rel_errors(y.cpu().numpy(), (mxq(bf(xu)) @ w.T)[idx].cpu().numpy())
    print(f"mxfp8 linear which={which} M={M}: max-rel {mx:.3e} rel-L2 {l2:.3e}")
    assert mx < LINEAR_BAR[0] and l2 < LINEAR_BAR[1], (mx, l2)


def block_emulation_mx(mf, layer, x, T, H):
    """block_emulation of test_gpu_bf16_act.py with the three MX quantisations of the GEMM operands inserted."""
    p = f"layers.{layer}."
    D = x.shape[-1]
    xb = x.double().reshape(-1, T, D)
    a = mxq(layer_norm(xb, vec(mf, p + "self_attn_layer_norm.weight"), vec(mf, p + "self_attn_layer_norm.bias")).float())
    q = bf((a @ w_mx(mf, p + "self_attn.q_proj.weight").T + vec(mf, p + "self_attn.q_proj.bias")) * 0.125)
    k = bf(a @ w_mx(mf, p + "self_attn.k_proj.weight").T)
    v = bf(a @ w_mx(mf, p + "self_attn.v_proj.weight").T + vec(mf, p + "self_attn.v_proj.bias"))
    B = xb.shape[0]
    qh, kh, vh = (t.reshape(B, T, H, 64).transpose(1, 2) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2)
    pr = torch.exp(s - s.amax(-1, keepdim=True))
    o = mxq(bf(((bf(pr) @ vh) / pr.sum(-1, keepdim=True)).transpose(1, 2).reshape(B, T, D)))
    x1 = o @ w_mx(mf, p + "self_attn.out_proj.weight").T + vec(mf, p + "self_attn.out_proj.bias") + xb
    a2 = mxq(layer_norm(x1, vec(mf, p + "final_layer_norm.weight"), vec(mf, p + "final_layer_norm.bias")).float())
    h = mxq(bf(gelu_lut(a2 @ w_mx(mf, p + "fc1.weight").T + vec(mf, p + "fc1.bias"))))
    return (h @ w_mx(mf, p + "fc2.weight").T + vec(mf, p + "fc2.bias") + x1).reshape(-1, D)


@pytest.mark.parametrize("n_clips", [1, 30, 44])   # 44: 66 000 rows, O and fc2 (N = 256) on the 256x256 RESID tiles + a tail
def test_mxfp8_block_matches_emulation(eng, make_model, n_clips):
    mf, T = ggmlfile.read(make_model("tiny", "q8_0")), 1500
    x0 = torch.from_numpy((np.random.default_rng(11).standard_normal((T, D_TINY)) * 0.5).astype(np.float32)).cuda()
    x = x0.repeat(n_clips, 1)
    ref = block_emulation_mx(mf, 0, x0, T, H_TINY).cpu().numpy()
    _, gap = rel_errors(ref, block_emulation(mf, 0, x0, T, H_TINY).cpu().numpy())
    eng.test_block(0, x.data_ptr(), n_clips)
    out = x.cpu().numpy().reshape(n_clips, T, D_TINY)
    mx, l2 = rel_errors(out[0], ref)
    print(f"mxfp8 block n_clips={n_clips}: kernel-to-emulation max-rel {mx:.3e} rel-L2 {l2:.3e}; MXFP8-to-bf16 emulations rel-L2 {gap:.3e}")
    assert np.array_equal(out[0], out[-1])
    assert l2 <= gap / 4 and l2 < BLOCK_BAR, (l2, gap)   # a quarter of the two emulations' distance, and 3x the measured value


def test_mxfp8_encode_tiny(eng, make_model, make_clip, golden):   # finite; same bytes alone, in a batch of 4, from a device blob
    _, g = golden
    pcm = [make_clip(0)] + [make_clip(100 + i, 480000) for i in range(3)]
    d = torch.from_numpy(np.stack(pcm)).cuda()
    out = torch.empty((4,) + eng.out_shape, dtype=torch.float32, device="cuda")
    st1 = eng.encode_device(d.data_ptr(), d.shape[1], [d.shape[1]], out.data_ptr())
    alone = out.cpu().numpy()[:1]
    st4 = eng.encode_device(d.data_ptr(), d.shape[1], [d.shape[1]] * 4, out.data_ptr())
    batch = out.cpu().numpy()
    assert st1[0] == 0 and list(st4) == [0] * 4 and np.isfinite(batch).all() and np.array_equal(alone[0], batch[0])
    mx, l2 = rel_errors(batch[0][g["rows_stride5"]], g["tiny_q8_0_c0_rows"])
    print(f"mxfp8 encode tiny vs golden Q8_0: max-rel {mx:.3e} rel-L2 {l2:.3e}")
    assert l2 < ENCODE_BAR, (mx, l2)
    dev = torch.frombuffer(bytearray(q2a.pack_model(make_model("tiny", "q8_0"), q2a.ACT_MXFP8)), dtype=torch.uint8).cuda()
    with closing(q2a.Engine(device=0, device_blob=dev.data_ptr(), blob_size=dev.numel())) as e1:
        assert e1.info.act == eng.info.act == q2a.ACT_MXFP8 and np.array_equal(e1.encode_host([pcm[0]])[0], alone)


def test_mxfp8_through_q2a_main(eng, make_model, make_clip, tmp_path):   # bin/q2a_main -mxfp8 (Q2A_ACT=mxfp8): the engine's bytes
    s16, wav, emb = np.clip(np.round(make_clip(0) * 32767.0), -32768, 32767).astype(np.int16), str(tmp_path / "c0.wav"), tmp_path / "emb.f32"
    with wave.open(wav, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(s16.tobytes())
    ref, _ = eng.encode_host([s16.astype(np.float32) / np.float32(32768.0)])
    for extra in ([], ["-b"]):   # whisper_full, and the batched entry point (one device under this contract)
        subprocess.run([os.path.join(PKG, "bin", "q2a_main"), "-m", make_model("tiny", "q8_0"), "-np", "-mxfp8", *extra, "-oemb", str(emb), wav],
                       capture_output=True, text=True, timeout=300, check=True)
        assert np.array_equal(np.fromfile(emb, dtype=np.float32).reshape(ref[0].shape), ref[0]), extra


@pytest.mark.parametrize("call", ["padded", "varlen", "features", "inputs_embeds", "gemm_epi", "bf16_key_lengths", "projector", "group"])
def test_mxfp8_refusals(eng, make_model, call):
    L, T, D = q2a.lib(), eng.info.n_audio_ctx, eng.info.n_audio_state   # (each call: its code, the poisoned output untouched)
    pcm = torch.zeros((1, 32000), dtype=torch.float32, device="cuda")
    out = torch.full((T // 2 * D,), 7.0, dtype=torch.float32, device="cuda")
    if call in ("projector", "group"):
        L.q2a_group_open.restype = L.q2a_group_open_with.restype = C.c_void_p
        path = make_model("tiny", "q8_0").encode()
        h = L.q2a_projector_open_ex(path, 0, q2a.ACT_MXFP8) if call == "projector" else L.q2a_group_open(path, None, 0, q2a.ACT_MXFP8)
        assert not h and b"MXFP8" in L.q2a_last_error()
        assert call == "projector" or (not L.q2a_group_open_with(C.c_void_p(eng.h), None, 0) and b"MXFP8" in L.q2a_last_error())
        return
    ids = torch.full((T // 2,), 9, dtype=torch.int32, device="cuda")   # every token the audio token: dst is all feature rows
    dst, src = q2a.feat_dst(out.data_ptr(), D, T // 2, q2a.DT_F32), q2a.embeds_src(ids.data_ptr(), 4, T // 2, 9)
    calls = {"inputs_embeds": lambda: eng.inputs_embeds_device(pcm.data_ptr(), 32000, [32000], dst, src, None),
             "padded": lambda: eng.encode_device_padded(pcm.data_ptr(), 32000, [32000], out.data_ptr(), key_len=[100]),
             "varlen": lambda: eng.encode_device_varlen(pcm.data_ptr(), 32000, [32000], out.data_ptr(), key_len=[100]),
             "features": lambda: eng.audio_features_device(pcm.data_ptr(), 32000, [32000], 0, out.data_ptr(), T // 2),
             "gemm_epi": lambda: eng.test_gemm_epi(0, 1, 1, pcm.data_ptr(), 16, [out.data_ptr()]),
             "bf16_key_lengths": lambda: eng.set_bf16_key_lengths(True)}
    with pytest.raises(q2a.Q2AError) as ei:
        calls[call]()
    # Q2A_ERR_ARG as on any non-bf16 engine, else Q2A_ERR_UNSUPPORTED; the comparison synchronises
    assert ei.value.rc == (-4 if call == "bf16_key_lengths" else -6) and bool((out == 7.0).all()), (call, ei.value.rc)
