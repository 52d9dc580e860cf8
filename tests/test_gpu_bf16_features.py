"""bf16-activation engines: the bf16 projector (q2a_projector_open_ex), the bf16 x bf16 row-map GEMM epilogue, the pool
kernel's bf16 operand and the audio_features / inputs_embeds calls of a bf16 engine + projector pair. The GEMM is held
against float64 under a derived bound; everything else is bit for bit against the composition of the existing calls.
Destinations, clips and the whole-buffer check are tests/test_gpu_features_to.py's. All tests need an MI355X."""
import numpy as np
import pytest

import embed_q_cases as qc
from test_gpu_features_to import (DTYPES, ERR_UNSUPPORTED, S16, T, _check_dest, _dt, _ibits, _reverse_rows, _sentinel,   # noqa: F401
                                  batch13, projector_path)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# (file type, d_in, M, regime): every M has a partial last tile; F16 / Q4_K / Q6_K at M = 1003 so each decode reaches W
CASES = [("q8_0", 256, 203, "NARROW"), ("q8_0", 256, 1003, "128"), ("q8_0", 256, 8003, "PIPE8"), ("f16", 320, 8003, "256"),
         ("f16", 256, 1003, "128"), ("q4_k", 256, 1003, "128"), ("q6_k", 256, 1003, "128")]


@pytest.mark.parametrize("wt,d_in,M,regime", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_gemm_and_row_map_epilogue(projector_path, wt, d_in, M, regime):
    """apply against ref = bf16(x) @ bf16(W)^T + bias in float64, every element, under the any-order f32 summation bound
    with one more rounding for the bias: (K + 2) 2^-24 (sum_k |bf16(x_k) bf16(w_k)| + |bias|) — room for the MFMA's
    internal order, none for a wrong or missing K-step. Then apply_to = that f32 result cast on the CPU, bit for bit, the
    sentinel everywhere else (guard rows included); at M = 1003 also through a permutation whose entries < 0 and
    >= n_rows are dropped."""
    import q2a
    from q2a import ggmlfile
    path = projector_path(d_in, 4096, wt)
    mf = ggmlfile.read(path)
    wf = mf.t("multi_modal_projector.linear.weight")
    w = wf.as_f32().reshape(-1) if wt == "f16" else q2a.dequantize_row(wf.type, wf.data, 4096 * d_in)
    wb = torch.from_numpy(w.reshape(4096, d_in).copy()).bfloat16().double()
    bias = torch.from_numpy(mf.t("multi_modal_projector.linear.bias").as_f32().reshape(-1).copy()).double()
    pr = q2a.Projector(path, 0, q2a.ACT_BF16)
    assert pr.act == q2a.ACT_BF16 and pr.regime(M) == getattr(q2a, "REGIME_" + regime)
    x = torch.randn((M, d_in), device="cuda", generator=torch.Generator(device="cuda").manual_seed(7 * d_in + M))
    yd = torch.empty((M, 4096), device="cuda")
    pr.apply(x.data_ptr(), M, yd.data_ptr())
    torch.cuda.synchronize()
    y, xb = yd.cpu(), x.cpu().bfloat16().double()
    ratio = (y.double() - (xb @ wb.T + bias)).abs() / ((d_in + 2) * 2.0 ** -24 * (xb.abs() @ wb.abs().T + bias.abs()))
    print(f"{wt} {regime}: worst |y - ref| / bound {float(ratio.max()):.3e}")
    assert bool((ratio <= 1).all()), f"{int((ratio > 1).sum())} elements past the bound, worst ratio {float(ratio.max())}"
    rm = np.random.default_rng(17).permutation(M + 37)[:M].astype(np.int32)
    rm[[0, 127, 128, M // 2, M - 1]] = [-1, M + 37, -2 ** 31, 2 ** 31 - 1, M + 42]
    for dt, row_of in [("bf16", None), ("f16", None), ("f32", None)] + ([("bf16", rm)] if M == 1003 else []):
        n_rows = M if row_of is None else M + 37
        dst = _sentinel(n_rows + 5, 4096, DTYPES[dt])
        rmd = torch.from_numpy(row_of).cuda() if row_of is not None else None
        pr.apply_to(x.data_ptr(), M, q2a.feat_dst(dst.data_ptr(), 4096, n_rows, _dt(dt)), rmd.data_ptr() if rmd is not None else 0)
        torch.cuda.synchronize()
        _check_dest(dst, y.to(DTYPES[dt]), np.arange(M) if row_of is None else row_of, 4096, f"{wt} {regime} {dt}", n_rows=n_rows)
    pr.close()


@pytest.fixture(scope="module")
def pair(make_model, projector_path):
    """bf16 tiny Q8_0 engines with and without the opt-in, a reference one, and the bf16 / reference Q8_0 projectors."""
    import q2a
    m, p = make_model("tiny", "q8_0"), projector_path(256, 4096, "q8_0")
    hs = (q2a.Engine(m, act=q2a.ACT_BF16, bf16_key_lengths=True), q2a.Engine(m, act=q2a.ACT_BF16), q2a.Engine(m),
          q2a.Projector(p, 0, q2a.ACT_BF16), q2a.Projector(p))
    yield hs
    for h in hs:
        h.close()


def test_pool_operand_bf16(pair):
    """Mode 4: the bf16 rows are the call's own f32 embd rows rounded to nearest even, embd is mode 0's, no row past N_tot."""
    import q2a
    e, lens = pair[0], [1, 2, 3, 15, 16, 17, 31, 33, 365, 1500]
    m_tot, n_tot = q2a.varlen_rows(lens, T)[0], q2a.packed_out_rows(lens)[0]
    x = torch.randn((m_tot, 256), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    got = {}
    for mode in (4, 0):
        embd, codes = _sentinel(n_tot + 2, 256, torch.float32), _sentinel(n_tot + 2, 256, torch.bfloat16)
        e.test_pool_operand(mode, x.data_ptr(), len(lens), lens, embd.data_ptr(), codes.data_ptr())
        torch.cuda.synchronize()
        got[mode] = (embd.cpu(), codes.cpu())
    embd, codes = got[4]
    _check_dest(embd, got[0][0][:n_tot], np.arange(n_tot), 256, "embd against mode 0", n_rows=n_tot)
    assert bool((_ibits(embd[:n_tot]) != 0x5A5A5A5A).any(1).all())
    _check_dest(codes, embd[:n_tot].to(torch.bfloat16), np.arange(n_tot), 256, "bf16 operand", n_rows=n_tot)


@pytest.fixture(scope="module")
def composed(pair, batch13):
    """encode_device_varlen + the valid rows + Projector.apply on batch13 -> (embd, feat) f32 on the CPU; computed once."""
    (pcm, stride, ns), lens, want = batch13
    out = torch.zeros((len(ns), T // 2, 256), device="cuda")
    ol, _ = pair[0].encode_device_varlen(pcm.data_ptr(), stride, ns, out.data_ptr(), key_len=lens)
    assert list(ol) == want
    rows = torch.cat([out[c, :n] for c, n in enumerate(want)]).contiguous()
    feat = torch.empty((rows.shape[0], 4096), device="cuda")
    pair[3].apply(rows.data_ptr(), rows.shape[0], feat.data_ptr())
    torch.cuda.synchronize()
    return rows.cpu(), feat.cpu()


def test_audio_features_equal_the_composition(pair, batch13, composed):
    """The f32 call, the bf16 _to call with gaps between the clips' rows, and log-mel against PCM on three of the clips."""
    import q2a
    e, pr = pair[0], pair[3]
    (pcm, stride, ns), lens, want = batch13
    n_tot = sum(want)
    feat, embd = _sentinel(n_tot + 2, 4096, torch.float32), _sentinel(n_tot + 2, 256, torch.float32)
    ol, _ = e.audio_features_device(pcm.data_ptr(), stride, ns, feat.data_ptr(), embd.data_ptr(), n_tot, projector=pr, key_len=lens)
    torch.cuda.synchronize()
    assert list(ol) == want
    _check_dest(embd, composed[0], np.arange(n_tot), 256, "embd", n_rows=n_tot)
    _check_dest(feat, composed[1], np.arange(n_tot), 4096, "feat", n_rows=n_tot)
    clip_row, n_rows = _reverse_rows(want)
    dst = _sentinel(n_rows + 3, 4096 + 64, torch.bfloat16)
    e.audio_features_device_to(pcm.data_ptr(), stride, ns, q2a.feat_dst(dst.data_ptr(), 4096 + 64, n_rows, q2a.DT_BF16), pr,
                               clip_rows=clip_row, key_len=lens)
    torch.cuda.synchronize()
    _check_dest(dst, composed[1].to(torch.bfloat16), q2a.feat_rows(want, clip_row, n_rows)[1], 4096, "_to", n_rows=n_rows)
    pick = [lens.index(k) for k in (17, 365, 1500)]
    kl, sub = [lens[c] for c in pick], pcm[pick].contiguous()
    md = torch.from_numpy(np.stack([e.pcm_to_mel(c) for c in sub.cpu().numpy()])).cuda()
    fp, fm = (_sentinel(sum(k // 2 for k in kl), 4096, torch.float32) for _ in range(2))
    e.audio_features_device(sub.data_ptr(), stride, [ns[c] for c in pick], fp.data_ptr(), 0, fp.shape[0], projector=pr, key_len=kl)
    e.audio_features_device_mel(md.data_ptr(), md.shape[1] * md.shape[2], md.shape[2], [md.shape[2]] * 3, fm.data_ptr(), 0, fm.shape[0],
                                projector=pr, key_len=kl)
    torch.cuda.synchronize()
    assert torch.equal(_ibits(fp), _ibits(fm)) and bool((_ibits(fp) != 0x5A5A5A5A).all())


@pytest.mark.parametrize("table", ["dense", "q8_0"])
def test_inputs_embeds_equal_the_composition(pair, batch13, composed, table):
    """int64 ids with a dense bf16 table, or (the _q call) a Q8_0 table of ggml blocks: table[ids] with the k-th feature
    row of the composition, cast to bf16, at the k-th audio token."""
    import q2a
    e, pr = pair[0], pair[3]
    (pcm, stride, ns), lens, want = batch13
    n_feat, audio = sum(want), 151646
    n_tok = n_feat + 61
    qt = q2a.QuantTable.from_host(qc.rows(qc.Q8_0, 4096), qc.Q8_0, 4096)
    tab = (torch.from_numpy(qc.values(qc.Q8_0, 4096).copy()) if table == "q8_0"
           else torch.randn((qt.vocab, 4096), generator=torch.Generator().manual_seed(5))).bfloat16()
    rng = np.random.default_rng(11)
    ids = rng.integers(0, qt.vocab, size=n_tok).astype(np.int64)
    ids[rng.permutation(n_tok)[:n_feat]] = audio
    ids_dev, tab_dev = torch.from_numpy(ids).cuda(), tab.cuda()
    dst = _sentinel(n_tok + 3, 4096, torch.bfloat16)
    report = torch.zeros(4, dtype=torch.int32, device="cuda")
    fd = q2a.feat_dst(dst.data_ptr(), 4096, n_tok, q2a.DT_BF16)
    if table == "q8_0":
        src = q2a.embeds_src(ids_dev.data_ptr(), 8, n_tok, audio, report_ptr=report.data_ptr())
        ol, _ = e.inputs_embeds_device_q(pcm.data_ptr(), stride, ns, fd, src, qt, pr, key_len=lens)
    else:
        src = q2a.embeds_src(ids_dev.data_ptr(), 8, n_tok, audio, tab_dev.data_ptr(), qt.vocab, 4096, report.data_ptr())
        ol, _ = e.inputs_embeds_device(pcm.data_ptr(), stride, ns, fd, src, pr, key_len=lens)
    torch.cuda.synchronize()
    assert list(ol) == want and report.cpu().tolist() == [n_feat, n_feat, 0, 0]
    rows = tab[torch.from_numpy(np.where(ids == audio, 0, ids))]
    rows[torch.from_numpy(ids == audio)] = composed[1].to(torch.bfloat16)
    _check_dest(dst, rows, np.arange(n_tok), 4096, f"inputs_embeds {table}", n_rows=n_tok)


@pytest.mark.parametrize("eng,proj", [(1, 3), (0, 4), (2, 3)], ids=["no-opt-in", "reference-projector", "reference-engine"])
def test_contract_mismatch_is_refused(pair, batch13, eng, proj):
    import q2a
    (pcm, stride, ns), lens, want = batch13
    dst = _sentinel(sum(want), 4096, torch.bfloat16)
    with pytest.raises(q2a.Q2AError) as ei:
        pair[eng].audio_features_device_to(pcm.data_ptr(), stride, ns, q2a.feat_dst(dst.data_ptr(), 4096, sum(want), q2a.DT_BF16),
                                           pair[proj], key_len=lens)
    torch.cuda.synchronize()
    assert ei.value.rc == ERR_UNSUPPORTED and bool((_ibits(dst) == S16).all())
