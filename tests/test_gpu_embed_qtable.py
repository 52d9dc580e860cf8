"""The quantized embedding table of the inputs_embeds calls (q2a_embed_qtable): the decoding gather alone, the whole call
against the dense-table call, and the argument checks. Every comparison is exact, on integer views: the expected values
are float32(the float64 formula) of tests/embed_q_cases.py cast to the destination's dtype by torch on the CPU. The
destinations, the engine and the projector are tests/test_gpu_inputs_embeds.py's. All tests need an MI355X."""
import numpy as np
import pytest

import embed_q_cases as qc
from test_gpu_inputs_embeds import (AUDIO, D_OUT, DTYPES, FILL, GUARD, KEY_LENS, LD, N_FEAT, N_SEQ, N_TOK, OUT_LENS, S16, SEQ,
                                    _assert_same, _dt, _ibits, _layout_ids, _mel_call, _sentinel, _want_buffer, engines, mel4,
                                    projectors)   # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ERR_ARG = -4


def _qtable(t, n_cols):
    """(QuantTable on the device, its values float32 [vocab][n_cols]) of the CPU test's rows."""
    import q2a
    return q2a.QuantTable.from_host(qc.rows(t, n_cols), t, n_cols), torch.from_numpy(qc.values(t, n_cols).copy())


# ---------------------------------------------------------------- 1. the gather alone
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("name", list(qc.TYPES))
def test_gather_alone(name, dt):
    import q2a
    t, dtype = qc.TYPES[name], DTYPES[dt]
    n, guard, audio = 1237, 3, 7   # the audio id lies inside the table's range: its row must still not be stored
    for n_cols, width in ((256, 4), (512, 8), (4096, 4), (4096, 8)):
        qt, vals = _qtable(t, n_cols)
        assert qt.row_bytes % 16 == 0 and (t != qc.Q6_K or n_cols == 4096 or qt.row_bytes > q2a.quant_row_size(t, n_cols))
        vocab, ld = qt.vocab, n_cols + 64
        rng = np.random.default_rng(n_cols + width)
        ids = rng.integers(0, vocab, size=n).astype(np.int32 if width == 4 else np.int64)
        ids[rng.random(n) < 0.2] = audio
        ids[20:38] = [0, vocab - 1] + list(range(vocab - 16, vocab))   # every end-code row is gathered
        bad_at = [0, 5, 64, 700, n - 1]
        ids[bad_at] = [-1, vocab, vocab + 1000, np.iinfo(ids.dtype).min, np.iinfo(ids.dtype).max]
        if width == 8:
            ids[9] = 3 + (1 << 32)     # a valid low word under a high word: outside the table
            bad_at = bad_at + [9]
        dst = _sentinel(guard + n + guard, ld, dtype)
        report = torch.full((4,), FILL, dtype=torch.int32, device="cuda")
        ids_dev = torch.from_numpy(ids).cuda()
        src = q2a.embeds_src(ids_dev.data_ptr(), width, n, audio, report_ptr=report.data_ptr())
        q2a.test_embed_gather_q(src, qt, q2a.feat_dst(dst[guard:].data_ptr(), ld, n, _dt(dt)), n_cols)
        torch.cuda.synchronize()
        text = np.flatnonzero((ids != audio) & (ids >= 0) & (ids < vocab))
        assert len(text) + len(bad_at) + int((ids == audio).sum()) == n
        want = _want_buffer(dst, [(guard + text, vals[torch.from_numpy(ids[text].astype(np.int64))].to(dtype))])
        _assert_same(dst, want, f"gather {name} {dt} n_cols {n_cols} width {width}")
        assert report.cpu().tolist() == [0, 0, len(bad_at), 2]


# ---------------------------------------------------------------- 2. the whole call
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["q4_k", "q6_k"])
def test_whole_call_equals_the_dense_table_call(engines, projectors, mel4, name, dt):
    import q2a
    e, pr, dtype = engines("q4_k"), projectors("q4_k"), DTYPES[dt]
    qt, vals = _qtable(qc.TYPES[name], D_OUT)
    dense = vals.to(dtype).cuda()
    ids = _layout_ids() % np.int64(qt.vocab)
    ids[_layout_ids() == AUDIO] = AUDIO
    ids_dev = torch.from_numpy(ids).cuda()
    outs = []
    for quant in (False, True):
        dst = _sentinel(N_TOK + GUARD, LD, dtype)
        report = torch.full((4,), FILL, dtype=torch.int32, device="cuda")
        fd = q2a.feat_dst(dst.data_ptr(), LD, N_TOK, _dt(dt))
        if quant:
            src = q2a.embeds_src(ids_dev.data_ptr(), 8, N_TOK, AUDIO, report_ptr=report.data_ptr())
            x = mel4[0]
            ol, st = e.inputs_embeds_device_mel_q(x.data_ptr(), x.shape[1] * x.shape[2], x.shape[2], [x.shape[2]] * x.shape[0], fd, src,
                                                  qt, pr, key_len=KEY_LENS)
        else:
            src = q2a.embeds_src(ids_dev.data_ptr(), 8, N_TOK, AUDIO, dense.data_ptr(), qt.vocab, D_OUT, report.data_ptr())
            ol, st = _mel_call(e, pr, mel4, fd, src)
        torch.cuda.synchronize()
        assert list(ol) == OUT_LENS and list(st) == [q2a.CLIP_ENCODED] * 4 and report.cpu().tolist() == [N_FEAT, N_FEAT, 0, 0]
        outs.append(_ibits(dst.cpu()))
    assert torch.equal(outs[0], outs[1]) and bool((outs[1][:N_TOK, :D_OUT] != (S16 if dt == "bf16" else 0x5A5A5A5A)).any(1).all())
    mine = _sentinel(N_TOK, D_OUT, dtype).view(N_SEQ, SEQ, D_OUT)
    out, ol, rep = e.inputs_embeds(mel4[0], mel4[1], ids_dev.view(N_SEQ, SEQ), AUDIO, pr, embed_table=qt, out=mine)
    torch.cuda.synchronize()
    assert out is mine and list(ol) == OUT_LENS and rep.cpu().tolist() == [N_FEAT, N_FEAT, 0, 0]
    assert torch.equal(_ibits(mine.cpu().view(N_TOK, D_OUT)), outs[1][:N_TOK, :D_OUT])


# ---------------------------------------------------------------- 3. arguments: nothing is launched or written
def test_arguments():
    import q2a
    qt, _ = _qtable(qc.Q6_K, 256)                     # rows of 210 bytes at a stride of 224
    n = 64
    ids_dev = torch.zeros(n, dtype=torch.int64, device="cuda")
    dense = torch.zeros((8, 256), dtype=torch.bfloat16, device="cuda")
    dst = _sentinel(n, 512, torch.bfloat16)
    report = torch.full((4,), FILL, dtype=torch.int32, device="cuda")
    good = dict(rows=qt.rows.data_ptr(), ggml_type=qc.Q6_K, reserved=0, vocab=qt.vocab, n_cols=256, row_bytes=qt.row_bytes)
    cases = {
        "an unknown type": dict(q=dict(ggml_type=1)),
        "Q8_K is not a table type": dict(q=dict(ggml_type=15)),
        "n_cols % 256 != 0": dict(q=dict(n_cols=384), d_out=384),
        "n_cols != d_out": dict(q=dict(n_cols=512, row_bytes=448), d_out=256),
        "a short row_bytes": dict(q=dict(row_bytes=208)),
        "a misaligned row_bytes": dict(q=dict(row_bytes=216)),
        "a misaligned base": dict(q=dict(rows=qt.rows.data_ptr() + 8)),
        "no rows": dict(q=dict(rows=0)),
        "vocab 0": dict(q=dict(vocab=0)),
        "reserved set": dict(q=dict(reserved=1)),
        "a dense table beside the quantized one": dict(table_ptr=dense.data_ptr(), vocab=8, table_ld=256),
        "no quantized table": dict(no_qt=True),
    }
    for why, kw in cases.items():
        q = dict(good, **kw.get("q", {}))
        desc = None if kw.get("no_qt") else q2a.EmbedQTable(q["rows"] or None, q["ggml_type"], q["reserved"], q["vocab"], q["n_cols"],
                                                             q["row_bytes"])
        src = q2a.embeds_src(ids_dev.data_ptr(), 8, n, AUDIO, kw.get("table_ptr", 0), kw.get("vocab", 0), kw.get("table_ld", 0),
                             report.data_ptr())
        with pytest.raises(q2a.Q2AError) as ei:
            q2a.test_embed_gather_q(src, desc, q2a.feat_dst(dst.data_ptr(), 512, n, q2a.DT_BF16), kw.get("d_out", 256))
        assert ei.value.rc == ERR_ARG, why
        torch.cuda.synchronize()
        assert bool((_ibits(dst) == S16).all() and (report == FILL).all()), why
    # and the call itself works with these buffers
    src = q2a.embeds_src(ids_dev.data_ptr(), 8, n, AUDIO, report_ptr=report.data_ptr())
    q2a.test_embed_gather_q(src, q2a.EmbedQTable(**good), q2a.feat_dst(dst.data_ptr(), 512, n, q2a.DT_BF16), 256)
    torch.cuda.synchronize()
    assert report.cpu().tolist() == [0, 0, 0, 0] and not bool((_ibits(dst[:, :256]) == S16).all())
