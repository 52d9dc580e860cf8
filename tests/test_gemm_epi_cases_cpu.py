"""The epilogue rules and checkers of tests/gemm_epi_cases.py, proven on the CPU before any GPU sees them: the rules
reproduce the oracle's own layer-0 intermediates from the oracle's own accumulators, and the checkers reject every
planted epilogue fault (tests/test_gpu_gemm_epilogues.py relies on exactly these checkers)."""
import numpy as np
import pytest

import gemm_epi_cases as gc
import operand_cases as oc
import oracle_py
from q2a import ggmlfile

S16, S32 = oc.SENTINEL16, oc.SENTINEL32
PAD = 16


@pytest.fixture(scope="module", autouse=True)
def _oracle(host_build):
    return True


def _f32(mf, name):
    return mf.t(name).as_f32().reshape(-1).astype(np.float32)


def _raw(mf, name):
    return np.ascontiguousarray(mf.t(name).data)


# --------------------------------------------------------------------------------- 1. the rules against the oracle
@pytest.mark.parametrize("wt", ["f16", "q4_k"])
def test_rules_reproduce_the_oracles_layer0_intermediates(make_model, make_clip, wt):
    """oracle_encode's dumps of layer 0 — Q, K, V (split hi / lo), x1 and the GELU output — equal the rules applied to
    oracle_gemm's accumulators of the dumped operands. The oracle scales Q by 1/sqrt(dh) only and carries x >= 10
    through its GELU as f32 (the tiny model has no such pre-activation: asserted)."""
    mf = ggmlfile.read(make_model("tiny", wt))
    o = oracle_py.Oracle(mf)
    _, d = o.encode(o.mel_window(o.log_mel(make_clip(0))), dump=True)
    D, H = mf.hparams["n_audio_state"], mf.hparams["n_audio_head"]
    p = "layers.0."
    w = np.concatenate([_raw(mf, p + f"self_attn.{n}_proj.weight") for n in "qkv"])
    bias = np.concatenate([_f32(mf, p + "self_attn.q_proj.bias"), np.zeros(D, np.float32), _f32(mf, p + "self_attn.v_proj.bias")])
    acc = oracle_py.gemm(mf.wtype, w, d["ln1"], 3 * D)
    qs = gc.qscale(D // H, bf16=True)          # 1/sqrt(dh) alone: the oracle's (and the bf16 contract's) scale
    want = gc.rule_qkv(acc, bias, D, qs)
    for name, dump in (("q", d["q"]), ("k", d["k"]), ("v", d["v"])):
        hi = dump.astype(np.float16)
        lo = (dump - hi.astype(np.float32)).astype(np.float16)
        gc.assert_same(hi.view(np.uint16), want[name + "h"], f"{wt} {name} hi")
        gc.assert_same(lo.view(np.uint16), want[name + "l"], f"{wt} {name} lo")
    assert (want["ql"] != 0).mean() > 0.9                          # the lo image carries something
    acc_o = oracle_py.gemm(mf.wtype, _raw(mf, p + "self_attn.out_proj.weight"), d["attn"], D)
    gc.assert_same(gc.rule_resid(acc_o, _f32(mf, p + "self_attn.out_proj.bias"), d["conv_out"]), d["x1"], f"{wt} x1")
    ln2 = oc.ln_ref(d["x1"], _f32(mf, p + "final_layer_norm.weight"), _f32(mf, p + "final_layer_norm.bias"))
    acc1 = oracle_py.gemm(mf.wtype, _raw(mf, p + "fc1.weight"), ln2, 4 * D)
    assert np.abs(d["gelu"]).max() < 10
    g = gc.rule_gelu_h(acc1, _f32(mf, p + "fc1.bias"))
    # (+0 and -0 aside: the oracle returns the table's -0 as an f32 -0 too, so even the signs of zero agree)
    gc.assert_same(g, d["gelu"].astype(np.float16).view(np.uint16), f"{wt} GELU")
    assert np.array_equal(g.view(np.float16).astype(np.float32), d["gelu"])      # the table's values are fp16 exactly
    pre = gc.rule_pre_h(acc1, _f32(mf, p + "fc1.bias"))
    assert np.array_equal(oc.gelu_ref(pre), d["gelu"])                        # PRE_H + the GELU quantizer's lookup


def test_gelu_rule_branches():
    v = np.array([[-30.0, -10.0, -9.99, -0.0, 0.0, 1.0, 9.99, 9.999, 10.0, 10.004, 37.123, 70000.0]], np.float32)
    b = gc.gelu_h_bits(v)[0]
    f = b.view(np.float16).astype(np.float32)
    assert b[0] == 0 and b[1] == 0                                 # v <= -10: +0
    assert f[5] == oc.gelu_values()[np.float16(1.0).view(np.uint16)]
    assert f[7] == 10.0 and f[8] == 10.0                           # 9.999 rounds to fp16 10: the table's 10
    assert f[9] == np.float32(np.float16(10.004)) and f[10] == np.float32(np.float16(37.123)) != v[0, 10]   # fp16 carry
    assert np.isinf(f[11])
    assert gc.gelu_h_bits(np.array([[-9.999]], np.float32))[0, 0] == 0x8000   # rounds to fp16 -10: the table's -0
    assert b[2] == 0x8000                                          # so does every table entry down there


# ---------------------------------------------------------------------------------- 2. planted faults are rejected
M, D, F = 150, 128, 512
TILE = (64, 128)


def _guarded(a, fill=None):
    """a [M][W] -> [M + PAD][W] with sentinel guard rows."""
    s = S16 if a.dtype.itemsize == 2 else S32
    g = np.full((a.shape[0] + PAD, a.shape[1]), s, a.view(np.uint16 if a.dtype.itemsize == 2 else np.uint32).dtype)
    g[:a.shape[0]] = a.view(g.dtype)
    return g


@pytest.fixture(scope="module")
def qkv_case():
    rng = np.random.default_rng(1)
    acc = rng.standard_normal((M, 3 * D)).astype(np.float32) * 3
    bias = rng.standard_normal(3 * D).astype(np.float32)
    qs = gc.qscale(64)
    want = gc.rule_qkv(acc, bias, D, qs)
    bufs = [_guarded(want[n]) for n in gc.QKV_NAMES]
    gc.check_qkv(bufs, acc, bias, D, qs, M, "clean", TILE)          # the clean image passes
    return acc, bias, qs, bufs


def _reject(check, match=None):
    with pytest.raises(AssertionError, match=match):
        check()


def test_checker_rejects_qkv_faults(qkv_case):
    acc, bias, qs, clean = qkv_case
    chk = lambda bufs: gc.check_qkv(bufs, acc, bias, D, qs, M, "planted", TILE)   # noqa: E731
    cp = lambda: [b.copy() for b in clean]                                        # noqa: E731
    b = cp(); b[0], b[1] = b[1], b[0]                                 # hi and lo swapped
    _reject(lambda: chk(b), "qh")
    b = cp(); b[3][M - 7:M] = 0                                       # lo zeroed in the last 7 rows
    with pytest.raises(AssertionError) as ei:
        chk(b)
    assert "kl" in str(ei.value) and f"'row': {M - 7}" in str(ei.value) and "'n_rows': 7" in str(ei.value)
    b = cp(); b[4][64:80] = np.roll(b[4][64:80], 8, axis=0)           # one 16-row group's halves exchanged (rotated by 8)
    with pytest.raises(AssertionError) as ei:
        chk(b)
    assert "vh" in str(ei.value) and "'row': 64" in str(ei.value) and "'tile': (1, 0)" in str(ei.value)
    for part, names in ((0, (0, 1)), (2, (4, 5))):                    # bias dropped (Q, V)
        nb = bias.copy(); nb[part * D:(part + 1) * D] = 0
        w = gc.rule_qkv(acc, nb, D, qs)
        b = cp()
        for i in names:
            b[i][:M] = w[gc.QKV_NAMES[i]]
        _reject(lambda: chk(b), gc.QKV_NAMES[names[0]])
    w = gc.rule_qkv(np.concatenate([acc[:, :D], acc[:, D:2 * D] * 0 + (acc[:, D:2 * D] + bias[D:2 * D]) * qs - bias[D:2 * D],
                                    acc[:, 2 * D:]], axis=1), bias, D, qs)
    b = cp(); b[2][:M], b[3][:M] = w["kh"], w["kl"]                   # Q scale applied to K
    _reject(lambda: chk(b), "kh")
    b = cp(); b[2][M] = b[2][M - 1]                                   # row M written
    _reject(lambda: chk(b), "rows >= M")
    b = cp(); b[5][M + PAD - 1, D - 1] = 0                            # the far corner of the guard
    _reject(lambda: chk(b), "vl rows >= M")


def test_checker_rejects_v_layout_faults():
    """bf16 contract: V must be V^T [clip][head][64][TP]; a row-major V in that buffer, or a V^T image where the
    reference contract wants rows, is rejected; so is a t past the last row of the partly filled clip."""
    T, TP, Mv = 100, 128, 252
    rng = np.random.default_rng(2)
    acc = rng.standard_normal((Mv, 3 * D)).astype(np.float32)
    bias = rng.standard_normal(3 * D).astype(np.float32)
    qs = gc.qscale(64, bf16=True)
    want = gc.rule_qkv(acc, bias, D, qs, bf16=True)
    clips = 4                                                         # 2.5 clips written, a whole guard clip behind
    vt = gc.vt_image(want["v"], T, TP, S16, clips=clips)
    assert (vt[2, :, :, 52:] == S16).all() and (vt[3] == S16).all() and (vt[:2, :, :, T:] == S16).all()
    assert vt[1, 1, 5, 7] == want["v"][T + 7, 64 + 5]
    q, k = _guarded(want["q"]), _guarded(want["k"])
    chk = lambda v: gc.check_qkv_bf16([q, k, v], acc, bias, D, qs, Mv, T, TP, "planted", TILE)   # noqa: E731
    chk(vt)
    rows = np.full(vt.size, S16, np.uint16)
    rows[:Mv * D] = want["v"].reshape(-1)                             # V stored row-major where V^T belongs
    _reject(lambda: chk(rows.reshape(vt.shape)), "V\\^T")
    v2 = vt.copy(); v2[2, 0, 0, 52] = v2[2, 0, 0, 51]                  # t = 52 of the partly filled clip (row M)
    with pytest.raises(AssertionError) as ei:
        chk(v2)
    assert "'clip': 2" in str(ei.value) and "'t': 52" in str(ei.value)
    # M % 4 != 0: the epilogue's 4-t store group that holds row M - 1 is written whole (the stated deviation) — those
    # one to three t are not asserted, the next one is
    assert gc.vt_cut_group(252, T) is None and gc.vt_cut_group(250, T) == (2, 50, 52) and gc.vt_cut_group(301, T) == (3, 1, 4)
    w250 = {k: v[:250] for k, v in want.items()}
    vt250 = gc.vt_image(w250["v"], T, TP, S16, clips=clips)
    q250, k250 = _guarded(w250["q"]), _guarded(w250["k"])
    chk250 = lambda v: gc.check_qkv_bf16([q250, k250, v], acc[:250], bias, D, qs, 250, T, TP, "planted", TILE)   # noqa: E731
    chk250(vt250)
    v4 = vt250.copy(); v4[2, :, :, 50:52] = 0x1234
    chk250(v4)
    v4[2, 1, 9, 52] = 0x1234
    _reject(lambda: chk250(v4), "V\\^T")
    v3 = vt.copy(); v3[0, 1, 2, T] = 0                                # a pad column of a full clip
    _reject(lambda: chk(v3), "V\\^T")
    one = gc.vt_image(want["v"][:T], T, TP, S16)                      # one whole clip alone: the pad columns are zeros
    assert (one[0, :, :, T:] == 0).all()
    # the reverse: the reference contract's row-major V buffer handed a V^T image
    r = gc.rule_qkv(acc, bias, D, gc.qscale(64))
    bufs = [_guarded(r[n]) for n in gc.QKV_NAMES]
    t_img = gc.vt_image(r["vh"], T, TP, S16).reshape(-1)
    bufs[4] = np.resize(t_img, bufs[4].shape).copy()
    _reject(lambda: gc.check_qkv(bufs, acc, bias, D, gc.qscale(64), Mv, "planted", TILE), "vh")


def test_checker_rejects_resid_and_h_faults():
    rng = np.random.default_rng(3)
    acc = rng.standard_normal((M, D)).astype(np.float32)
    bias = rng.standard_normal(D).astype(np.float32)
    x = gc.resid_rows(M, D, 0)
    want = gc.rule_resid(acc, bias, x)
    assert (want != acc + (bias + x)).any()                           # the association is visible on these rows
    buf = _guarded(want)
    gc.check_resid(buf, acc, bias, x, M, "clean", TILE)
    for bad in (acc + (bias[None, :] + x), acc + x):                  # the other association; bias dropped
        b = buf.copy(); b[:M] = bad.astype(np.float32).view(np.uint32)
        _reject(lambda: gc.check_resid(b, acc, bias, x, M, "planted", TILE), "residual")
    b = buf.copy(); b[M, 3] = b[M - 1, 3]                             # row M written
    _reject(lambda: gc.check_resid(b, acc, bias, x, M, "planted", TILE), "rows >= M")
    b = buf.copy(); b[16:32] = np.roll(b[16:32], 8, axis=0)
    _reject(lambda: gc.check_resid(b, acc, bias, x, M, "planted", TILE), "'row': 16")

    acc = rng.standard_normal((M, F)).astype(np.float32) * 4
    acc[:, 7] += 20; acc[:, 9] -= 20                                  # both range branches
    bias = rng.standard_normal(F).astype(np.float32)
    for gelu in (False, True):
        want = gc.rule_gelu_h(acc, bias) if gelu else gc.rule_pre_h(acc, bias)
        buf = _guarded(want)
        gc.check_h(buf, acc, bias, M, gelu, what="clean", tile=TILE)
        b = buf.copy(); b[:M] = gc.rule_gelu_h(acc, 0 * bias) if gelu else gc.rule_pre_h(acc, 0 * bias)
        _reject(lambda: gc.check_h(b, acc, bias, M, gelu, what="planted", tile=TILE))
        b = buf.copy(); b[M] = b[0]
        _reject(lambda: gc.check_h(b, acc, bias, M, gelu, what="planted", tile=TILE), "rows >= M")
    # GELU stored where the pre-activation belongs, and the reverse
    _reject(lambda: gc.check_h(_guarded(gc.rule_gelu_h(acc, bias)), acc, bias, M, False, what="planted", tile=TILE))
    _reject(lambda: gc.check_h(_guarded(gc.rule_pre_h(acc, bias)), acc, bias, M, True, what="planted", tile=TILE))
    # F32 files: the copy at column 2F
    dup = _guarded(gc.rule_gelu_h(acc, bias, o_dup=True))
    gc.check_h(dup, acc, bias, M, True, o_dup=True, what="clean", tile=TILE)
    b = dup.copy(); b[:M, 2 * F:] = S16                               # the o_dup copy missing
    _reject(lambda: gc.check_h(b, acc, bias, M, True, o_dup=True, what="planted", tile=TILE), f"'col': {2 * F}")
    b = dup.copy(); b[:M, F:2 * F] = b[:M, :F]                        # the copy one third too early
    _reject(lambda: gc.check_h(b, acc, bias, M, True, o_dup=True, what="planted", tile=TILE), f"'col': {F}")


def _q8k_buffers(y, ld):
    """The engine's layout of the oracle's Q8_K of y: codes [M + PAD][F], d [nb][ld], aext [nb][ld][16]."""
    qs, d, bs32 = oc.ref_q8k(y)
    Mq, K = y.shape
    nb = K // 256
    codes = _guarded(qs.astype(np.float16).view(np.uint16))
    dd = np.full((nb, ld), S32, np.uint32)
    dd[:, :Mq] = d.T.view(np.uint32) if d.T.flags["C_CONTIGUOUS"] else np.ascontiguousarray(d.T).view(np.uint32)
    hi = np.where(bs32 >= 0, bs32 >> 6, -((-bs32 + 63) >> 6))
    pairs = np.stack([hi, bs32 - 64 * hi], axis=-1).reshape(Mq, nb, 16).astype(np.float16)
    ae = np.full((nb, ld, 16), S16, np.uint16)
    ae[:, :Mq] = pairs.transpose(1, 0, 2).view(np.uint16)
    return codes, dd, ae


def test_checker_rejects_q8k_faults():
    rng = np.random.default_rng(4)
    acc = rng.standard_normal((M, F)).astype(np.float32) * 3
    bias = rng.standard_normal(F).astype(np.float32)
    y = gc.gelu_h_values(acc, bias)
    ld = 256
    codes, d, ae = _q8k_buffers(y, ld)
    gc.check_gelu_q8k(codes, d, ae, acc, bias, M, "clean")
    d2 = d.copy(); d2[1, 77] += 1                                     # one Q8_K d off by an ulp
    _reject(lambda: gc.check_gelu_q8k(codes, d2, ae, acc, bias, M, "planted"), "d differs")
    d3 = d.copy(); d3[0, M] = d3[0, M - 1]                            # d of row M written
    _reject(lambda: gc.check_gelu_q8k(codes, d3, ae, acc, bias, M, "planted"), "d rows >= M")
    a2 = ae.copy(); a2[1, M] = a2[1, 0]
    _reject(lambda: gc.check_gelu_q8k(codes, d, a2, acc, bias, M, "planted"), "block sums rows >= M")
    c2 = codes.copy(); c2[3, 300] ^= 0x8000                           # one code's sign
    _reject(lambda: gc.check_gelu_q8k(c2, d, ae, acc, bias, M, "planted"))
    # the codes of ggml's own GELU (f32 carry above 10) are not the fp16-carry rule's
    acc_hi = acc.copy(); acc_hi[:, 5] = 30.0 + rng.uniform(0, 1, M).astype(np.float32)
    y_f32 = np.where(acc_hi + bias >= 10, acc_hi + bias, gc.gelu_h_values(acc_hi, bias)).astype(np.float32)
    assert (y_f32 != gc.gelu_h_values(acc_hi, bias)).any()
    c3, d4, a3 = _q8k_buffers(y_f32, ld)
    _reject(lambda: gc.check_gelu_q8k(c3, d4, a3, acc_hi, bias, M, "planted"))


# ------------------------------------------------------------------------------------------- 3. the helpers themselves
def test_first_mismatch_names_the_tile_and_the_wave_row():
    a = np.zeros((600, 512), np.uint16)
    b = a.copy()
    assert gc.first_mismatch(a, b) is None
    b[300:, 260] = 1
    m = gc.first_mismatch(a, b)
    assert (m["row"], m["col"], m["tile"], m["wave_row"], m["group16"], m["row_in_group"]) == (300, 260, (1, 1), 0, 2, 12)
    assert m["n_elements"] == 300 and m["n_rows"] == 300 and m["last_row"] == 599
    f = np.zeros((4, 4), np.float32)
    g = f.copy(); g[1, 1] = -0.0                                      # bit comparison: -0 is not +0
    assert gc.first_mismatch(f, g)["want"] == "0x80000000"


@pytest.mark.parametrize("M_,tile,extra", [(1, 64, ()), (65, 64, ()), (1500, 128, ()), (43777, 256, ()), (130817, 256, ()),
                                          (26241, 256, (26112, 26240))])
def test_sample_rows_hold_the_ends_and_the_seams(M_, tile, extra):
    r = gc.sample_rows(M_, tile, extra)
    assert len(r) <= 384 and r[0] == 0 and r[-1] == M_ - 1 and len(np.unique(r)) == len(r)
    s = set(r.tolist())
    for e in extra:
        assert e - 1 in s and e in s
    seams = np.arange(tile, M_, tile)
    held = [x for x in seams if x in s and x - 1 in s]
    assert len(held) == len(seams) or len(held) >= 150                # every seam while they fit into 384 rows
    if len(seams):
        assert seams[0] in held and seams[-1] in held
