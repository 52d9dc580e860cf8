"""Every fused epilogue of the weight GEMM, element by element, in every tile regime the launcher can pick: one block
GEMM run through q2a_test_gemm_epi (run_block's own argument helpers, the kernel storing straight into sentinel-filled
caller buffers with 256 guard rows) and compared bit for bit with the numpy rule of tests/gemm_epi_cases.py applied to
the raw accumulators q2a_test_linear returns for the same rows — which holds because every tile regime sums K in the
same order. Per case:
  a. q2a_test_gemm_regime names the regime the case was built for (a failure, never a skip)
  b. the exact rule on every element
  c. the accumulators themselves against the float64 oracle on <= 384 sampled rows (row 0, row M-1, tile-row seams,
     the main / tail seam), at the one-linear bars of tests/test_gpu_parity.py (1e-5 max-rel, 1e-6 rel-L2; the F32
     files' own 2e-6 rel-L2 of tests/test_gpu_f32_models.py)
  d. planted all-zero input rows give rule(bias alone) — a check that uses no other GPU result
  e. nothing behind row M (for V^T: behind the last t of a partly filled clip) was written
Rules and checkers are proven on the CPU in tests/test_gemm_epi_cases_cpu.py. All tests need an MI355X."""
import numpy as np
import pytest

import gemm_epi_cases as gc
import kquant_cases as kc
import operand_cases as oc
import oracle_py
from conftest import rel_errors
from q2a import ggmlfile

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

QKV, RESID, GELU_H, GELU_Q8K, PRE_H = 0, 1, 2, 6, 7
EPI_NAME = {QKV: "QKV", RESID: "RESID", GELU_H: "GELU_H", GELU_Q8K: "GELU_Q8K", PRE_H: "PRE_H"}
NARROW, T128, T128x256, T256, PIPE8, PERSISTENT, TAIL, FIXED = range(8)
REGIME_NAME = ["narrow 64x128", "128x128", "128x256", "256x256", "8-phase", "8-phase persistent", "8-phase + 128x128 tail",
               "fixed"]
# tile (rows, columns) and rows per wave of each regime: what a mismatch report is expressed in
TILE = {NARROW: ((64, 128), 16), T128: ((128, 128), 64), T128x256: ((128, 256), 64), T256: ((256, 256), 128),
        PIPE8: ((256, 256), 128), PERSISTENT: ((256, 256), 128), TAIL: ((256, 256), 128), FIXED: ((128, 128), 64)}
GUARD = 256
BLK = {"f16": 0, "f32": 0, "q4_k": 256, "q5_k": 256, "q8_0": 32, "q6_k": 16, "bf16": 1}


# ------------------------------------------------------------------------------------------------------ engines
class Ctx:
    def __init__(self, e, path, kind):
        self.e, self.kind, self.mf = e, kind, ggmlfile.read(path)
        hp = self.mf.hparams
        self.D, self.H, self.T, self.L = hp["n_audio_state"], hp["n_audio_head"], hp["n_audio_ctx"], hp["n_audio_layer"]
        self.F = 4 * self.D
        self.TP = (self.T + 63) // 64 * 64
        self.layer = min(7, self.L - 1)
        self.kx = 3 if kind == "f32" else 1
        self._w = {}

    def nk(self, which):
        return {0: 3 * self.D, 1: self.D, 2: self.F, 3: self.D}[which], (self.F if which == 3 else self.D)

    def names(self, which):
        p = f"layers.{self.layer}."
        return [p + n for n in {0: ["self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight"],
                                1: ["self_attn.out_proj.weight"], 2: ["fc1.weight"], 3: ["fc2.weight"]}[which]]

    def bias(self, which):
        p = f"layers.{self.layer}."
        f = lambda n: self.mf.t(p + n).as_f32().reshape(-1).astype(np.float32)   # noqa: E731
        if which == 0:      # (whisper's K projection has no bias)
            return np.concatenate([f("self_attn.q_proj.bias"), np.zeros(self.D, np.float32), f("self_attn.v_proj.bias")])
        return f({1: "self_attn.out_proj.bias", 2: "fc1.bias", 3: "fc2.bias"}[which])

    def anchor(self, which, x):
        """The float64-class reference of the raw accumulators on the rows x, by the oracle of the engine's mode."""
        N, _ = self.nk(which)
        if self.kind in ("f16", "q4_k", "q8_0"):
            w = np.concatenate([np.ascontiguousarray(self.mf.t(n).data) for n in self.names(which)])
            return oracle_py.gemm(self.mf.wtype, w, x, N)
        if self.kind in ("q5_k", "q6_k"):
            return kc.kq_linear_ref(kc.matrix_tensors(self.mf, self.layer, which), x)
        if self.kind == "f32":
            w = np.concatenate([self.mf.t(n).as_f32().astype(np.float64) for n in self.names(which)])
            return x.astype(np.float64) @ w.reshape(N, -1).T
        from test_gpu_bf16_act import bf, w_bf16        # bf16 contract: bf16 x bf16 products, exact
        w = torch.cat([w_bf16(self.mf, n) for n in self.names(which)])
        return (bf(torch.from_numpy(x).cuda()).double() @ w.T).cpu().numpy()


@pytest.fixture(scope="module")
def ctxs(make_model):
    import q2a
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    cache = {}

    def get(cfg, kind):
        if (cfg, kind) not in cache:
            wt = "q8_0" if kind == "bf16" else kind
            path = make_model(cfg, wt)
            cache[(cfg, kind)] = Ctx(q2a.Engine(path, device=0, act=q2a.ACT_BF16 if kind == "bf16" else 0), path, kind)
        return cache[(cfg, kind)]

    yield get
    for c in cache.values():
        c.e.close()


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------- the launcher's formulas, restated (q2a_gemm.hip)
def cdiv(a, b):
    return -(-a // b)


def is_narrow(M, N):
    return cdiv(M, 128) * (N // 128) < 256


def is_wide(M, N):
    return cdiv(M, 256) * (N // 256) >= 512 and N % 256 == 0


def tail_split(M, N, K, cus):
    """m_main (256-row tiles of the main launch) when the 8-phase launch of a TAILABLE epilogue is cut in two, else 0."""
    nbn, nbm = N // 256, cdiv(M, 256)
    ntl = nbn * nbm
    rem = ntl % cus
    m_main = (ntl - rem) // nbn
    return m_main if K >= 4096 and 0 < rem and rem * 8 <= cus * 5 and 0 < m_main < nbm else 0


def expected_regime(kind, epi, M, N, K, D, cus):
    blk = BLK[kind]
    if blk == 16:
        return FIXED
    wide = is_wide(M, N)
    p8 = wide and ((K // 64) % 2 == 0 if blk in (0, 1) else blk == 256 and (K // 64) % 4 == 0)
    if epi == GELU_Q8K:
        return PIPE8 if p8 else T128x256
    if p8:
        ntl = (N // 256) * (M // 256)
        grid = min(ntl, cus // 8 * 8)
        if epi in (PRE_H, QKV) and blk == 256 and M % 256 == 0 and K >= 512 and 0 < ntl <= 64 * grid and cus >= 8 and \
                (epi != QKV or D % 256 == 0):
            return PERSISTENT
        if epi in (RESID, PRE_H, GELU_H) and tail_split(M, N, K, cus):
            return TAIL
        return PIPE8
    if not wide and is_narrow(M, N):
        return NARROW
    return T128 if not wide else (T256 if blk in (0, 1) else T128x256)


# ------------------------------------------------------------------------------------------------------ one case
def dev_rows(M, K, seed, scale=1.0, zero_rows=()):
    """gemm_epi_cases.input_rows made on the device: Gaussian rows, four outlier channels, a common offset, the
    planted all-zero rows."""
    g = torch.Generator(device="cuda").manual_seed(11000 + seed)
    x = torch.randn((M, K), device="cuda", generator=g)
    x[:, torch.randperm(K, device="cuda", generator=g)[:4]] *= 8.0
    x = (x + 0.25) * scale
    if len(zero_rows):
        x[torch.as_tensor(np.asarray(zero_rows), device="cuda")] = 0.0
    return x


def dev_resid(M, D, seed):
    g = torch.Generator(device="cuda").manual_seed(12000 + seed)
    x = torch.randn((M, D), device="cuda", generator=g)
    x[5 % M::97] *= 1e4
    return x


def sentinel16(*shape):
    return torch.full(shape, oc.SENTINEL16, dtype=torch.int16, device="cuda")


def host16(t):
    return t.cpu().numpy().view(np.uint16)


def launch(c, which, epi, M, x):
    """The hook on the rows x [M][K]: sentinel-filled output buffers with GUARD rows behind M (V^T: up to the padded
    clip, and a whole guard clip where none is ragged; RESID: the residual rows in place). Returns (device buffers,
    the residual rows or None)."""
    N, _ = c.nk(which)
    R = M + GUARD
    resid = None
    if epi == QKV and c.kind != "bf16":
        bufs = [sentinel16(R, c.D) for _ in range(6)]
    elif epi == QKV:
        clips = cdiv(M, c.T) + (1 if M % c.T == 0 else 0)
        bufs = [sentinel16(R, c.D), sentinel16(R, c.D), sentinel16(clips, c.H, 64, c.TP)]
    elif epi == RESID:
        resid = dev_resid(M, c.D, seed=M % 1000 + which)
        buf = torch.full((R, c.D), oc.SENTINEL32, dtype=torch.int32, device="cuda")
        buf[:M] = resid.view(torch.int32)
        bufs = [buf]
    elif epi == GELU_Q8K:
        ld = cdiv(R, 256) * 256
        bufs = [sentinel16(R, N), torch.full((N // 256, ld), oc.SENTINEL32, dtype=torch.int32, device="cuda"),
                sentinel16(N // 256, ld, 16)]
    else:
        bufs = [sentinel16(R, N * c.kx)]
    c.e.test_gemm_epi(c.layer, which, epi, x.data_ptr(), M, [b.data_ptr() for b in bufs],
                      ld=bufs[1].shape[1] if epi == GELU_Q8K else 0)
    return bufs, resid


def run_case(c, which, epi, M, expect, cus, seams=(), x_base=None):
    """One launch of GEMM `which` with epilogue `epi` at M rows on the engine of c; assertions a - e. x_base: input rows
    [>= M][K] on the device to take the first M of (cases that compare shared rows); the zero rows are planted in a
    copy. Returns (the output buffers as host arrays, the planted zero rows)."""
    e = c.e
    N, K = c.nk(which)
    what = f"{c.kind} D={c.D} {('QKV', 'O', 'fc1', 'fc2')[which]} {EPI_NAME[epi]} M={M} [{REGIME_NAME[expect]}]"
    # a. the regime, by the launcher's own decision function and by the formulas restated above
    got_regime = e.test_gemm_regime(which, epi, M)
    assert got_regime == expect, f"{what}: the launcher picks {REGIME_NAME[got_regime]}"
    assert expected_regime(c.kind, epi, M, N, K * c.kx, c.D, cus) == expect, f"{what}: the restated formulas disagree"
    (tile, wave_rows) = TILE[expect]
    tile_rows = np.arange(tile[0], M, tile[0])
    zero = gc.seam_rows(M, list(seams) + ([int(tile_rows[len(tile_rows) // 2])] if len(tile_rows) else []))
    if M < 8:
        zero = zero[:0]                # (a launch of all-zero rows has no accumulator for the oracle to confirm)
    if x_base is None:
        x = dev_rows(M, K, seed=which * 7 + M % 1000, scale=0.3 if which == 3 else 1.0, zero_rows=zero)
    else:
        x = x_base[:M].clone()
        x[torch.as_tensor(zero, device="cuda")] = 0.0
    acc_d = torch.empty((M, N), dtype=torch.float32, device="cuda")
    e.test_linear(c.layer, which, x.data_ptr(), M, acc_d.data_ptr())
    bias = c.bias(which)
    bf16 = c.kind == "bf16"
    qs = gc.qscale(c.D // c.H, bf16)
    bufs, resid = launch(c, which, epi, M, x)
    torch.cuda.synchronize()
    acc = acc_d.cpu().numpy()
    # c. the accumulators against the float64-class oracle on sampled rows
    rows = gc.sample_rows(M, tile[0], seams, seed=M)
    ref = c.anchor(which, x[torch.from_numpy(rows).cuda()].cpu().numpy())
    mx, l2 = rel_errors(acc[rows], ref)
    print(f"{what}: accumulators vs oracle on {len(rows)} rows: max-rel {mx:.3e} rel-L2 {l2:.3e}")
    assert mx < 1e-5 and l2 < (2e-6 if c.kind == "f32" else 1e-6), (what, mx, l2)
    # b + e. the exact rule on every element, the sentinel behind row M; d. zero rows from the bias alone
    zacc = np.zeros((len(zero), N), np.float32)
    if epi == QKV and not bf16:
        got = [host16(b) for b in bufs]
        gc.check_qkv(got, acc, bias, c.D, qs, M, what, tile)
        want0 = gc.rule_qkv(zacc, bias, c.D, qs)
        for name, g in zip(gc.QKV_NAMES, got):
            gc.assert_same(g[zero], want0[name], f"{what} zero rows {name}")
    elif epi == QKV:
        got = [host16(b) for b in bufs]
        gc.check_qkv_bf16(got, acc, bias, c.D, qs, M, c.T, c.TP, what, tile)
        want0 = gc.rule_qkv(zacc, bias, c.D, qs, bf16=True)
        gc.assert_same(got[0][zero], want0["q"], f"{what} zero rows q")
        gc.assert_same(got[1][zero], want0["k"], f"{what} zero rows k")
        vt = got[2]
        for i, r in enumerate(zero):
            col = vt[r // c.T, :, :, r % c.T].reshape(-1)
            assert np.array_equal(col, want0["v"][i]), f"{what} zero row {r} of V^T"
    elif epi == RESID:
        got = bufs[0].cpu().numpy().view(np.uint32)
        xr = resid.cpu().numpy()
        gc.check_resid(got, acc, bias, xr, M, what, tile)
        gc.assert_same(got[zero], gc.rule_resid(zacc, bias, xr[zero]), f"{what} zero rows")
    elif epi == GELU_Q8K:
        codes, d, ae = host16(bufs[0]), bufs[1].cpu().numpy().view(np.uint32), host16(bufs[2])
        gc.check_gelu_q8k(codes, d, ae, acc, bias, M, what)
        got = [codes, d, ae]
        dec = gc.decode_q8k(codes, d, ae, M)
        oc.check_q8k({k: v[zero] for k, v in dec.items()}, gc.gelu_h_values(zacc, bias), f"{what} zero rows")
    else:
        got = host16(bufs[0])
        gelu = epi == GELU_H
        gc.check_h(got, acc, bias, M, gelu, o_dup=c.kind == "f32", what=what, tile=tile)
        want0 = gc.rule_gelu_h(zacc, bias, o_dup=c.kind == "f32") if gelu else gc.rule_pre_h(zacc, bias)
        gc.assert_same(got[zero], want0, f"{what} zero rows")
        if gelu:
            v = acc + bias
            print(f"{what}: {int((v >= 10).sum())} pre-activations >= 10, {int((v <= -10).sum())} <= -10")
    return (got if isinstance(got, list) else [got]), zero


# ---------------------------------------------------------------------------------------------------- the cases
# (which, epilogue) pairs the block launches per engine kind (fc1: under some q2a_test_fc1_path)
LAUNCHES = {"f16": [(0, QKV), (1, RESID), (2, GELU_H), (3, RESID)],
            "f32": [(0, QKV), (1, RESID), (2, GELU_H), (3, RESID)],
            "q8_0": [(0, QKV), (1, RESID), (2, GELU_H), (3, RESID)],
            "q4_k": [(0, QKV), (1, RESID), (2, PRE_H), (2, GELU_H), (3, RESID)],
            "q6_k": [(0, QKV), (1, RESID), (2, PRE_H), (2, GELU_H), (3, RESID)]}
SMALL_M = [1, 63, 64, 65, 1500]
SMALL = [(k, w, ep) for k, l in LAUNCHES.items() for w, ep in l]


def _id(v):
    return EPI_NAME.get(v, str(v)) if isinstance(v, int) else str(v)


@pytest.mark.parametrize("kind,which,epi", SMALL, ids=[f"{k}-{('qkv', 'o', 'fc1', 'fc2')[w]}-{EPI_NAME[ep]}" for k, w, ep in SMALL])
def test_small_tiles(ctxs, cus, kind, which, epi):
    """One clip or less: the narrow 64x128 tiles (8 waves, 16 rows each) at M = 1, 63, 64, 65 (one tile, its last row,
    the first row of the second) and 1500; Q6_K on its one 128x128 configuration."""
    c = ctxs("tiny", kind)
    for M in SMALL_M:
        run_case(c, which, epi, M, FIXED if kind == "q6_k" else NARROW, cus, seams=[64] if M > 64 else [])


@pytest.mark.parametrize("kind", ["f16", "q4_k", "q8_0", "f32", "q6_k"])
def test_qkv_narrow_to_128_switch(ctxs, cus, kind):
    """Tiny QKV (N = 768): ceil(M / 128) * 6 reaches 256 at M = 5377 — 5376 is the last narrow launch, 5377 the first
    on 128x128 tiles (one row in its last tile), 5505 one more ragged 128-row tile (row 5504 alone)."""
    c = ctxs("tiny", kind)
    for M, rg in ((5376, NARROW), (5377, T128), (5505, T128)):
        run_case(c, 0, QKV, M, FIXED if kind == "q6_k" else rg, cus, seams=[5376] if M > 5376 else [])


WIDE = [(2, m) for m in (32513, 32768, 32769)] + [(0, m) for m in (43521, 43776, 43777)] + [(1, 130817), (3, 130817)]


@pytest.mark.parametrize("which,M", WIDE, ids=[f"{('qkv', 'o', 'fc1', 'fc2')[w]}-{m}" for w, m in WIDE])
@pytest.mark.parametrize("kind", ["f16", "q4_k", "q8_0"])
def test_wide_tiles_tiny(ctxs, cus, kind, which, M):
    """The first wide launches of the tiny model (ceil(M / 256) * (N / 256) >= 512): one row, all rows and one row more
    than all rows of the last 256-row tile. F16 and Q4_K: the 8-phase kernel (K = 256 or 1024: no tail, no persistent
    kernel); Q8_0: 128x256 tiles. Q4_K fc1 runs all three of its epilogues, the fused GELU + Q8_K one included."""
    c = ctxs("tiny", kind)
    rg = T128x256 if kind == "q8_0" else PIPE8
    last = (M - 1) // 256 * 256
    if which == 2 and kind == "q4_k":
        for epi in (PRE_H, GELU_H, GELU_Q8K):
            run_case(c, which, epi, M, rg, cus, seams=[last])
    else:
        run_case(c, which, dict(LAUNCHES[kind])[which], M, rg, cus, seams=[last])


@pytest.mark.parametrize("M", [43521, 43777])
def test_wide_qkv_bf16_transposed_v(ctxs, cus, M):
    """bf16 activation contract: Q, K as bf16 rows and V through the LDS-staged transposing epilogue into V^T
    [clip][head][64][TP], the last clip cut mid-way (43 521 = 29 clips + 21 rows; 43 777 = 29 clips + 277 rows): every
    pad column t >= T and the rows behind M of Q and K still hold the sentinel, and so does every t behind the last
    row but one group: both M are 1 mod 4, and the epilogue stores t in groups of four, so t = 21 .. 23 (277 .. 279) of
    clip 29 are written (found by this test; the stated deviation of DESIGN.md §2, gemm_epi_cases.vt_cut_group) —
    the sentinel is asserted from t = 24 (280) on."""
    run_case(ctxs("tiny", "bf16"), 0, QKV, M, PIPE8, cus, seams=[(M - 1) // 256 * 256, 29 * 1500])


def test_small_bf16_transposed_v(ctxs, cus):
    """The same epilogue on the small tiles: part of a clip, one whole clip alone (its pad columns are written as
    zeros), one clip and one row."""
    c = ctxs("tiny", "bf16")
    for M in (65, 1500, 1501):
        run_case(c, 0, QKV, M, NARROW, cus, seams=[64] + ([1500] if M > 1500 else []))


# -- full size: the persistent kernel, its neighbours, the two-launch tail ------------------------------------------
def persistent_rows(N, cus, first_wide_rows):
    """The smallest wide tile-row count whose tiles do not divide evenly over the persistent grid (uneven lists)."""
    grid = cus // 8 * 8
    for nr in range(first_wide_rows, first_wide_rows + 64):
        ntl = nr * (N // 256)
        if ntl % min(ntl, grid) != 0 and ntl <= 64 * min(ntl, grid):
            return nr
    raise AssertionError("no uneven persistent tile count near the wide threshold on this device")


@pytest.mark.parametrize("side", ["at", "below", "above", "under_wide"])
@pytest.mark.parametrize("kind", ["q4_k", "q5_k", "f16"])
@pytest.mark.parametrize("which", [0, 2], ids=["qkv", "fc1"])
def test_persistent_kernel_and_its_neighbours(ctxs, cus, kind, which, side):
    """Full size (K = 1280): M0 a multiple of 256 on the persistent 8-phase kernel (Q4_K / Q5_K QKV and fc1 PRE_H; 256
    CUs: QKV M0 = 8 960 = 35 x 15 = 525 tiles, fc1 M0 = 6 656 = 520 tiles, lists of two and three tiles) — "at"; its
    neighbours M0 - 1 and M0 + 1 on the plain 8-phase grid — "below", "above": exact by the rule, and every row they
    share with a second launch at M0 on the same input rows identical to it; the last row count under the wide
    threshold (fc1: 6 400) on 128x128 tiles — "under_wide". Full-size F16 takes the same M on its 8-phase kernels."""
    c = ctxs("full", kind)
    N, K = c.nk(which)
    epi = QKV if which == 0 else (GELU_H if kind == "f16" else PRE_H)
    first = cdiv(512, N // 256)
    M0 = 256 * persistent_rows(N, cus, first)
    at = PERSISTENT if kind != "f16" else PIPE8
    if side == "under_wide":
        Mb = 256 * (first - 1)
        run_case(c, which, epi, Mb, T128, cus, seams=[Mb - 128])
    elif side == "at":
        run_case(c, which, epi, M0, at, cus, seams=[M0 - 256])
    else:
        M = M0 - 1 if side == "below" else M0 + 1
        x_base = dev_rows(M0 + 1, K, seed=which)
        got, zero = run_case(c, which, epi, M, PIPE8, cus, seams=[M0 - 256, M0], x_base=x_base)
        assert c.e.test_gemm_regime(which, epi, M0) == at
        x0 = x_base[:M0].clone()
        x0[torch.as_tensor(zero[zero < M0], device="cuda")] = 0.0
        bufs, _ = launch(c, which, epi, M0, x0)
        torch.cuda.synchronize()
        n = min(M, M0)
        for i, (a, b) in enumerate(zip(got, bufs)):
            gc.assert_same(a[:n], host16(b)[:n], f"{kind} {EPI_NAME[epi]} buffer {i}: rows shared by M = {M} and M0 = {M0}")


@pytest.mark.parametrize("side", ["at_cap", "over_cap"])
def test_persistent_tile_list_cap(ctxs, cus, side):
    """The persistent kernel's tile list holds 64 entries per workgroup: full-size Q4_K fc1 PRE_H (20 tile columns) at
    the last M that fits (256 CUs: 819 tile rows = 16 380 tiles <= 64 x 256, every list full or one short) stays
    persistent; one tile row more (16 400 tiles) falls back to the plain 8-phase grid. The one heavy case (about 12 GB
    of device memory): the rule fp16(acc + bias) is evaluated and compared on the device in row chunks, and only a
    differing chunk is brought to the host for the mismatch report."""
    c = ctxs("full", "q4_k")
    N, K = c.nk(2)
    rows_cap = 64 * (cus // 8 * 8) // (N // 256)
    M = 256 * (rows_cap if side == "at_cap" else rows_cap + 1)
    expect = PERSISTENT if side == "at_cap" else PIPE8
    what = f"q4_k fc1 PRE_H M={M} [{REGIME_NAME[expect]}]"
    assert c.e.test_gemm_regime(2, PRE_H, M) == expect, what
    assert expected_regime("q4_k", PRE_H, M, N, K, c.D, cus) == expect, what
    zero = gc.seam_rows(M, [256, 256 * (rows_cap // 2), M - 256])
    x = dev_rows(M, K, seed=5, zero_rows=zero)
    acc_d = torch.empty((M, N), dtype=torch.float32, device="cuda")
    c.e.test_linear(c.layer, 2, x.data_ptr(), M, acc_d.data_ptr())
    (out,), _ = launch(c, 2, PRE_H, M, x)
    torch.cuda.synchronize()
    bias = c.bias(2)
    bias_d = torch.from_numpy(bias).cuda()
    for r0 in range(0, M, 32768):
        r1 = min(r0 + 32768, M)
        want = (acc_d[r0:r1] + bias_d).to(torch.float16).view(torch.int16)       # rule_pre_h, RNE like numpy's cast
        if not torch.equal(out[r0:r1], want):
            bad = gc.first_mismatch(host16(out[r0:r1]), gc.rule_pre_h(acc_d[r0:r1].cpu().numpy(), bias))
            bad["row"] += r0
            raise AssertionError(f"{what}: {bad}")
    assert bool((out[M:] == oc.SENTINEL16).all()), f"{what}: rows >= M were written"
    rows = gc.sample_rows(M, 256, [256 * (rows_cap // 2)], seed=M)
    ri = torch.from_numpy(rows).cuda()
    mx, l2 = rel_errors(acc_d[ri].cpu().numpy(), c.anchor(2, x[ri].cpu().numpy()))
    print(f"{what}: accumulators vs oracle on {len(rows)} rows: max-rel {mx:.3e} rel-L2 {l2:.3e}")
    assert mx < 1e-5 and l2 < 1e-6, (what, mx, l2)
    zi = torch.from_numpy(zero).cuda()
    gc.assert_same(host16(out[zi]), gc.rule_pre_h(np.zeros((len(zero), N), np.float32), bias), f"{what} zero rows")


@pytest.mark.parametrize("kind", ["q4_k", "f16"])
def test_partial_round_tail(ctxs, cus, kind):
    """Full-size fc2 (K = 5120, N = 1280: five tile columns), RESID in place. With 256 CUs: M = 26 112 + 129 is 103
    tile rows = 515 tiles, rem = 3: the main launch runs 102 tile rows on the 8-phase kernel, the tail 129 rows — one
    full and one 1-row 128x128 tile — behind the seam at row 26 112. 135 tile rows leave rem = 163 > 5/8 of the CUs:
    one launch. The O projection (K = 1280) never splits."""
    c = ctxs("full", kind)
    N, K = c.nk(3)
    nbm = next(n for n in range(103, 400) if tail_split(n * 256, N, K, cus) == n - 1)
    M = (nbm - 1) * 256 + 129
    assert tail_split(M, N, K, cus) == nbm - 1
    run_case(c, 3, RESID, M, TAIL, cus, seams=[(nbm - 1) * 256, (nbm - 1) * 256 + 128])
    nb1 = next(n for n in range(103, 400) if (n * 5) % cus * 8 > cus * 5)
    M1 = nb1 * 256 - 60
    run_case(c, 3, RESID, M1, PIPE8, cus, seams=[(nb1 - 1) * 256])
    run_case(c, 1, RESID, 26200, PIPE8, cus, seams=[26112])


# ---------------------------------------------------------------------------------------- coverage and arguments
def test_every_regime_of_the_loaded_weight_types_is_hit(ctxs, cus):
    """The launcher's answers for the cases above cover every regime it can return for these files: all but the plain
    256x256 tiles (fp16 / bf16 weights with an odd number of 64-deep K-steps: D = 256 and 1280 give 4 and 20)."""
    hit = set()
    for kind, which, epi in SMALL:
        hit |= {ctxs("tiny", kind).e.test_gemm_regime(which, epi, M) for M in SMALL_M}
    hit |= {ctxs("tiny", "f16").e.test_gemm_regime(0, QKV, 5377), ctxs("tiny", "q8_0").e.test_gemm_regime(0, QKV, 43777),
            ctxs("tiny", "q4_k").e.test_gemm_regime(2, GELU_Q8K, 32769)}
    full = ctxs("full", "q4_k")
    hit.add(full.e.test_gemm_regime(0, QKV, 256 * persistent_rows(3 * full.D, cus, cdiv(512, 15))))
    nbm = next(n for n in range(103, 400) if tail_split(n * 256, full.D, full.F, cus) == n - 1)
    hit.add(full.e.test_gemm_regime(3, RESID, (nbm - 1) * 256 + 129))
    cap = 64 * (cus // 8 * 8) // 20               # the tile-list cap: its two sides are two regimes
    assert [full.e.test_gemm_regime(2, PRE_H, 256 * r) for r in (cap, cap + 1)] == [PERSISTENT, PIPE8]
    assert hit == {NARROW, T128, T128x256, PIPE8, PERSISTENT, TAIL, FIXED}, sorted(hit)


def test_hook_rejects_what_the_block_never_launches(ctxs):
    import q2a
    x = torch.zeros((40000, 256), dtype=torch.float32, device="cuda")
    o = [torch.zeros((40000 + 256, 1024), dtype=torch.int16, device="cuda").data_ptr()] * 6
    bad = [("f16", 2, PRE_H, 64), ("f16", 1, QKV, 64), ("f16", 0, RESID, 64), ("f16", 2, RESID, 64), ("f16", 2, GELU_Q8K, 33000),
           ("q8_0", 2, PRE_H, 64), ("q8_0", 2, GELU_Q8K, 33000), ("q4_k", 2, GELU_Q8K, 1500), ("q6_k", 2, GELU_Q8K, 33000),
           ("q4_k", 3, GELU_H, 64), ("q4_k", 2, 5, 64), ("q4_k", 4, RESID, 64), ("bf16", 2, PRE_H, 64)]
    for kind, which, epi, M in bad:
        e = ctxs("tiny", kind).e
        with pytest.raises(q2a.Q2AError) as ei:
            e.test_gemm_epi(0, which, epi, x.data_ptr(), M, o, ld=40192)
        assert ei.value.rc == -4, (kind, which, epi, M)
        with pytest.raises(q2a.Q2AError) as ei:
            e.test_gemm_regime(which, epi, M)
        assert ei.value.rc == -4, (kind, which, epi, M)
    e = ctxs("tiny", "q4_k").e
    for ld in (33000, 32768 - 256):          # not a multiple of 256; below M
        with pytest.raises(q2a.Q2AError) as ei:
            e.test_gemm_epi(0, 2, GELU_Q8K, x.data_ptr(), 32768, o, ld=ld)
        assert ei.value.rc == -4
