"""Rules, inputs and comparisons shared by tests/test_gemm_epi_cases_cpu.py and tests/test_gpu_gemm_epilogues.py: what
each fused epilogue of the weight GEMM (q2a_gemm.hip: val() and the store code behind it) must put into memory for
given raw f32 accumulators — the values q2a_test_linear returns (Q2A_EPI_STORE_F with store_bias 0). Every rule is
plain numpy in f32, one rounding per written operation:

  QKV       v = acc + bias; the Q third only: v = v * qscale; hi = fp16(v), lo = fp16(v - f32(hi))
            bf16 contract: bf16(v), no lo, V stored as V^T [clip][head][64][TP]
  RESID     (acc + bias) + x
  PRE_H     fp16(acc + bias)
  GELU_H    v = acc + bias: v <= -10 -> +0, v >= 10 -> fp16(v) (the fp16 carry pinned in tests/test_gpu_operands.py),
            else ggml's fp16 table at fp16(v); F32 files: the row again at column 2F (o_dup)
  GELU_Q8K  quantize_row_q8_K_ref of the GELU_H values of the row (operand_cases.check_q8k)
"""
import numpy as np

import operand_cases as oc

LOG2E = np.float32(1.4426950408889634)


def qscale(dh: int, bf16: bool = False) -> np.float32:
    """run_block's Q scale: (1.0f / sqrtf(dh)) and, under the reference contract, one f32 multiply by fl(log2 e)."""
    s = np.float32(1.0) / np.sqrt(np.float32(dh))
    return np.float32(s) if bf16 else np.float32(s * LOG2E)


# ------------------------------------------------------------------------------------------------------------ rules
def _biased(acc: np.ndarray, bias: np.ndarray) -> np.ndarray:
    v = oc.f32(acc) + oc.f32(bias)[None, :]
    assert v.dtype == np.float32
    return v


def rule_qkv(acc: np.ndarray, bias: np.ndarray, D: int, qs, bf16: bool = False) -> dict:
    """acc [M][3D], bias [3D] -> uint16 bit images [M][D]: reference contract qh, ql, kh, kl, vh, vl; bf16 contract
    q, k, v (V still row-major: vt_image lays it out)."""
    v = _biased(acc, bias)
    v[:, :D] = v[:, :D] * np.float32(qs)
    if bf16:
        b = oc.bf16_bits(v)
        return {"q": b[:, :D], "k": b[:, D:2 * D], "v": b[:, 2 * D:]}
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)
    hb, lb = hi.view(np.uint16), lo.view(np.uint16)
    return {"qh": hb[:, :D], "ql": lb[:, :D], "kh": hb[:, D:2 * D], "kl": lb[:, D:2 * D], "vh": hb[:, 2 * D:], "vl": lb[:, 2 * D:]}


def vt_image(v_bits: np.ndarray, T: int, TP: int, fill: int, clips: int = None) -> np.ndarray:
    """Row-major V bits [M][D] -> the V^T image [clips][H][64][TP] with `fill` wherever the epilogue may not write:
    t >= T of every clip and every t past row M-1 of the last clip — except one whole clip alone (M == T), whose pad
    columns T <= t < TP the epilogue writes as zeros (q2a_gemm.hip: "so no caller has to clear them")."""
    M, D = v_bits.shape
    H = D // 64
    n = -(-M // T)
    clips = n if clips is None else clips
    out = np.full((clips, H, 64, TP), fill, np.uint16)
    for c in range(n):
        rows = v_bits[c * T:min((c + 1) * T, M)]                       # [t][H*64]
        out[c, :, :, :len(rows)] = rows.reshape(len(rows), H, 64).transpose(1, 2, 0)
    if M == T:
        out[0, :, :, T:TP] = 0
    return out


def rule_resid(acc: np.ndarray, bias: np.ndarray, x: np.ndarray) -> np.ndarray:
    r = _biased(acc, bias) + oc.f32(x)
    assert r.dtype == np.float32
    return r


def rule_pre_h(acc: np.ndarray, bias: np.ndarray) -> np.ndarray:
    return oc.fp16_bits(_biased(acc, bias))


def gelu_h_bits(v: np.ndarray) -> np.ndarray:
    """The GELU epilogues on the f32 pre-activation v: the range branches test v itself, the table is read at fp16(v).
    The two disagree only for |v| < 10 that rounds to fp16 +-10 (a 2^-8 wide sliver each side): at +10 both give 10;
    at -10 the branch gives +0 but the table entry is read, which holds -0 (q2a_internal.h, Q2A_EPI_PRE_H: "for every
    fp16 h <= -10 the table holds -0": tanhf saturates, 0.5 h (1 - 1))."""
    v = oc.f32(v)
    h = oc.fp16_bits(v)
    tab = oc.gelu_table_bits().copy()
    tab[0xC900] = 0x8000                  # the entry at fp16 -10 itself (the oracle's GELU never reads it: its branch)
    return np.where(v <= -10, np.uint16(0), np.where(v >= 10, h, tab[h])).astype(np.uint16)


def rule_gelu_h(acc: np.ndarray, bias: np.ndarray, o_dup: bool = False, fill: int = oc.SENTINEL16) -> np.ndarray:
    """fp16 bits [M][F]; o_dup (F32 files): [M][3F] = row | untouched (fill) | row."""
    g = gelu_h_bits(_biased(acc, bias))
    if not o_dup:
        return g
    return np.concatenate([g, np.full_like(g, fill), g], axis=1)


def gelu_h_values(acc: np.ndarray, bias: np.ndarray) -> np.ndarray:
    """The GELU_H output as f32 values: what GELU_Q8K quantizes (check_q8k's y)."""
    return gelu_h_bits(_biased(acc, bias)).view(np.float16).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------- inputs
def input_rows(M: int, K: int, seed: int, scale: float = 1.0, zero_rows=()) -> np.ndarray:
    """realistic_rows-style Gaussian rows (a few outlier channels, a common offset) with all-zero rows planted."""
    rng = np.random.default_rng(11000 + seed)
    x = rng.standard_normal((M, K)).astype(np.float32)
    x[:, rng.choice(K, size=4, replace=False)] *= 8.0
    x = (x + np.float32(0.25)) * np.float32(scale)
    for r in zero_rows:
        x[r] = 0.0
    return x


def resid_rows(M: int, D: int, seed: int) -> np.ndarray:
    """Gaussian residuals with every 97th row at 1e4 scale: there (acc + bias) + x differs from acc + (bias + x)."""
    rng = np.random.default_rng(12000 + seed)
    x = rng.standard_normal((M, D)).astype(np.float32)
    x[5 % M::97] *= np.float32(1e4)
    return x


def seam_rows(M: int, seams=(), tile: int = 256) -> np.ndarray:
    """Rows on both sides of every seam in `seams` (a seam s separates rows s-1 | s), row 0 and row M-1."""
    r = {0, M - 1}
    for s in seams:
        r |= {s - 1, s}
    return np.array(sorted(x for x in r if 0 <= x < M), dtype=np.int64)


def sample_rows(M: int, tile: int, extra_seams=(), n: int = 384, seed: int = 0) -> np.ndarray:
    """At most n rows: row 0, row M-1, both sides of every tile-row seam (every one while they fit, else an even
    spread that keeps the first and the last) and of every seam in extra_seams, filled up at random."""
    seams = np.arange(tile, M, tile)
    must = seam_rows(M, extra_seams)
    room = (n - len(must)) // 2
    if len(seams) > room:
        seams = seams[np.unique(np.linspace(0, len(seams) - 1, max(room, 2)).astype(np.int64))]
    rows = set(must.tolist())
    for s in seams:
        rows |= {int(s) - 1, int(s)}
    rows = sorted(rows)[:n] if len(rows) > n else sorted(rows)
    rng = np.random.default_rng(13000 + seed)
    rest = np.setdiff1d(np.arange(M), rows)
    fill = rng.choice(rest, size=min(n - len(rows), len(rest)), replace=False) if n > len(rows) else []
    out = np.unique(np.concatenate([np.array(rows, np.int64), np.array(fill, np.int64)]))
    assert len(out) <= n and set(must.tolist()) <= set(out.tolist())
    return out


# ------------------------------------------------------------------------------------------------------ comparisons
def first_mismatch(got: np.ndarray, want: np.ndarray, tile=(256, 256), wave_rows: int = 128):
    """None when the 2-D arrays are equal bit for bit, else where they first differ (row-major order): row, column,
    the tile (tile row, tile column) and the wave-row inside the tile, the 16-row group and the row within it (the
    epilogues' line exchange trades rows l and l ^ 8 of a group), the two values, and how many elements and rows
    differ."""
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, (got.shape, want.shape)
    kind = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    g, w = got.view(kind), want.view(kind)
    ne = g != w
    if not ne.any():
        return None
    rows = np.flatnonzero(ne.any(axis=1))
    r = int(rows[0])
    c = int(np.flatnonzero(ne[r])[0])
    bm, bn = tile
    return {"row": r, "col": c, "tile": (r // bm, c // bn), "wave_row": (r % bm) // wave_rows, "group16": (r % bm) // 16,
            "row_in_group": r % 16, "got": hex(int(g[r, c])), "want": hex(int(w[r, c])), "n_elements": int(ne.sum()),
            "n_rows": int(len(rows)), "last_row": int(rows[-1])}


def assert_same(got: np.ndarray, want: np.ndarray, what: str, tile=(256, 256), wave_rows: int = 128) -> None:
    bad = first_mismatch(got, want, tile, wave_rows)
    assert bad is None, f"{what}: {bad}"


def assert_untouched(buf: np.ndarray, what: str) -> None:
    """Every element still holds the sentinel it was filled with."""
    s = oc.SENTINEL16 if buf.dtype.itemsize == 2 else oc.SENTINEL32
    kind = np.uint16 if buf.dtype.itemsize == 2 else np.uint32
    b = buf.view(kind).reshape(buf.shape[0], -1) if buf.ndim > 1 else buf.view(kind).reshape(1, -1)
    hit = np.argwhere(b != s)
    assert len(hit) == 0, f"{what}: {len(hit)} elements behind the output were written, first at {tuple(hit[0])}"


def decode_q8k(codes16: np.ndarray, d32: np.ndarray, aext16: np.ndarray, M: int) -> dict:
    """The GELU_Q8K outputs (codes [rows][F], d [F/256][ld], block sums [F/256][ld][16]) -> check_q8k's `got`."""
    hi, lo = oc.decode_bsum(aext16, M)
    return {"codes": oc.decode_codes(codes16[:M]), "d": oc.decode_d(d32.view(np.float32), M), "hi": hi, "lo": lo}


# ---------------------------------------------------------------------------------------- whole-buffer checkers
# `bufs` are the buffers the hook wrote into, guard rows included (filled with the sentinel beforehand); M the row
# count of the launch. Each checker asserts the exact rule on rows 0 .. M-1 and the sentinel everywhere else.
QKV_NAMES = ("qh", "ql", "kh", "kl", "vh", "vl")


def check_qkv(bufs, acc, bias, D, qs, M, what="", tile=(256, 256)):
    want = rule_qkv(acc, bias, D, qs)
    for name, b in zip(QKV_NAMES, bufs):
        assert_same(b[:M], want[name], f"{what} {name}", tile)
        assert_untouched(b[M:], f"{what} {name} rows >= M")


def vt_cut_group(M: int, T: int):
    """(clip, t0, t1): the t range the V^T epilogue writes past row M-1 when M % 4 != 0, or None. It stores t in groups
    of four (one 8-byte store), the group that holds row M-1 whole: t0 = M % T .. t1 = t0 rounded up to 4, exclusive,
    of the partly filled clip get values computed from operand rows >= M. A stated deviation: no encode
    launches the V^T contract with M % 4 != 0 (M = clips * T, T % 4 == 0)."""
    if M % 4 == 0:
        return None
    t0 = M % T
    return M // T, t0, (t0 + 3) // 4 * 4


def check_qkv_bf16(bufs, acc, bias, D, qs, M, T, TP, what="", tile=(256, 256)):
    """bufs = Q [rows][D], K [rows][D], V^T [clips][H][64][TP] (clips may exceed ceil(M / T): whole guard clips). V^T is
    held to the rule and the sentinel on every element but vt_cut_group's (at most three t of one clip)."""
    want = rule_qkv(acc, bias, D, qs, bf16=True)
    for name, b in zip(("q", "k"), bufs):
        assert_same(b[:M], want[name], f"{what} {name}", tile)
        assert_untouched(b[M:], f"{what} {name} rows >= M")
    vt = bufs[2]
    img = vt_image(want["v"], T, TP, oc.SENTINEL16, clips=vt.shape[0])
    cut = vt_cut_group(M, T)
    if cut is not None:
        c, t0, t1 = cut
        img[c, :, :, t0:t1] = vt[c, :, :, t0:t1]
    bad = first_mismatch(vt.reshape(-1, TP), img.reshape(-1, TP), tile=(64, TP), wave_rows=64)
    if bad is not None:
        c, rem = divmod(bad["row"], (D // 64) * 64)
        bad.update(clip=c, head=rem // 64, d=rem % 64, t=bad["col"], row_of_batch=c * T + bad["col"])
    assert bad is None, f"{what} V^T (sentinel expected past the rows written): {bad}"


def check_resid(buf, acc, bias, x, M, what="", tile=(256, 256)):
    assert_same(buf[:M], rule_resid(acc, bias, x), f"{what} residual", tile)
    assert_untouched(buf[M:], f"{what} rows >= M")


def check_h(buf, acc, bias, M, gelu: bool, o_dup: bool = False, what="", tile=(256, 256)):
    want = rule_gelu_h(acc, bias, o_dup) if gelu else rule_pre_h(acc, bias)
    assert_same(buf[:M], want, f"{what} {'GELU_H' if gelu else 'PRE_H'}", tile)
    assert_untouched(buf[M:], f"{what} rows >= M")


def check_gelu_q8k(codes, d, aext, acc, bias, M, what=""):
    """codes [rows][F] uint16, d [F/256][ld] 32-bit, aext [F/256][ld][16] uint16."""
    assert_untouched(codes[M:], f"{what} codes rows >= M")
    assert_untouched(d[:, M:], f"{what} d rows >= M")
    assert_untouched(aext[:, M:].reshape(aext.shape[0], -1), f"{what} block sums rows >= M")
    oc.check_q8k(decode_q8k(codes, d, aext, M), gelu_h_values(acc, bias), what)
