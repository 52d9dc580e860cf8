"""Inputs, references and layout decoders shared by tests/test_operand_cases_cpu.py and tests/test_gpu_operands.py:
the operands the conversion kernels (q2a_exact.hip, q2a_quant.h) write for the weight GEMMs, checked through
q2a_test_operand against the CPU oracle's quantize_row_q8_K_ref / AVX2 quantize_row_q8_0 (oracle_py.quantize_act).

Input families (every generator is deterministic in its arguments):
  tie_rows_q8k / tie_rows_q80   blocks whose scale is exactly +-1 and whose other elements are n + 0.5: every code is a
                                rounding tie, and the block maximum occurs twice with opposite signs
  gelu_tie_rows                 the same idea for the GELU + Q8_K kernel (inputs >= 10, which GELU returns unchanged)
  gelu_sign_rows                blocks whose maximum AFTER the GELU occurs twice with opposite signs
  edge_rows                     end codes, extreme block sums, zero blocks, the smallest and largest scales
  lattice_rows                  LayerNorm inputs on a 2^-6 lattice whose mean and variance are exact in any summation
                                order, so ln_ref predicts the LayerNorm-fused producers bit for bit
  realistic_rows                Gaussian rows with outlier channels and a common offset (order-dependent sums)
  gelu_pattern_rows             every finite fp16 bit pattern and -inf as a GELU input
"""
import numpy as np

import oracle_py
from kquant_cases import q8k

SENTINEL16 = 0x7B7B              # fp16 62 304: no code, and not a value any family produces
SENTINEL32 = 0x7B7B7B7B


# ---------------------------------------------------------------------------------------------- casts and references
def f32(x):
    return np.asarray(x, dtype=np.float32)


def bf16_bits(y: np.ndarray) -> np.ndarray:
    """Round-to-nearest-even bf16 bit patterns of finite f32 values."""
    u = f32(y).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def fp16_bits(y: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        return f32(y).astype(np.float16).view(np.uint16)


def split_bits(y: np.ndarray) -> np.ndarray:
    """The F32 files' operand [M][3K] = hi | lo | hi with hi = fp16(y), lo = fp16(y - hi)."""
    y = f32(y)
    hi = y.astype(np.float16)
    lo = (y - hi.astype(np.float32)).astype(np.float16)
    return np.concatenate([hi, lo, hi], axis=1).view(np.uint16)


def ordered16(bits: np.ndarray) -> np.ndarray:
    """fp16 / bf16 bit patterns as integers ordered like the values (adjacent values differ by 1; +0 and -0 coincide)."""
    b = bits.astype(np.int32)
    return np.where(b & 0x8000, -(b & 0x7FFF), b)


def ln_ref(x: np.ndarray, g: np.ndarray, b: np.ndarray, return_stats: bool = False):
    """ggml_compute_forward_norm_f32 + MUL + ADD with every f32 step explicit: double sums, each result rounded to f32,
    1 / sqrtf(var + 1e-5f), then (v * scale) * g + b."""
    x = f32(x)
    D = x.shape[1]
    mean = (x.astype(np.float64).sum(axis=1) / D).astype(np.float32)
    v = x - mean[:, None]                                   # f32
    sq = v * v                                              # f32
    var = (sq.astype(np.float64).sum(axis=1) / D).astype(np.float32)
    scale = np.float32(1.0) / np.sqrt(var + np.float32(1e-5))
    y = (v * scale[:, None]) * f32(g)[None, :] + f32(b)[None, :]
    assert y.dtype == np.float32
    return (y, mean, var) if return_stats else y


def ref_q8k(y: np.ndarray):
    """codes [M][K], d [M][nb] f32, bsum32 [M][nb][8] (the sum of the reference's two 16-wide bsums)."""
    qs, d, bs = q8k(f32(y))
    return qs, d, bs[:, :, 0::2] + bs[:, :, 1::2]


def ref_q80(y: np.ndarray):
    """codes [M][K], d [M][K/32] as the f32 value of the stored fp16, and the fp16 bits themselves."""
    y = f32(y)
    M, K = y.shape
    raw = oracle_py.quantize_act("q80", y).reshape(M, K // 32, 34)
    dbits = raw[:, :, 0:2].copy().view(np.uint16)[..., 0]
    qs = raw[:, :, 2:34].copy().view(np.int8).astype(np.int32).reshape(M, K)
    return qs, dbits.view(np.float16).astype(np.float32), dbits


_GELU_VALUES = None


def gelu_values() -> np.ndarray:
    """ggml_vec_gelu_f32 of the exact value of every fp16 bit pattern: f32 [65536] (x <= -10 -> 0, x >= 10 -> x, else
    the reference's fp16 table; NaN patterns give whatever the table holds and are never used)."""
    global _GELU_VALUES
    if _GELU_VALUES is None:
        L = oracle_py.lib()
        xs = np.arange(65536, dtype=np.uint16).view(np.float16).astype(np.float32)
        _GELU_VALUES = np.array([L.oracle_gelu(float(v)) for v in xs], dtype=np.float32)
    return _GELU_VALUES


def gelu_table_bits() -> np.ndarray:
    """The reference's 64 Ki-entry table itself: fp16(gelu_f32(fp16 x)) through oracle_gelu / oracle_fp32_to_fp16 for
    |x| < 10 (outside it the branches of ggml_vec_gelu_f32 never read the table)."""
    L = oracle_py.lib()
    g = gelu_values()
    return np.array([L.oracle_fp32_to_fp16(float(v)) for v in g], dtype=np.uint16)


def gelu_ref(xh: np.ndarray) -> np.ndarray:
    """GELU of fp16 rows (given as float16 or as uint16 bit patterns) -> f32."""
    bits = xh.view(np.uint16) if xh.dtype == np.float16 else xh
    return gelu_values()[bits]


# ------------------------------------------------------------------------------------------------- layout decoders
def decode_codes(raw16: np.ndarray):
    """Codes stored as halves -> int32 (asserting every one is an integer code)."""
    v = raw16.view(np.float16).astype(np.float32)
    q = np.rint(v).astype(np.int32)
    assert np.array_equal(q.astype(np.float32), v) and np.abs(q).max(initial=0) <= 127, "a stored code is not an integer code"
    return q


def decode_d(dy: np.ndarray, M: int) -> np.ndarray:
    """Block-major d[bf * ld + m] ([nblk][ld] f32) -> [M][nblk]."""
    return np.ascontiguousarray(dy[:, :M].T)


def decode_bsum(aext16: np.ndarray, M: int):
    """[nb][ld][16] halves = (hi, lo) pairs of the 8 32-wide sub-blocks -> hi, lo [M][nb][8] int32."""
    v = aext16.view(np.float16).astype(np.float32)[:, :M].transpose(1, 0, 2)
    q = np.rint(v).astype(np.int32)
    assert np.array_equal(q.astype(np.float32), v), "a block-sum half is not an integer"
    return np.ascontiguousarray(q[..., 0::2]), np.ascontiguousarray(q[..., 1::2])


# -------------------------------------------------------------------------------------------------- input families
# where the first block maximum sits, and where the later one of opposite sign: the first / last element of a lane's
# float4 (a lane of the 64-lane producers holds elements 4l .. 4l+3, a lane of the 16-lane ones 16s .. 16s+15), another
# lane, another 16-lane group (64 elements); the second of each pair in the same lane, the next lane, the same lane of
# the 16-lane layout, the last element
TIE_POSITIONS = ((0, 2), (3, 4), (21, 23), (150, 255))


def tie_block_q8k(variant: int, rng) -> np.ndarray:
    """256 values: the first maximum -+127 at TIE_POSITIONS[variant % 4][0] (sign by variant // 4), the same magnitude
    with the opposite sign later, and the 254 half-integers -126.5 .. 126.5 shuffled over the other positions."""
    p, p2 = TIE_POSITIONS[variant % 4]
    first = -127.0 if (variant // 4) % 2 == 0 else 127.0
    halves = rng.permutation(np.arange(-127, 127, dtype=np.float32) + np.float32(0.5))
    blk = np.empty(256, np.float32)
    rest = [i for i in range(256) if i not in (p, p2)]
    blk[rest] = halves
    blk[p], blk[p2] = first, -first
    return blk


def tie_rows_q8k(M: int, K: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(1000 + seed)
    nb = K // 256
    x = np.empty((M, nb, 256), np.float32)
    for m in range(M):
        for b in range(nb):
            x[m, b] = tie_block_q8k(m * nb + b + seed, rng)
    return x.reshape(M, K)


def tie_rows_q80(M: int, K: int, seed: int = 0) -> np.ndarray:
    """32-blocks with amax exactly 127 (d = 1, id = 1) at a moving position and sign, the rest half-integers."""
    rng = np.random.default_rng(2000 + seed)
    nb = K // 32
    x = (rng.integers(-127, 127, size=(M, nb, 32)).astype(np.float32) + np.float32(0.5))
    idx = np.arange(M * nb).reshape(M, nb)
    pos = (idx * 7 + seed) % 32
    sign = np.where((idx + seed) % 2 == 0, 127.0, -127.0).astype(np.float32)
    np.put_along_axis(x, pos[..., None], sign[..., None], axis=2)
    return x.reshape(M, K)


def gelu_tie_rows(M: int, K: int, seed: int = 0) -> np.ndarray:
    """fp16 inputs of the GELU + Q8_K kernel, all >= 10 (returned unchanged): the first maximum 127 at a TIE_POSITIONS
    place, the maximum once more later, the rest the half-integers 10.5 .. 126.5 — iscale is exactly -1 and every
    other code a tie."""
    rng = np.random.default_rng(3000 + seed)
    nb = K // 256
    x = (rng.integers(10, 127, size=(M, nb, 256)).astype(np.float32) + np.float32(0.5))
    for m in range(M):
        for b in range(nb):
            p, p2 = TIE_POSITIONS[(m * nb + b + seed) % 4]
            x[m, b, p] = x[m, b, p2] = 127.0
    return x.reshape(M, K).astype(np.float16)


def gelu_sign_rows(M: int, K: int, seed: int = 0) -> np.ndarray:
    """fp16 inputs of the GELU + Q8_K kernel whose block maximum occurs twice with opposite signs AFTER the GELU: an
    x in [-1, -0.5] and a y in [0.2, 0.4] whose table values are -v and +v exactly (v about 0.17), at the TIE_POSITIONS
    places in either order; every other input lies in (-0.1, 0.1), where |GELU| stays below 0.06."""
    g = gelu_values()
    neg = np.arange(0xB800, 0xBC01, dtype=np.uint16)       # -0.5 .. -1.0
    pos = np.arange(0x3266, 0x3667, dtype=np.uint16)       # 0.2 .. 0.4
    by_value = {float(g[b]): b for b in pos}
    pairs = [(xb, by_value[float(-g[xb])]) for xb in neg if float(-g[xb]) in by_value]
    assert len(pairs) >= 4
    rng = np.random.default_rng(3500 + seed)
    nb = K // 256
    x = rng.uniform(-0.1, 0.1, size=(M, nb, 256)).astype(np.float16).view(np.uint16)
    for m in range(M):
        for b in range(nb):
            i = m * nb + b + seed
            p, p2 = TIE_POSITIONS[i % 4]
            xb, yb = pairs[(i * 5) % len(pairs)]
            x[m, b, p], x[m, b, p2] = (xb, yb) if (i // 4) % 2 == 0 else (yb, xb)
    return x.reshape(M, K).view(np.float16)


EDGE_VARIANTS = ("const", "one_then_minus", "zero", "tiny_only", "amax_1e-5", "amax_6e6", "gauss")


def edge_block(name: str, rng, half: bool) -> np.ndarray:
    """One 256-block of the end-code family. half: values an fp16 row can hold (2^-24 for 1e-30, 6e4 for 6e6)."""
    c = np.float32(0.37)
    if name == "const":                  # every code -127: bsum32 -4064 = (hi, lo) (-64, 32)
        return np.full(256, c, np.float32)
    if name == "one_then_minus":         # first code -127, the others +127: bsums near +4064
        b = np.full(256, -c, np.float32)
        b[0] = c
        return b
    if name == "zero":                   # all zero, some of them -0.0
        b = np.zeros(256, np.float32)
        b[1::3] = -0.0
        return b
    if name == "tiny_only":              # the only non-zero value at the edge of the format
        b = np.zeros(256, np.float32)
        b[1::5] = -0.0
        b[77] = np.float32(2.0 ** -24) if half else np.float32(1e-30)
        return b
    if name in ("amax_1e-5", "amax_6e6"):   # every 32-block's amax exactly a: Q8_0's smallest / largest stored d
        a = np.float32(1e-5) if name == "amax_1e-5" else np.float32(6e4 if half else 6e6)
        b = (rng.uniform(-1, 1, 256).astype(np.float32) * a)
        b[np.arange(8) * 32 + np.array([0, 31, 5, 16, 9, 30, 1, 17])] = a * np.array([1, -1, 1, 1, -1, -1, 1, -1], np.float32)
        return b
    return rng.standard_normal(256).astype(np.float32)


def edge_rows(M: int, K: int, half: bool = False, seed: int = 0) -> np.ndarray:
    """Rows of edge blocks, the variants rotating over blocks and rows; every fifth row (m % 5 == 3) is all zero (with
    -0.0 entries). half=True: the result is float16 (every value exactly representable)."""
    rng = np.random.default_rng(4000 + seed)
    nb = K // 256
    x = np.empty((M, nb, 256), np.float32)
    for m in range(M):
        for b in range(nb):
            x[m, b] = edge_block("zero" if m % 5 == 3 else EDGE_VARIANTS[(m * nb + b + seed) % len(EDGE_VARIANTS)], rng, half)
    x = x.reshape(M, K)
    if half:
        h = x.astype(np.float16)
        return h
    return x


def edge_variant(m: int, b: int, nb: int, seed: int = 0) -> str:
    return "zero" if m % 5 == 3 else EDGE_VARIANTS[(m * nb + b + seed) % len(EDGE_VARIANTS)]


def lattice_rows(M: int, D: int, seed: int = 0) -> np.ndarray:
    """Entries k * 2^-6, |k| <= 4096, with each row's sum of k a multiple of D / 4: the mean is a multiple of 2^-8
    (exact in f32), the centred values are exact, their f32-rounded squares lie on a 2^-16 grid and sum to below 2^25,
    so both double sums are exact in any order. Row 2 (when there is one) is constant: variance 0, output = bias."""
    rng = np.random.default_rng(5000 + seed)
    k = rng.integers(-4096, 4097, size=(M, D)).astype(np.int64)
    k[:, 0] = 0
    k[:, 0] = -(k.sum(axis=1) % (D // 4))
    if M > 2:
        k[2, :] = 1234
    assert (k.sum(axis=1) % (D // 4) == 0).all() and np.abs(k).max() <= 4096
    return (k.astype(np.float64) * 2.0 ** -6).astype(np.float32)


def affine(D: int, seed: int = 0):
    """LayerNorm gain and bias: random, some gains negative, some exactly zero."""
    rng = np.random.default_rng(6000 + seed)
    g = (1.0 + 0.5 * rng.standard_normal(D)).astype(np.float32)
    g[3::17] *= -1
    g[5::29] = 0.0
    b = (0.3 * rng.standard_normal(D)).astype(np.float32)
    return g, b


def realistic_rows(M: int, D: int, seed: int = 0) -> np.ndarray:
    """Gaussian rows, a few outlier channels (x200) and a large common offset."""
    rng = np.random.default_rng(7000 + seed)
    x = rng.standard_normal((M, D)).astype(np.float32)
    x[:, rng.choice(D, size=4, replace=False)] *= 200.0
    return x + np.float32(30.0)


_PATTERN_POOL = None


def gelu_pattern_pool() -> np.ndarray:
    """uint16 [249][256]: every finite fp16 pattern and -inf (0xFC00), sorted by magnitude and cut into 256-blocks (the
    last block filled up from the start), each block's elements then shuffled."""
    global _PATTERN_POOL
    if _PATTERN_POOL is None:
        pos = np.arange(0x7C00, dtype=np.uint16)
        bits = np.stack([pos, pos | 0x8000], axis=1).reshape(-1)         # +x, -x by rising magnitude
        bits = np.concatenate([bits, np.array([0xFC00], np.uint16)])     # 63 489 patterns
        pad = (-len(bits)) % 256
        bits = np.concatenate([bits, bits[1000:1000 + pad]]).reshape(-1, 256)
        rng = np.random.default_rng(8000)
        _PATTERN_POOL = rng.permuted(bits, axis=1)
    return _PATTERN_POOL


def gelu_pattern_rows(M: int, K: int, seed: int = 0) -> np.ndarray:
    """uint16 bit patterns [M][K]: the pool's blocks in a shuffled order, repeated to fill the shape."""
    pool = gelu_pattern_pool()
    n = M * (K // 256)
    rng = np.random.default_rng(9000 + seed)
    order = np.concatenate([rng.permutation(len(pool)) for _ in range(-(-n // len(pool)))])[:n]
    return pool[order].reshape(M, K)


# ------------------------------------------------------------------------------------------------------- comparisons
def nonzero_blocks(y: np.ndarray, blk: int) -> np.ndarray:
    M, K = y.shape
    return (f32(y).reshape(M, K // blk, blk) != 0).any(axis=2)


def check_q8k(got: dict, y: np.ndarray, what: str = "") -> None:
    """got = decoded operand (codes, d, hi, lo) against the oracle's Q8_K of y, bit for bit. An all-zero block is the
    one stated difference: ggml stores d = 0, the engine a finite non-zero d (q2a_quant.h: it keeps the wide Q4_K
    GEMM's block-ratio rescaling finite) — its codes and block sums must be zero, its d finite."""
    qs, d, bs32 = ref_q8k(y)
    assert np.array_equal(got["codes"], qs), f"{what}: {int((got['codes'] != qs).sum())} Q8_K codes differ"
    nz = nonzero_blocks(y, 256)
    assert np.array_equal(got["d"].view(np.uint32)[nz], d.view(np.uint32)[nz]), f"{what}: d differs"
    assert np.isfinite(got["d"][~nz]).all() and (d[~nz] == 0).all(), f"{what}: d of an all-zero block"
    assert (got["lo"] >= 0).all() and (got["lo"] < 64).all(), f"{what}: bsum lo outside [0, 64)"
    assert np.array_equal(64 * got["hi"] + got["lo"], bs32), f"{what}: bsum32 differs"
    assert (qs[np.repeat(~nz, 256, axis=1)] == 0).all() and (bs32[~nz] == 0).all()


def check_q80(got: dict, y: np.ndarray, what: str = "") -> None:
    """Q8_0 codes and the fp16-rounded d against the oracle, bit for bit (an all-zero block: d = 0 on both sides)."""
    qs, d, _ = ref_q80(y)
    assert np.array_equal(got["codes"], qs), f"{what}: {int((got['codes'] != qs).sum())} Q8_0 codes differ"
    assert np.array_equal(got["d"].view(np.uint32), d.view(np.uint32)), f"{what}: d differs"
