"""Rows of the five ggml block formats for the quantized embedding table's tests, and their float64 decode.

rows(t, n_cols): uint8 [n][row_size] — (a) the host library's q2a_quantize_row_* on a seeded numpy draw at three
magnitudes, (b) hand-made end-code blocks: d / dmin over the largest finite fp16, the smallest subnormal, 0 and a negative
value; every 6-bit scale and min 63; Q6_K scales -128 and 127; codes all 0 and all maximum (Q8_0: -128 and 127).
decode(t, rows, n_cols): float32(the float64 formula of ggml's dequantize_row_*), read off the block bytes in numpy.
Both are computed once per (type, n_cols)."""
import ctypes as C
import functools

import numpy as np

Q4_0, Q8_0, Q4_K, Q5_K, Q6_K = 2, 8, 12, 13, 14
TYPES = {"q4_0": Q4_0, "q8_0": Q8_0, "q4_k": Q4_K, "q5_k": Q5_K, "q6_k": Q6_K}
BLOCK = {Q4_0: (18, 32), Q8_0: (34, 32), Q4_K: (144, 256), Q5_K: (176, 256), Q6_K: (210, 256)}   # bytes, columns
D_BITS = [0x7BFF, 0x0001, 0x0000, 0xB266]   # 65504, 2^-24, 0, about -0.2
N_QUANT = 281


def _f16(b):
    """little-endian byte pairs [..., 2] -> float64"""
    return np.ascontiguousarray(b).view(np.float16)[..., 0].astype(np.float64)


def _scale_min_k4(s):
    """get_scale_min_k4 on scales [..., 12] -> sc, m [..., 8]"""
    s = s.astype(np.int64)
    sc = np.concatenate([s[..., 0:4] & 63, (s[..., 8:12] & 0xF) | ((s[..., 0:4] >> 6) << 4)], -1)
    m = np.concatenate([s[..., 4:8] & 63, (s[..., 8:12] >> 4) | ((s[..., 4:8] >> 6) << 4)], -1)
    return sc, m


def decode(t, rows, n_cols):
    bb, bc = BLOCK[t]
    nb = n_cols // bc
    b = rows[:, :nb * bb].reshape(len(rows), nb, bb)
    if t in (Q4_0, Q8_0):
        d = _f16(b[..., 0:2])[..., None]
        q = b[..., 2:].view(np.int8) if t == Q8_0 else np.concatenate([b[..., 2:] & 0xF, b[..., 2:] >> 4], -1).astype(np.int64) - 8
        y = q * d
    elif t in (Q4_K, Q5_K):
        d, dmin = _f16(b[..., 0:2]), _f16(b[..., 2:4])
        sc, m = _scale_min_k4(b[..., 4:16])
        qs = b[..., (48 if t == Q5_K else 16):].reshape(len(rows), nb, 4, 1, 32).astype(np.int64)
        q = np.concatenate([qs & 0xF, qs >> 4], 3).reshape(len(rows), nb, 8, 32)
        if t == Q5_K:
            q = q + (((b[..., None, 16:48].astype(np.int64) >> np.arange(8)[:, None]) & 1) << 4)
        y = (d[..., None] * sc)[..., None] * q - (dmin[..., None] * m)[..., None]
    else:
        k = np.arange(256)
        h, r, l = k // 128, (k % 128) // 32, k % 32
        n = b[..., 64 * h + 32 * (r & 1) + l].astype(np.int64)
        q = ((n >> (4 * (r >> 1))) & 0xF) | (((b[..., 128 + 32 * h + l].astype(np.int64) >> (2 * r)) & 3) << 4)
        y = (_f16(b[..., 208:210])[..., None] * b[..., 192 + k // 16].view(np.int8)) * (q - 32)
    return y.reshape(len(rows), n_cols).astype(np.float32)


def _end_code_rows(t, n_cols):
    bb, bc = BLOCK[t]
    nb = n_cols // bc
    out = []
    for v in range(16):   # the d value rotates from block to block; codes and scales by the row
        row = np.zeros((nb, bb), dtype=np.uint8)
        code = 0x00 if v & 4 else 0xFF
        for i in range(nb):
            d = np.array([D_BITS[(v + i) % 4]], dtype="<u2").view(np.uint8)
            if t in (Q4_K, Q5_K):
                row[i, 0:2], row[i, 2:4] = d, np.array([D_BITS[(v // 4 + 1 + i) % 4]], dtype="<u2").view(np.uint8)
                row[i, 4:16], row[i, 16:] = 0xFF, code
            elif t == Q6_K:
                row[i, 208:210], row[i, 0:192] = d, code
                row[i, 192:208] = 0x80 if v & 8 else 0x7F
            else:
                row[i, 0:2] = d
                row[i, 2:] = code if t == Q4_0 else (0x80 if v & 4 else 0x7F)
        out.append(row.reshape(-1))
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def rows(t, n_cols):
    import q2a
    fn = getattr(q2a._host(), "q2a_quantize_row_" + {Q4_0: "q4_0", Q8_0: "q8_0", Q4_K: "q4_K", Q5_K: "q5_K", Q6_K: "q6_K"}[t])
    fn.argtypes, fn.restype = [C.c_void_p, C.c_void_p, C.c_int64], None
    x = np.random.default_rng(100 * t + n_cols).standard_normal((N_QUANT, n_cols)).astype(np.float32)
    x *= np.float32(10.0) ** (np.arange(N_QUANT) % 3 * 3 - 4)[:, None].astype(np.float32)   # 1e-4, 1e-1, 1e2
    quant = np.zeros((N_QUANT, n_cols // BLOCK[t][1] * BLOCK[t][0]), dtype=np.uint8)
    for i in range(N_QUANT):
        fn(x[i].ctypes.data_as(C.c_void_p), quant[i].ctypes.data_as(C.c_void_p), n_cols)
    out = np.concatenate([quant, _end_code_rows(t, n_cols)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def values(t, n_cols):
    v = decode(t, rows(t, n_cols), n_cols)
    v.setflags(write=False)
    return v
