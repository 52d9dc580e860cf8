"""The MXFP8 contract's quantisation rule in numpy, for test_mxfp8_pack_cpu.py and test_gpu_mxfp8.py.
32 consecutive finite values x along K: amax = max|x|; amax == 0 -> scale code 127; else e = floor(log2 amax) - 8, code =
clamp(e + 127, 0, 254); elements e4m3fn(x * 2^(127 - code)), nearest even, saturated at +-448."""
import numpy as np


def e4m3_bytes(v: np.ndarray) -> np.ndarray:
    """e4m3fn code of float64 v, |v| <= 448, round to nearest even."""
    a = np.abs(v)
    ex = np.maximum(np.frexp(a)[1] - 1, -6)             # exponent of the leading bit, the subnormals' at least
    q = np.rint(np.ldexp(a, 3 - ex)).astype(np.int64)   # mantissa in units of 2^(ex - 3): 0 .. 16 (np.rint: half to even)
    ex, q = ex + (q == 16), np.where(q == 16, 8, q)
    return (np.where(q < 8, q, ((ex + 7) << 3) | (q - 8)) | (np.signbit(v) << 7)).astype(np.uint8)


def mx_quant(x: np.ndarray):
    """x [..., K] (K % 32 == 0, finite) -> (bytes uint8 [..., K], scale codes uint8 [..., K/32])."""
    xb = np.asarray(x, dtype=np.float64).reshape(*x.shape[:-1], x.shape[-1] // 32, 32)
    amax = np.abs(xb).max(-1)
    e = np.frexp(np.where(amax == 0, 1.0, amax))[1] - 1 - 8   # floor(log2 amax) - 8
    code = np.where(amax == 0, 127, np.clip(e + 127, 0, 254)).astype(np.int64)
    scaled = np.clip(np.ldexp(xb, (127 - code)[..., None]), -448.0, 448.0)
    return e4m3_bytes(scaled).reshape(x.shape), code.astype(np.uint8)


def mx_value(b: np.ndarray, code: np.ndarray) -> np.ndarray:
    """the float64 values an MXFP8 operand stands for."""
    b = b.astype(np.int64).reshape(*code.shape, 32)
    ex, m = (b >> 3) & 15, b & 7
    mag = np.where(ex == 0, np.ldexp(m.astype(np.float64), -9), np.ldexp(8.0 + m, ex - 10))
    return np.ldexp(np.where(b & 0x80, -mag, mag), code.astype(np.int64)[..., None] - 127).reshape(*code.shape[:-1], -1)
