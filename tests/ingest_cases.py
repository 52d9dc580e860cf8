"""The value contract of the native-rate ingestion (include/q2a_encoder.h, q2a_ingest_*) restated in numpy float64 by
direct evaluation of g — no coefficient bank, no phases — and the inputs of tests/test_gpu_ingest.py."""
from math import gcd

import numpy as np

Z, BETA, RHO = 64, 14.769656459379492, 0.9475937167399596


def plan(rate):
    """(L, M, H, T): 16000 / rate = L / M reduced, H = ceil(Z / s), T = 2 H + 1, s = min(1, L / M)."""
    d = gcd(16000, rate)
    L, M = 16000 // d, rate // d
    H = -(-Z * max(L, M) // L)
    return L, M, H, 2 * H + 1


def source(wave):
    """x[k], float32: the downmix rule for int16 / float32 arrays [frames] or [frames][2]."""
    if wave.dtype == np.int16:
        w = wave.astype(np.int32)
        return (w / 32768.0 if w.ndim == 1 else (w[:, 0] + w[:, 1]) / 65536.0).astype(np.float32)   # exact in f32
    return wave if wave.ndim == 1 else np.float32(0.5) * (wave[:, 0] + wave[:, 1])


def resample64(x, rate):
    """(y, S): y[n] = sum over |s (k - t_n)| < Z of g(k - t_n) x[k] and S[n] = sum |g(k - t_n) x[k]|, in float64, for
    n < ceil(len(x) * 16000 / rate), t_n = n M / L."""
    L, M, H, _ = plan(rate)
    n_in = len(x)
    n_out = (n_in * 16000 + rate - 1) // rate
    if rate == 16000:
        return x.astype(np.float64), np.abs(x.astype(np.float64))
    s, den = min(1.0, L / M), max(L, M)
    xz = np.concatenate([np.zeros(H + 1), x.astype(np.float64), np.zeros(H + 1)])
    y, S = np.zeros(n_out), np.zeros(n_out)
    j = np.arange(-H - 1, H + 2)
    for a in range(0, n_out, 4096):
        n = np.arange(a, min(a + 4096, n_out))
        k = (n * M // L)[:, None] + j[None, :]             # every k that can satisfy the window condition, and more
        num = k * L - (n * M)[:, None]                     # k - t_n = num / L, s (k - t_n) = num / max(L, M)
        u = num / den
        inside = np.abs(num) < Z * den
        w = np.i0(BETA * np.sqrt(np.where(inside, 1.0 - (u / Z) ** 2, 0.0))) / np.i0(BETA)
        g = np.where(inside, RHO * s * np.sinc(RHO * u) * w, 0.0)
        p = g * xz[k + H + 1]
        y[n], S[n] = p.sum(axis=1), np.abs(p).sum(axis=1)
    return y, S


# the kernel's run: periods of L outputs a workgroup owns, as input frames (Q M): 64 periods where L >= 4, 1024 / L for
# L = 1, 2 (csrc/q2a_ingest.hip, q2a_ingest_geom_of). The longest clip covers more than two runs and a ragged end.
def run_frames(rate):
    L, M, _, _ = plan(rate)
    return (64 if L >= 4 else 1024 // L) * M


def clip_lengths(rate):
    _, M, _, _ = plan(rate)
    return [1, 100, 3 * M + 7, 2 * run_frames(rate) + run_frames(rate) // 3 + 11]


def wave(rate, n_in, fmt, channels, seed):
    """Seeded noise of amplitude 0.5, the first and last 50 frames at full scale."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(-0.5, 0.5, size=(n_in, channels))
    edge = np.where(rng.integers(0, 2, size=(50, channels)) == 1, 1.0, -1.0)
    w[:50] = edge[:n_in]
    w[max(0, n_in - 50):] = edge[: min(50, n_in)]
    w = w[:, 0] if channels == 1 else w
    return np.clip(np.round(w * 32767), -32768, 32767).astype(np.int16) if fmt == "s16" else w.astype(np.float32)
