"""Inputs and references shared by tests/test_k23_formats_cpu.py, tests/test_gpu_k23.py and
tests/golden/make_golden_k23.py (Q2_K / Q3_K model files).

The "ext" tiny model is kquant_cases' (the same hand-made rows: zeros, an outlier per block, +0.75, +-1, -0.75, a zero
first block). Between them the rows reach, as the CPU test asserts: Q2_K d = 0 with dmin != 0 (all -0.75: every value
is the min) and q = 3 with sc = 15 (all +0.75); Q3_K a negative d (all -0.75) and sc - 32 = -32 with q - 4 = -4 (all
+0.75: the product 128, the largest weight of the layout).

The integer contract of one linear in float64 (k23_linear_ref), ggml's vec_dot against Q8_K activations per 256-block:
Q3_K d*dy*I, Q2_K d*dy*I - dmin*dy*sum_j m_j*bsum16_j over the sixteen 16-sums (ggml_vec_dot_q3_K_q8_K, _q2_K_q8_K)."""
import json
import os

import numpy as np

import kquant_cases as kc
from q2a import ggmlfile

WT_TYPE = {"q2_k": ggmlfile.TYPE_Q2_K, "q3_k": ggmlfile.TYPE_Q3_K}
WT_FTYPE = {"q2_k": 10, "q3_k": 11}
TYPES = list(WT_TYPE)


def load_golden_k23(golden_dir: str):
    """(golden_k23.json, the arrays of golden_k23.npz and golden_k23_tiny_<wt>.npz) — tests/golden/make_golden_k23.py."""
    with open(os.path.join(golden_dir, "golden_k23.json")) as f:
        meta = json.load(f)
    arrays = {}
    for name in ["golden_k23.npz"] + [f"golden_k23_tiny_{wt}.npz" for wt in TYPES]:
        arrays.update(np.load(os.path.join(golden_dir, name), allow_pickle=False))
    return meta, arrays


def int_weights(tensors):
    """Rows of the listed tensors concatenated: wint [N][K] float64 ((sc & 15) * q, or (sc - 32) * (q - 4)), d [N][nb],
    and for Q2_K dmin [N][nb], m [N][nb][16]."""
    parts = [t.kq() for t in tensors]
    v = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    N, nb = v["d"].shape
    if tensors[0].type == ggmlfile.TYPE_Q2_K:
        w = v["q"].reshape(N, nb, 16, 16) * v["sc"][..., None]
    else:
        w = (v["q"] - 4).reshape(N, nb, 16, 16) * (v["sc"] - 32)[..., None]
    v["wint"] = w.reshape(N, nb * 256).astype(np.float64)
    return v


def k23_linear_ref(tensors, x: np.ndarray):
    """(y, mag) [M][N] float64: ggml's Q2_K / Q3_K x Q8_K dot products (integer dots exact in float64), and the sum of the
    magnitudes of the terms each output is made of (test_linear_extremes' per-row bound)."""
    v = int_weights(tensors)
    qs, dy, bs = kc.q8k(np.ascontiguousarray(x, dtype=np.float32))
    M, K = qs.shape
    N = v["d"].shape[0]
    y, mag = np.zeros((M, N)), np.zeros((M, N))
    for b in range(K // 256):
        qb, wb = qs[:, b * 256:(b + 1) * 256].astype(np.float64), v["wint"][:, b * 256:(b + 1) * 256]
        dyb = dy[:, b].astype(np.float64)[:, None]
        d = v["d"][:, b].astype(np.float64)[None, :]
        term = d * (qb @ wb.T)
        mag += np.abs(dyb) * np.abs(d) * (np.abs(qb) @ np.abs(wb).T)
        if "dmin" in v:
            dmin, m = v["dmin"][:, b].astype(np.float64)[None, :], v["m"][:, b].astype(np.float64)
            term = term - dmin * (bs[:, b].astype(np.float64) @ m.T)
            mag += np.abs(dyb) * np.abs(dmin) * (np.abs(qb).reshape(M, 16, 16).sum(-1) @ m.T)
        y += dyb * term
    return y, mag
