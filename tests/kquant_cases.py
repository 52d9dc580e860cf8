"""Inputs and references shared by tests/test_kquant_formats_cpu.py, tests/test_gpu_kquant.py and
tests/golden/make_golden_kq.py (Q5_K / Q6_K model files).

1. The "ext" tiny model: the deterministic tiny F16 model with hand-made rows written into layer 0's q_proj, out_proj,
   fc1 and fc2 weights (every value exact in fp16), so that both quantizers reach the branches and the end codes random
   weights seldom do. Per matrix, rows 0..5:
     0  all zeros                 every 256-block zeroed (Q6_K: GROUP_MAX_EPS branch; Q5_K: d = 0, dmin = 0)
     1  N(0, 0.02) with one 6.0   a single large outlier per 256-block
     2  all +0.75                 Q5_K: sc = 63, q = 31 everywhere; Q6_K: sc = -128, q = 0 everywhere
     3  +1, -1, +1, ...           Q6_K: sc = -128 with q = 63 (the -1s; the scale search settles on +-31, the +1s at q = 1)
     4  all -0.75                 Q6_K: sc = -128, q = 0 with d < 0; Q5_K: q = 0 with the largest min
     5  first 256-block zeros, then N(0, 0.02): a d = 0 block in front of ordinary ones (the block-ratio recurrence)
2. The integer contract of one linear in float64 (kq_linear_ref): ggml's vec_dot of the type against Q8_K
   activations, per 256-block  Q5_K: d*dy*I - dmin*dy*sum_j m_j*bsum_j,  Q6_K: d*dy*I  (ggml_vec_dot_q5_K_q8_K,
   ggml_vec_dot_q6_K_q8_K), with I the integer dot of the block.
"""
import json
import os

import numpy as np

import oracle_py
from q2a import ggmlfile

D, F = 256, 1024
WT_TYPE = {"q5_k": ggmlfile.TYPE_Q5_K, "q6_k": ggmlfile.TYPE_Q6_K}
WT_FTYPE = {"q5_k": 13, "q6_k": 14}
MATRIX_NAMES = {0: ["self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight"],
                1: ["self_attn.out_proj.weight"], 2: ["fc1.weight"], 3: ["fc2.weight"]}
EXT_ROWS = 6
EXT_TENSORS = ["layers.0.self_attn.q_proj.weight", "layers.0.self_attn.out_proj.weight", "layers.0.fc1.weight",
               "layers.0.fc2.weight"]


def kq_npz_name(key: str) -> str:
    """The fixture file an array lives in: the tiny models' sampled rows per weight type (0.77 MB each), everything
    else (full-size samples, their indices, the hand-made rows' reference bytes) in golden_kq.npz."""
    for wt in WT_TYPE:
        if key.startswith(f"tiny_{wt}_"):
            return f"golden_kq_tiny_{wt}.npz"
    return "golden_kq.npz"


def load_golden_kq(golden_dir: str):
    """(golden_kq.json, every golden_kq*.npz array) — tests/golden/make_golden_kq.py."""
    with open(os.path.join(golden_dir, "golden_kq.json")) as f:
        meta = json.load(f)
    arrays = {}
    for name in ["golden_kq.npz"] + [f"golden_kq_tiny_{wt}.npz" for wt in WT_TYPE]:
        arrays.update(np.load(os.path.join(golden_dir, name), allow_pickle=False))
    return meta, arrays


def ext_rows(K: int, seed: int) -> np.ndarray:
    """The hand-made rows [EXT_ROWS][K] (float16-exact values)."""
    rng = np.random.default_rng(seed)
    r = np.zeros((EXT_ROWS, K), np.float32)
    r[1] = rng.standard_normal(K) * 0.02
    r[1, 5::256] = 6.0
    r[2] = 0.75
    r[3] = np.where(np.arange(K) % 2 == 0, 1.0, -1.0)
    r[4] = -0.75
    r[5] = rng.standard_normal(K) * 0.02
    r[5, :256] = 0.0
    return r.astype(np.float16)


def write_ext_model(base_f16: str, out: str) -> None:
    """base_f16 (the tiny F16 model file) with the hand-made rows in place, written to out."""
    buf = np.fromfile(base_f16, dtype=np.uint8)
    mf = ggmlfile.read(base_f16)
    for i, name in enumerate(EXT_TENSORS):
        t = mf.t(name)
        assert t.type == ggmlfile.TYPE_F16
        rows = ext_rows(t.ne[0], 1000 + i)
        buf[t.offset:t.offset + rows.nbytes] = rows.view(np.uint8).reshape(-1)
    buf.tofile(out)


def matrix_tensors(mf, layer: int, which: int):
    return [mf.t(f"layers.{layer}.{n}") for n in MATRIX_NAMES[which]]


def kq_int_weights(tensors):
    """The matrix's integer view, rows of the listed tensors concatenated: Wint [N][K] float64 (sc_j * q, or
    sc_j * (q - 32)), d [N][nb], and for Q5_K dmin [N][nb], m [N][nb][8]."""
    parts = [t.kq() for t in tensors]
    typ = tensors[0].type
    v = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    N, nb = v["d"].shape
    if typ == ggmlfile.TYPE_Q5_K:
        w = v["q"].reshape(N, nb, 8, 32) * v["sc"][..., None]
    else:
        w = (v["q"] - 32).reshape(N, nb, 16, 16) * v["sc"][..., None]
    v["wint"] = w.reshape(N, nb * 256).astype(np.float64)
    return typ, v


def q8k(x: np.ndarray):
    """Q8_K of the rows of x (the C oracle's quantize_row_q8_K_ref): codes [M][K] int, d [M][nb] f32, bsums [M][nb][16]."""
    M, K = x.shape
    raw = oracle_py.quantize_act("q8k", x).reshape(M, K // 256, 292)
    d = raw[:, :, 0:4].copy().view(np.float32)[..., 0]
    qs = raw[:, :, 4:260].copy().view(np.int8).astype(np.int32).reshape(M, K)
    bs = raw[:, :, 260:292].copy().view(np.int16).astype(np.int32)
    return qs, d, bs


def kq_linear_ref(tensors, x: np.ndarray, return_int: bool = False):
    """y [M][N] float64 of ggml's Q5_K / Q6_K x Q8_K dot products. The integer dots are taken in float64, where they
    are exact (|I_b| <= 256 * 128 * 32 * 127 < 2^53). With return_int also the largest |I_b| and mag [M][N], the sum of
    the magnitudes of the terms each output is made of (|d dy| sum |sc q y| + |dmin dy| sum m |y|): what an fp32
    summation's error scales with when the terms cancel."""
    typ, v = kq_int_weights(tensors)
    qs, dy, bs = q8k(np.ascontiguousarray(x, dtype=np.float32))
    M, K = qs.shape
    nb = K // 256
    N = v["d"].shape[0]
    y = np.zeros((M, N), np.float64)
    mag = np.zeros((M, N), np.float64)
    imax = 0.0
    for b in range(nb):
        qb, wb = qs[:, b * 256:(b + 1) * 256].astype(np.float64), v["wint"][:, b * 256:(b + 1) * 256]
        I = qb @ wb.T
        imax = max(imax, float(np.abs(I).max()))
        dyb = dy[:, b].astype(np.float64)[:, None]
        d = v["d"][:, b].astype(np.float64)[None, :]
        term = d * I
        if return_int:
            mag += np.abs(dyb) * np.abs(d) * (np.abs(qb) @ np.abs(wb).T)
        if typ == ggmlfile.TYPE_Q5_K:
            bs32 = (bs[:, b, 0::2] + bs[:, b, 1::2]).astype(np.float64)              # [M][8]
            dmin, m = v["dmin"][:, b].astype(np.float64)[None, :], v["m"][:, b].astype(np.float64)
            term = term - dmin * (bs32 @ m.T)
            if return_int:
                mag += np.abs(dyb) * np.abs(dmin) * (np.abs(qb).reshape(M, 8, 32).sum(-1) @ m.T)
        y += dyb * term
    return (y, imax, mag) if return_int else y
