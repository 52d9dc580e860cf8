#!/usr/bin/env python3
"""Whole-step time of the k-quant weight types side by side: Q5_K and Q6_K beside Q4_K and Q8_0.

    python diag/kquant_time.py [--clips 64] [--types q4_k,q5_k,q6_k,q8_0] [--rounds 4] [--steps 3] [--out FILE]

Full-size model of every type, one engine each, all open in ONE process; `--clips` 30 s clips resident in HBM, the
same buffer for every engine. Alternating rounds: every round measures each type in turn, `--steps` encodes
(q2a_encode_device) between two synchronisations, profiling off: wall ms per step. Medians over the rounds and each
type's spread (max - min). A last pass with the engine's per-class timers on (q2a_profile_*, HIP events around every
launch; its sum is not a step time) gives the Q2A_PROF_* classes per step, the GEMM classes' share of their sum and the
GEMMs' TF/s. Prints one JSON line (and writes it to --out)."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (model generator, clip generator, package path)

CLASSES = ["mel", "conv1", "conv2", "ln", "gemm_qkv", "attn", "quant", "gemm_o", "gemm_fc1", "gemm_fc2", "pool"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--types", default="q4_k,q5_k,q6_k,q8_0")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--workdir", default=os.environ.get("Q2A_BENCH_DIR", os.path.join(tempfile.gettempdir(), "q2a_bench")))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import q2a

    os.makedirs(args.workdir, exist_ok=True)
    types = args.types.split(",")
    B = args.clips
    t0 = time.perf_counter()
    eng = {wt: q2a.Engine(bench.make_model(wt, args.workdir, min(16, os.cpu_count() or 8)), device=0) for wt in types}
    setup_s = time.perf_counter() - t0
    info = eng[types[0]].info
    D, L, T = info.n_audio_state, info.n_audio_layer, info.n_audio_ctx
    pcm = torch.from_numpy(bench.synth_clips(0, B)).cuda()
    out = torch.empty((B,) + eng[types[0]].out_shape, dtype=torch.float32, device="cuda")
    ns = [bench.N_SAMPLES] * B
    lib = q2a.lib()
    lib.q2a_profile_enable_mask.argtypes = [C.c_void_p, C.c_uint]
    ms = (C.c_double * 11)()
    cnt = (C.c_int64 * 11)()

    def steps(wt):
        for _ in range(args.steps):
            eng[wt].encode_device(pcm.data_ptr(), bench.N_SAMPLES, ns, out.data_ptr())
        torch.cuda.synchronize()

    for wt in types:   # warm-up, untimed (allocates the workspaces)
        eng[wt].reserve(B)
        eng[wt].encode_device(pcm.data_ptr(), bench.N_SAMPLES, ns, out.data_ptr())
    torch.cuda.synchronize()
    wall = {wt: [] for wt in types}
    for _ in range(args.rounds):
        for wt in types:
            t0 = time.perf_counter()
            steps(wt)
            wall[wt].append((time.perf_counter() - t0) * 1e3 / args.steps)
    classes = {}
    for wt in types:   # per-class pass
        h = C.c_void_p(eng[wt].h)
        lib.q2a_profile_enable_mask(h, (1 << 11) - 1)
        lib.q2a_profile_read(h, ms, cnt, 11, 1)
        steps(wt)
        lib.q2a_profile_read(h, ms, cnt, 11, 1)
        classes[wt] = {c: round(ms[i] / args.steps, 3) for i, c in enumerate(CLASSES)}
        lib.q2a_profile_enable_mask(h, 0)
    for e in eng.values():
        e.close()

    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    F = 4 * D
    shapes = {"gemm_qkv": (3 * D, D), "gemm_o": (D, D), "gemm_fc1": (F, D), "gemm_fc2": (D, F)}
    res = {"clips": B, "steps_per_measurement": args.steps, "rounds": args.rounds, "setup_s": round(setup_s, 1), "types": {}}
    for wt in types:
        cl = classes[wt]
        gemm = sum(cl[g] for g in shapes)
        res["types"][wt] = {
            "wall_ms_per_step": [round(x, 2) for x in wall[wt]],
            "median_ms": round(med(wall[wt]), 2), "spread_ms": round(max(wall[wt]) - min(wall[wt]), 2),
            "class_ms_per_step": cl, "gemm_share_of_classes": round(gemm / sum(cl.values()), 3),
            "gemm_tflops": {g: round(2.0 * B * T * n * k * L / (cl[g] * 1e-3) / 1e12, 1) for g, (n, k) in shapes.items() if cl[g] > 0}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
