#!/usr/bin/env python3
"""Whole-step time of the MXFP8 activation contract beside the bf16 one, on the same Q8_0 file.

    python diag/mxfp8_time.py [--clips 64] [--rounds 5] [--steps 3] [--out FILE]

One full-size Q8_0 model, a bf16 engine (ACT_BF16) and an MXFP8 engine (ACT_MXFP8) open in ONE process; `--clips` 30 s
clips resident in HBM, the same buffer for both. Alternating rounds: every round measures each engine in turn, `--steps`
encodes (q2a_encode_device) between two synchronisations, profiling off: wall ms per step, medians over the rounds and
each engine's spread (max - min). A last pass with the per-class timers on (q2a_profile_*, HIP events around every
launch; its sum is not a step time) gives the Q2A_PROF_* classes per step and the GEMMs' T(FL)OP/s. Prints one JSON
line (and writes it to --out)."""
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--workdir", default=os.environ.get("Q2A_BENCH_DIR", os.path.join(tempfile.gettempdir(), "q2a_bench")))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import q2a

    os.makedirs(args.workdir, exist_ok=True)
    B = args.clips
    t0 = time.perf_counter()
    path = bench.make_model("q8_0", args.workdir, min(16, os.cpu_count() or 8))
    eng = {"bf16": q2a.Engine(path, device=0, act=q2a.ACT_BF16), "mxfp8": q2a.Engine(path, device=0, act=q2a.ACT_MXFP8)}
    setup_s = time.perf_counter() - t0
    info = eng["bf16"].info
    D, L, T = info.n_audio_state, info.n_audio_layer, info.n_audio_ctx
    pcm = torch.from_numpy(bench.synth_clips(0, B)).cuda()
    out = torch.empty((B,) + eng["bf16"].out_shape, dtype=torch.float32, device="cuda")
    ns = [bench.N_SAMPLES] * B
    lib = q2a.lib()
    lib.q2a_profile_enable_mask.argtypes = [C.c_void_p, C.c_uint]
    ms = (C.c_double * 11)()
    cnt = (C.c_int64 * 11)()

    def steps(k):
        for _ in range(args.steps):
            eng[k].encode_device(pcm.data_ptr(), bench.N_SAMPLES, ns, out.data_ptr())
        torch.cuda.synchronize()

    for k in eng:   # warm-up, untimed (allocates the workspaces)
        eng[k].reserve(B)
        eng[k].encode_device(pcm.data_ptr(), bench.N_SAMPLES, ns, out.data_ptr())
    torch.cuda.synchronize()
    wall = {k: [] for k in eng}
    for _ in range(args.rounds):
        for k in eng:
            t0 = time.perf_counter()
            steps(k)
            wall[k].append((time.perf_counter() - t0) * 1e3 / args.steps)
    classes = {}
    for k in eng:   # per-class pass
        h = C.c_void_p(eng[k].h)
        lib.q2a_profile_enable_mask(h, (1 << 11) - 1)
        lib.q2a_profile_read(h, ms, cnt, 11, 1)
        steps(k)
        lib.q2a_profile_read(h, ms, cnt, 11, 1)
        classes[k] = {c: round(ms[i] / args.steps, 3) for i, c in enumerate(CLASSES)}
        lib.q2a_profile_enable_mask(h, 0)
    for e in eng.values():
        e.close()

    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    F = 4 * D
    shapes = {"gemm_qkv": (3 * D, D), "gemm_o": (D, D), "gemm_fc1": (F, D), "gemm_fc2": (D, F)}
    res = {"clips": B, "file": "q8_0", "steps_per_measurement": args.steps, "rounds": args.rounds, "setup_s": round(setup_s, 1),
           "engines": {}}
    for k in eng:
        cl = classes[k]
        res["engines"][k] = {
            "wall_ms_per_step": [round(x, 2) for x in wall[k]],
            "median_ms": round(med(wall[k]), 2), "spread_ms": round(max(wall[k]) - min(wall[k]), 2),
            "class_ms_per_step": cl, "gemm_ms_per_step": round(sum(cl[g] for g in shapes), 3),
            "gemm_tops": {g: round(2.0 * B * T * n * kk * L / (cl[g] * 1e-3) / 1e12, 1) for g, (n, kk) in shapes.items() if cl[g] > 0}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
