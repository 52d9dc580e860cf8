#!/usr/bin/env python3
"""Whole-step time of the variable-length encode against the padded encode.

    python diag/varlen_time.py [--clips 64] [--wt q4_k] [--rounds 4] [--steps 3] [--out FILE]

Full-size model, `--clips` 30 s clips resident in HBM; the key lengths are passed explicitly, so the same audio serves
every case. Cases: every key length 1500, 500 and 250, and one mixed batch (lengths drawn once from 100..1500, seed 0).
One process, alternating runs: every round measures, per case, the padded entry point (q2a_encode_device_padded) and
then the variable-length one (q2a_encode_device_varlen), `--steps` encodes each between two synchronisations, profiling
off: wall ms per step. Medians over the rounds and the spread (max - min) of either entry point per case. A last pass
with the engine's per-class timers on (q2a_profile_*, HIP events around every launch; its sum is not a step time) gives
the Q2A_PROF_* classes per step for both entry points, and from them the GEMMs' TF/s at the case's row count.
Prints one JSON line (and writes it to --out)."""
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
    ap.add_argument("--wt", default="q4_k")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--lens", default="1500,500,250")
    ap.add_argument("--workdir", default=os.environ.get("Q2A_BENCH_DIR", os.path.join(tempfile.gettempdir(), "q2a_bench")))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import q2a

    os.makedirs(args.workdir, exist_ok=True)
    model = bench.make_model(args.wt, args.workdir, min(16, os.cpu_count() or 8))
    eng = q2a.Engine(model, device=0)
    info = eng.info
    D, L, T = info.n_audio_state, info.n_audio_layer, info.n_audio_ctx
    B = args.clips
    eng.reserve(B)
    pcm = torch.from_numpy(bench.synth_clips(0, B)).cuda()
    out = torch.empty((B,) + eng.out_shape, dtype=torch.float32, device="cuda")
    ns = [bench.N_SAMPLES] * B
    cases = {f"key_len_{n}": [int(n)] * B for n in args.lens.split(",")}
    cases["mixed_100_1500"] = [int(x) for x in np.random.default_rng(0).integers(100, T + 1, size=B)]
    lib = q2a.lib()
    lib.q2a_profile_enable_mask.argtypes = [C.c_void_p, C.c_uint]
    ms = (C.c_double * 11)()
    cnt = (C.c_int64 * 11)()
    h = C.c_void_p(eng.h)
    entry = {"padded": eng.encode_device_padded, "varlen": eng.encode_device_varlen}

    def steps(which, kl):
        for _ in range(args.steps):
            entry[which](pcm.data_ptr(), bench.N_SAMPLES, ns, out.data_ptr(), key_len=kl)
        torch.cuda.synchronize()

    for kl in cases.values():   # warm-up, untimed (allocates the packed buffer too)
        for which in entry:
            entry[which](pcm.data_ptr(), bench.N_SAMPLES, ns, out.data_ptr(), key_len=kl)
    torch.cuda.synchronize()
    wall = {name: {"padded": [], "varlen": []} for name in cases}
    for _ in range(args.rounds):
        for name, kl in cases.items():
            for which in entry:
                t0 = time.perf_counter()
                steps(which, kl)
                wall[name][which].append((time.perf_counter() - t0) * 1e3 / args.steps)
    # per-class pass
    lib.q2a_profile_enable_mask(h, (1 << 11) - 1)
    classes = {}
    for name, kl in cases.items():
        classes[name] = {}
        for which in entry:
            lib.q2a_profile_read(h, ms, cnt, 11, 1)
            steps(which, kl)
            lib.q2a_profile_read(h, ms, cnt, 11, 1)
            classes[name][which] = {c: round(ms[i] / args.steps, 3) for i, c in enumerate(CLASSES)}
    lib.q2a_profile_enable_mask(h, 0)
    eng.close()

    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    F = 4 * D
    shapes = {"gemm_qkv": (3 * D, D), "gemm_o": (D, D), "gemm_fc1": (F, D), "gemm_fc2": (D, F)}
    res = {"clips": B, "wt": args.wt, "steps_per_measurement": args.steps, "rounds": args.rounds, "cases": {}}
    for name, kl in cases.items():
        m_tot, _ = q2a.varlen_rows(kl, T)
        rows = {"padded": B * T, "varlen": m_tot}
        tf = {which: {g: round(2.0 * rows[which] * n * k * L / (classes[name][which][g] * 1e-3) / 1e12, 1)
                      for g, (n, k) in shapes.items() if classes[name][which][g] > 0} for which in entry}
        res["cases"][name] = {
            "m_tot": m_tot, "rows_padded": B * T,
            "wall_ms_per_step": {w: [round(x, 2) for x in v] for w, v in wall[name].items()},
            "median_ms": {w: round(med(v), 2) for w, v in wall[name].items()},
            "spread_ms": {w: round(max(v) - min(v), 2) for w, v in wall[name].items()},
            "class_ms_per_step": classes[name], "gemm_tflops": tf}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
