#!/usr/bin/env python3
"""Whole-step time of q2a_audio_features_device against the composition of the existing entry points.

    python diag/features_time.py [--clips 64] [--wt q4_k] [--rounds 4] [--steps 3] [--out FILE]

Full-size model with a 1280 -> 4096 projector of the same weight type, `--clips` 30 s clips resident in HBM as PCM, at
key lengths 250 and 1500. Per case two calls that must give the same bytes (checked):
  composed  encode_device_varlen into the padded [clips][750][1280] buffer, a torch gather of the valid rows
            (torch.cat of out[c, :out_len[c]]), Projector.apply
  fused     audio_features_device into [N_tot][4096]
One process, alternating runs: every round measures, per case, the composition and then the new call, `--steps` calls
each between two synchronisations, profiling off: wall ms per step. Medians over the rounds and the spread (max - min)
of either call per case. A last pass with the engine's per-class timers on (q2a_profile_*, HIP events around every
launch; its sum is not a step time; the projector's GEMM and torch's gather are in no class) gives the Q2A_PROF_*
classes per step for both. Prints one JSON line (and writes it to --out)."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (model generator, clip generator, package path)

CLASSES = ["mel", "conv1", "conv2", "ln", "gemm_qkv", "attn", "quant", "gemm_o", "gemm_fc1", "gemm_fc2", "pool"]
D_IN, D_OUT = 1280, 4096


def make_projector(wt: str, workdir: str) -> str:
    import q2a
    base = os.path.join(workdir, "projector-f16.bin")
    if not os.path.exists(base):
        subprocess.check_call([q2a.TOOL_PATH, "gen-projector", base, str(D_IN), str(D_OUT), "f16", "0x51A2"])
    if wt == "f16":
        return base
    path = os.path.join(workdir, f"projector-{wt}.bin")
    if not os.path.exists(path):
        subprocess.check_call([q2a.TOOL_PATH, "quantize", base, path, wt, "8"])
    return path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--wt", default="q4_k")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--workdir", default=os.environ.get("Q2A_BENCH_DIR", os.path.join(tempfile.gettempdir(), "q2a_bench")))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import q2a

    os.makedirs(args.workdir, exist_ok=True)
    model = bench.make_model(args.wt, args.workdir, min(16, os.cpu_count() or 8))
    eng = q2a.Engine(model, device=0)
    pr = q2a.Projector(make_projector(args.wt, args.workdir), device=0)
    B = args.clips
    eng.reserve(B)
    pcm = torch.from_numpy(bench.synth_clips(0, B)).cuda()
    ns = [bench.N_SAMPLES] * B
    padded = torch.empty((B,) + eng.out_shape, dtype=torch.float32, device="cuda")
    res_buf = {}

    def composed(kl):
        ol, _ = eng.encode_device_varlen(pcm.data_ptr(), bench.N_SAMPLES, ns, padded.data_ptr(), key_len=kl)
        rows = torch.cat([padded[c, :ol[c]] for c in range(B)])
        y = torch.empty((rows.shape[0], D_OUT), dtype=torch.float32, device="cuda")
        pr.apply(rows.data_ptr(), rows.shape[0], y.data_ptr())
        res_buf["composed"] = y

    def fused(kl):
        n_tot = q2a.packed_out_rows(kl)[0]
        y = torch.empty((n_tot, D_OUT), dtype=torch.float32, device="cuda")
        eng.audio_features_device(pcm.data_ptr(), bench.N_SAMPLES, ns, y.data_ptr(), 0, n_tot, projector=pr, key_len=kl)
        res_buf["fused"] = y

    cases = {f"key_len_{L}": {"composed": (lambda L=L: composed([L] * B)), "fused": (lambda L=L: fused([L] * B))}
             for L in (250, 1500)}
    lib = q2a.lib()
    lib.q2a_profile_enable_mask.argtypes = [C.c_void_p, C.c_uint]
    ms = (C.c_double * 11)()
    cnt = (C.c_int64 * 11)()
    h = C.c_void_p(eng.h)

    def steps(call):
        for _ in range(args.steps):
            call()
        torch.cuda.synchronize()

    same = {}
    for name, entry in cases.items():   # warm-up, untimed; the two calls give the same bytes
        for call in entry.values():
            call()
        torch.cuda.synchronize()
        a, b = res_buf["composed"], res_buf["fused"]
        same[name] = bool(a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)))
    wall = {name: {"composed": [], "fused": []} for name in cases}
    for _ in range(args.rounds):
        for name, entry in cases.items():
            for which, call in entry.items():
                t0 = time.perf_counter()
                steps(call)
                wall[name][which].append((time.perf_counter() - t0) * 1e3 / args.steps)
    lib.q2a_profile_enable_mask(h, (1 << 11) - 1)
    classes = {}
    for name, entry in cases.items():
        classes[name] = {}
        for which, call in entry.items():
            lib.q2a_profile_read(h, ms, cnt, 11, 1)
            steps(call)
            lib.q2a_profile_read(h, ms, cnt, 11, 1)
            classes[name][which] = {c: round(ms[i] / args.steps, 3) for i, c in enumerate(CLASSES)}
    lib.q2a_profile_enable_mask(h, 0)
    res_buf.clear()
    pr.close()
    eng.close()

    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    res = {"clips": B, "wt": args.wt, "projector": [D_IN, D_OUT], "steps_per_measurement": args.steps, "rounds": args.rounds,
           "cases": {}}
    for name in cases:
        res["cases"][name] = {
            "same_bytes": same[name],
            "wall_ms_per_step": {w: [round(x, 2) for x in v] for w, v in wall[name].items()},
            "median_ms": {w: round(med(v), 2) for w, v in wall[name].items()},
            "spread_ms": {w: round(max(v) - min(v), 2) for w, v in wall[name].items()},
            "class_ms_per_step": classes[name]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
