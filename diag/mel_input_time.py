#!/usr/bin/env python3
"""Whole-step time of the encode from log-mel features against the encode from PCM.

    python diag/mel_input_time.py [--clips 64] [--wt q4_k] [--rounds 4] [--steps 3] [--out FILE]

Full-size model, `--clips` 30 s clips resident in HBM as PCM and as their log-mel (q2a_pcm_to_mel of each clip,
[clips][128][6000] f32), so both inputs describe the same audio and the outputs must be the same bytes (checked).
Cases: the plain encode, and the variable-length encode at key length 250 (5 s clips). One process, alternating runs:
every round measures, per case, the PCM entry point and then the mel entry point, `--steps` encodes each between two
synchronisations, profiling off: wall ms per step. Medians over the rounds and the spread (max - min) of either input
per case. A last pass with the engine's per-class timers on (q2a_profile_*, HIP events around every launch; its sum is
not a step time) gives the Q2A_PROF_* classes per step for both inputs: the mel class is what the input costs (the mel
kernels, or the ingest kernel), every other class runs the same launches. Prints one JSON line (and writes it to --out)."""
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
    ap.add_argument("--workdir", default=os.environ.get("Q2A_BENCH_DIR", os.path.join(tempfile.gettempdir(), "q2a_bench")))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import q2a

    os.makedirs(args.workdir, exist_ok=True)
    model = bench.make_model(args.wt, args.workdir, min(16, os.cpu_count() or 8))
    eng = q2a.Engine(model, device=0)
    B, M = args.clips, eng.info.n_mels
    eng.reserve(B)
    clips = bench.synth_clips(0, B)
    n_len = (bench.N_SAMPLES + 480000) // 160
    mel = torch.from_numpy(np.stack([eng.pcm_to_mel(c) for c in clips])).cuda()   # [B][M][n_len]
    pcm = torch.from_numpy(clips).cuda()
    out = {w: torch.empty((B,) + eng.out_shape, dtype=torch.float32, device="cuda") for w in ("pcm", "mel")}
    ns, nl = [bench.N_SAMPLES] * B, [n_len] * B
    kl = [250] * B
    cases = {
        "plain": {"pcm": lambda: eng.encode_device(pcm.data_ptr(), bench.N_SAMPLES, ns, out["pcm"].data_ptr()),
                  "mel": lambda: eng.encode_device_mel(mel.data_ptr(), M * n_len, n_len, nl, out["mel"].data_ptr())},
        "varlen_250": {"pcm": lambda: eng.encode_device_varlen(pcm.data_ptr(), bench.N_SAMPLES, ns, out["pcm"].data_ptr(), key_len=kl),
                       "mel": lambda: eng.encode_device_mel(mel.data_ptr(), M * n_len, n_len, nl, out["mel"].data_ptr(),
                                                            kind=q2a.ENCODE_VARLEN, key_len=kl)},
    }
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
    for name, entry in cases.items():   # warm-up, untimed; the two inputs give the same bytes
        for call in entry.values():
            call()
        torch.cuda.synchronize()
        same[name] = bool(torch.equal(out["pcm"].view(torch.int32), out["mel"].view(torch.int32)))
    wall = {name: {"pcm": [], "mel": []} for name in cases}
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
    eng.close()

    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    res = {"clips": B, "wt": args.wt, "steps_per_measurement": args.steps, "rounds": args.rounds, "cases": {}}
    for name in cases:
        res["cases"][name] = {
            "same_bytes": same[name],
            "wall_ms_per_step": {w: [round(x, 2) for x in v] for w, v in wall[name].items()},
            "median_ms": {w: round(med(v), 2) for w, v in wall[name].items()},
            "spread_ms": {w: round(max(v) - min(v), 2) for w, v in wall[name].items()},
            "class_ms_per_step": classes[name],
            "outside_mel_ms": {w: round(sum(v for c, v in classes[name][w].items() if c != "mel"), 3) for w in ("pcm", "mel")}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
