#!/usr/bin/env python3
"""Whole-step time of q2a_audio_features_device_to against today's composition.

    python diag/features_to_time.py [--clips 64] [--wt q4_k] [--rounds 4] [--steps 3] [--out FILE]

Full-size model with a 1280 -> 4096 projector of the same weight type, `--clips` 30 s clips resident in HBM as PCM, at
key lengths 250 and 1500. The destination is a bf16 [rows][4096] buffer standing for inputs_embeds: clip c's rows lie
behind 40 text rows each (rows = N_tot + 40 * clips + 40). Per case two calls that must give the same bytes (checked,
whole buffer):
  composed  audio_features_device into f32 [N_tot][4096], feat.to(torch.bfloat16), index_copy_ into the buffer (the index
            tensor is built once, outside the timed region)
  fused     audio_features_device_to with clip_rows, straight into the buffer
One process, alternating runs: every round measures, per case, the composition and then the new call, `--steps` calls
each between two synchronisations, profiling off: wall ms per step. Medians over the rounds and the spread (max - min)
of either call per case. Prints one JSON line (and writes it to --out)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench  # noqa: E402  (model generator, clip generator, package path)
from features_time import D_OUT, make_projector  # noqa: E402

TEXT_ROWS = 40


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
    pr = q2a.Projector(make_projector(args.wt, args.workdir), device=0)
    B = args.clips
    eng.reserve(B)
    pcm = torch.from_numpy(bench.synth_clips(0, B)).cuda()
    ns = [bench.N_SAMPLES] * B

    cases, bufs = {}, {}
    for L in (250, 1500):
        kl = [L] * B
        n_tot, out_start = q2a.packed_out_rows(kl)
        clip_rows = [int(out_start[c]) + TEXT_ROWS * (c + 1) for c in range(B)]
        n_rows = n_tot + TEXT_ROWS * (B + 1)
        _, row_map = q2a.feat_rows([L // 2] * B, clip_rows, n_rows)
        index = torch.from_numpy(row_map.astype(np.int64)).cuda()
        feat = torch.empty((n_tot, D_OUT), dtype=torch.float32, device="cuda")
        dst_c = torch.zeros((n_rows, D_OUT), dtype=torch.bfloat16, device="cuda")
        dst_f = torch.zeros((n_rows, D_OUT), dtype=torch.bfloat16, device="cuda")
        fd = q2a.feat_dst(dst_f.data_ptr(), D_OUT, n_rows, q2a.DT_BF16)

        def composed(kl=kl, n_tot=n_tot, feat=feat, dst=dst_c, index=index):
            eng.audio_features_device(pcm.data_ptr(), bench.N_SAMPLES, ns, feat.data_ptr(), 0, n_tot, projector=pr, key_len=kl)
            dst.index_copy_(0, index, feat.to(torch.bfloat16))

        def fused(kl=kl, fd=fd, clip_rows=clip_rows):
            eng.audio_features_device_to(pcm.data_ptr(), bench.N_SAMPLES, ns, fd, pr, clip_rows=clip_rows, key_len=kl)

        cases[f"key_len_{L}"] = {"composed": composed, "fused": fused}
        bufs[f"key_len_{L}"] = (dst_c, dst_f, n_tot, n_rows)

    def steps(call):
        for _ in range(args.steps):
            call()
        torch.cuda.synchronize()

    same = {}
    for name, entry in cases.items():   # warm-up, untimed; the two calls give the same bytes
        for call in entry.values():
            call()
        torch.cuda.synchronize()
        a, b = bufs[name][:2]
        same[name] = bool(torch.equal(a.view(torch.int16), b.view(torch.int16)) and bool((a != 0).any()))
    wall = {name: {"composed": [], "fused": []} for name in cases}
    for _ in range(args.rounds):
        for name, entry in cases.items():
            for which, call in entry.items():
                t0 = time.perf_counter()
                steps(call)
                wall[name][which].append((time.perf_counter() - t0) * 1e3 / args.steps)
    pr.close()
    eng.close()

    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    res = {"clips": B, "wt": args.wt, "projector": [1280, D_OUT], "dst": "bfloat16", "text_rows_between_clips": TEXT_ROWS,
           "steps_per_measurement": args.steps, "rounds": args.rounds, "cases": {}}
    for name in cases:
        res["cases"][name] = {
            "n_tot": bufs[name][2], "dst_rows": bufs[name][3], "same_bytes": same[name],
            "wall_ms_per_step": {w: [round(x, 2) for x in v] for w, v in wall[name].items()},
            "median_ms": {w: round(med(v), 2) for w, v in wall[name].items()},
            "spread_ms": {w: round(max(v) - min(v), 2) for w, v in wall[name].items()}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
