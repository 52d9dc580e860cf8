#!/usr/bin/env python3
"""Whole-step time of Engine.inputs_embeds against today's composition, and the two new kernels alone.

    python diag/inputs_embeds_time.py [--clips 64] [--wt q4_k] [--rounds 4] [--steps 3] [--out FILE]

Full-size model with a 1280 -> 4096 projector of the same weight type, `--clips` clips as log-mel input_features
[clips][128][3000] resident in HBM (four distinct clips, repeated), at key lengths 250 and 1500. inputs_embeds is bf16
[clips][S][4096]; every sequence holds 16 text tokens, its clip's run of audio tokens and 16 more text tokens
(S = key_len / 2 + 32), input_ids is an int64 CUDA tensor, the embedding table bf16 [--vocab][4096]. Per case two ways to
the same bytes (checked, whole buffer):
  composed  input_ids.cpu(), q2a.audio_token_runs, torch.nn.functional.embedding(input_ids, table), then
            Engine.audio_features(out=, clip_rows=) over it
  one_call  Engine.inputs_embeds(..., out=, check=False)
(the feature mask is a host array in both, so neither reads it back). One process, alternating runs: every round
measures, per case, the composition and then the one call, `--steps` calls each between two synchronisations, profiling
off: wall ms per step. Medians over the rounds and the spread (max - min) of either per case. Then, per case, the gather
alone (q2a_test_embed_gather) and the compaction alone (q2a_test_audio_token_rows) between two events, --kernel-reps
launches each: µs per launch, and for the gather the bytes it moves (text rows x 4096 x 2 bytes, read and written) per
second — to be held against diag/bwbench.hip's copy figure on the same box. Prints one JSON line (and writes it to --out)."""
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

TEXT_EACH_SIDE = 16
AUDIO = 151646
MEL_FRAMES = 3000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--wt", default="q4_k")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--vocab", type=int, default=156032)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--workdir", default=os.environ.get("Q2A_BENCH_DIR", os.path.join(tempfile.gettempdir(), "q2a_bench")))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    import q2a

    os.makedirs(args.workdir, exist_ok=True)
    model = bench.make_model(args.wt, args.workdir, min(16, os.cpu_count() or 8))
    eng = q2a.Engine(model, device=0)
    pr = q2a.Projector(make_projector(args.wt, args.workdir), device=0)
    B = args.clips
    eng.reserve(B)
    distinct = [eng.pcm_to_mel(c)[:, :MEL_FRAMES] for c in bench.synth_clips(0, min(4, B))]
    x = torch.from_numpy(np.stack([distinct[c % len(distinct)] for c in range(B)])).cuda()
    table = torch.randn((args.vocab, D_OUT), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)).to(torch.bfloat16)
    rng = np.random.default_rng(2)

    cases, info = {}, {}
    for L in (250, 1500):
        S = L // 2 + 2 * TEXT_EACH_SIDE
        ids = rng.integers(0, AUDIO, size=(B, S)).astype(np.int64)
        ids[:, TEXT_EACH_SIDE:TEXT_EACH_SIDE + L // 2] = AUDIO
        ids_dev = torch.from_numpy(ids).cuda()
        mask = np.zeros((B, MEL_FRAMES), dtype=np.int64)
        mask[:, :2 * L] = 1
        out_c = torch.zeros((B, S, D_OUT), dtype=torch.bfloat16, device="cuda")
        out_f = torch.zeros((B, S, D_OUT), dtype=torch.bfloat16, device="cuda")

        def composed(ids_dev=ids_dev, mask=mask, out=out_c):
            starts, _ = q2a.audio_token_runs(ids_dev.cpu().numpy(), AUDIO)
            out.copy_(F.embedding(ids_dev, table))
            eng.audio_features(x, mask, projector=pr, out=out, clip_rows=starts)

        def composed_in_place(ids_dev=ids_dev, mask=mask):
            # (what a caller without a buffer of its own does: the embedding's result is inputs_embeds)
            starts, _ = q2a.audio_token_runs(ids_dev.cpu().numpy(), AUDIO)
            emb = F.embedding(ids_dev, table)
            eng.audio_features(x, mask, projector=pr, out=emb, clip_rows=starts)
            return emb

        def one_call(ids_dev=ids_dev, mask=mask, out=out_f):
            eng.inputs_embeds(x, mask, ids_dev, AUDIO, pr, embed_tokens=table, out=out, check=False)

        name = f"key_len_{L}"
        cases[name] = {"composed": composed_in_place, "one_call": one_call}
        info[name] = dict(S=S, ids=ids_dev, out_c=out_c, out_f=out_f, check=composed, n_text=B * 2 * TEXT_EACH_SIDE, n_feat=B * (L // 2))

    def steps(call):
        for _ in range(args.steps):
            call()
        torch.cuda.synchronize()

    same = {}
    for name, entry in cases.items():   # warm-up, untimed; the two ways give the same bytes
        info[name]["check"]()
        for call in entry.values():
            call()
        torch.cuda.synchronize()
        a, b = info[name]["out_c"], info[name]["out_f"]
        same[name] = bool(torch.equal(a.view(torch.int16), b.view(torch.int16)) and bool((a != 0).any()))
    wall = {name: {"composed": [], "one_call": []} for name in cases}
    for _ in range(args.rounds):
        for name, entry in cases.items():
            for which, call in entry.items():
                t0 = time.perf_counter()
                steps(call)
                wall[name][which].append((time.perf_counter() - t0) * 1e3 / args.steps)

    # the two kernels alone, between two events
    def timed(call):
        call()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.kernel_reps):
            call()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / args.kernel_reps

    kernels = {}
    report = torch.zeros(4, dtype=torch.int32, device="cuda")
    for name, c in info.items():
        n_tok = B * c["S"]
        dst = q2a.feat_dst(c["out_f"].data_ptr(), D_OUT, n_tok, q2a.DT_BF16)
        src = q2a.embeds_src(c["ids"].data_ptr(), 8, n_tok, AUDIO, table.data_ptr(), args.vocab, D_OUT, report.data_ptr())
        row_map = torch.empty(c["n_feat"], dtype=torch.int32, device="cuda")

        g_us = timed(lambda: q2a.test_embed_gather(src, dst, D_OUT))
        c_us = timed(lambda: pr.test_audio_token_rows(c["ids"].data_ptr(), 8, n_tok, AUDIO, c["n_feat"], row_map.data_ptr(),
                                                      report.data_ptr()))
        moved = 2.0 * c["n_text"] * D_OUT * 2
        kernels[name] = {"tokens": n_tok, "text_rows": c["n_text"], "gather_us": round(g_us, 2), "gather_bytes": moved,
                         "gather_TB_per_s": round(moved / (g_us * 1e-6) / 1e12, 3),
                         "gather_note": "includes the hook's 16-byte report memset", "compaction_us": round(c_us, 2),
                         "compaction_note": "both kernels and the hook's copy of the map"}
    # the gather at a size where launch overhead does not count: 60 000 text rows (983 MB moved, bwbench's copy size)
    n_big = 60000
    ids_big = torch.from_numpy(rng.integers(0, AUDIO, size=n_big).astype(np.int64)).cuda()
    out_big = torch.empty((n_big, D_OUT), dtype=torch.bfloat16, device="cuda")
    src = q2a.embeds_src(ids_big.data_ptr(), 8, n_big, AUDIO, table.data_ptr(), args.vocab, D_OUT, report.data_ptr())
    big_us = timed(lambda: q2a.test_embed_gather(src, q2a.feat_dst(out_big.data_ptr(), D_OUT, n_big, q2a.DT_BF16), D_OUT))
    torch.cuda.synchronize()
    big_ok = bool(torch.equal(out_big.view(torch.int16), table[ids_big].view(torch.int16)))
    moved = 2.0 * n_big * D_OUT * 2
    gather_big = {"text_rows": n_big, "us": round(big_us, 2), "bytes": moved, "TB_per_s": round(moved / (big_us * 1e-6) / 1e12, 3),
                  "equals_table_rows": big_ok}
    pr.close()
    eng.close()

    med =lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    res = {"clips": B, "wt": args.wt, "projector": [1280, D_OUT], "dst": "bfloat16", "vocab": args.vocab,
           "text_tokens_per_sequence": 2 * TEXT_EACH_SIDE, "steps_per_measurement": args.steps, "rounds": args.rounds, "gather_60000_text_rows": gather_big,
           "cases": {}}
    for name in cases:
        res["cases"][name] = {
            "tokens_per_sequence": info[name]["S"], "n_feat": info[name]["n_feat"], "same_bytes": same[name],
            "wall_ms_per_step": {w: [round(v_, 2) for v_ in v] for w, v in wall[name].items()},
            "median_ms": {w: round(med(v), 2) for w, v in wall[name].items()},
            "spread_ms": {w: round(max(v) - min(v), 2) for w, v in wall[name].items()},
            "kernels": kernels[name]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
