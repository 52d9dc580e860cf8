#!/usr/bin/env python3
"""A/B of two builds of the ggml backend on the reference's whisper_full: best_encode_s of `HARNESS encode MODEL PCM OUT
10` for one full-size 30 s clip, F16 and Q4_K weights, with HIP graph replay (host cost nil) and with
GGML_Q2A_NO_GRAPH=1 (host node walking in the timed path). The two harness binaries run in fresh processes, alternating
on one box; each pair's embd_enc is compared byte for byte. Stops at the first failing process.

    python diag/backend_harness_ab.py --base OTHER/ggml_q2a_harness --new oracle/_ref/ggml_q2a_harness --out ab.json

--order: ab (base first in every pair), ba, or abba (alternating pair by pair)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "qwen2-audio-whisper-ggml_amd", "bin", "q2a_tool")
COUNTERS = ("nodes", "fused", "mul_mat_fast", "mm_grouped", "attn_fused", "other", "graph_replayed", "repack_lazy")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", required=True)
    ap.add_argument("--new", default=os.path.join(ROOT, "oracle", "_ref", "ggml_q2a_harness"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--order", default="ab", choices=("ab", "ba", "abba"))
    ap.add_argument("--out", default="backend_harness_ab.json")
    a = ap.parse_args()
    binary = {"base": a.base, "new": a.new}
    tmp = tempfile.mkdtemp(prefix="q2a_ab_")
    f16, q4k, clip = (os.path.join(tmp, n) for n in ("full-f16.bin", "full-q4_k.bin", "clip0.f32"))
    subprocess.check_call([TOOL, "gen-model", f16, "full", "f16", "0x51A2", "16"], timeout=600)
    subprocess.check_call([TOOL, "quantize", f16, q4k, "q4_k", "16"], timeout=600)
    subprocess.check_call([TOOL, "synth-clip", clip, "480000", "0"], timeout=120)
    runs = []
    for wt, model in (("f16", f16), ("q4_k", q4k)):
        for mode in ("graph", "nograph"):
            env = dict(os.environ)
            if mode == "nograph":
                env["GGML_Q2A_NO_GRAPH"] = "1"
            for rep in range(1, a.reps + 1):
                base_first = a.order == "ab" or (a.order == "abba" and rep % 2 == 1)
                outs = {}
                for variant in (("base", "new") if base_first else ("new", "base")):
                    out = os.path.join(tmp, f"embd_{variant}.f32")
                    r = subprocess.run([binary[variant], "encode", model, clip, out, "10"], capture_output=True, text=True,
                                       timeout=300, env=env)
                    if r.returncode != 0:
                        print(f"FAILED {variant} {wt} {mode} rep {rep}: rc {r.returncode}\n{r.stderr[-2000:]}", flush=True)
                        return 1
                    info = json.loads(r.stdout.strip().splitlines()[-1])
                    with open(out, "rb") as f:
                        outs[variant] = f.read()
                    row = {"weights": wt, "mode": mode, "variant": variant, "rep": rep,
                           "best_encode_ms": round(info["best_encode_s"] * 1e3, 4)}
                    row.update({k: info[k] for k in COUNTERS})
                    runs.append(row)
                    print(json.dumps(row), flush=True)
                runs[-1]["embd_equals_other"] = outs["base"] == outs["new"]
                print(f"  embd_enc byte-identical: {runs[-1]['embd_equals_other']}", flush=True)
    cells = {}
    for wt in ("f16", "q4_k"):
        for mode in ("graph", "nograph"):
            v = {k: [r["best_encode_ms"] for r in runs if (r["weights"], r["mode"], r["variant"]) == (wt, mode, k)]
                 for k in ("base", "new")}
            lo, hi, mean = min(v["base"]), max(v["base"]), sum(v["new"]) / len(v["new"])
            cells[f"{wt}/{mode}"] = {"base_ms": v["base"], "new_ms": v["new"], "base_min": lo, "base_max": hi,
                                     "base_mean": round(sum(v["base"]) / len(v["base"]), 4), "new_mean": round(mean, 4),
                                     "new_mean_within_base_spread": lo <= mean <= hi}
    with open(a.out, "w") as f:
        json.dump({"order": a.order, "cells": cells, "runs": runs}, f, indent=1)
    print(json.dumps(cells, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
