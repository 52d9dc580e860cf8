#!/usr/bin/env python3
"""The decoding gather from a quantized embedding table against the dense-table byte copy.

    python diag/embed_q_time.py [--rows 60000] [--vocab 156032] [--rounds 5] [--reps 100] [--out FILE]

`--rows` text ids drawn uniformly from a table of `--vocab` rows x 4096 columns, no audio id among them. Per destination
dtype (bf16, f32) four ways to fill the same destination bytes:
  dense           q2a_test_embed_gather (k_embed_gather) from a dense table of the destination's dtype
  q4_k/q6_k/q8_0  q2a_test_embed_gather_q from a table of that block type
The quantized tables are 512 distinct rows (the host quantizers on a seeded draw) repeated to --vocab rows, so a table
has its real footprint; the dense table holds the Q4_K table's values. Each quantized result is checked, whole buffer,
against q2a.dequantize_row of its rows cast by torch on the CPU. One process, alternating: every round times each of
the eight between two device events over --reps launches (each launch includes the hook's 16-byte report memset). Medians
over the rounds, spreads (max - min), the bytes each way reads and writes, and every table's HBM footprint. Prints one
JSON line (and writes it to --out); hold it against diag/bwbench.hip's uint4 copy figure on the same box."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen2-audio-whisper-ggml_amd"))

N_COLS, DISTINCT = 4096, 512
TYPES = {"q4_k": (12, "q2a_quantize_row_q4_K"), "q6_k": (14, "q2a_quantize_row_q6_K"), "q8_0": (8, "q2a_quantize_row_q8_0")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=60000)
    ap.add_argument("--vocab", type=int, default=156032)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import q2a

    rng = np.random.default_rng(5)
    x = rng.standard_normal((DISTINCT, N_COLS)).astype(np.float32)
    tables, values = {}, {}
    for name, (t, fn_name) in TYPES.items():
        fn = getattr(q2a._host(), fn_name)
        fn.argtypes, fn.restype = [C.c_void_p, C.c_void_p, C.c_int64], None
        raw = np.zeros((DISTINCT, q2a.quant_row_size(t, N_COLS)), dtype=np.uint8)
        for i in range(DISTINCT):
            fn(x[i].ctypes.data_as(C.c_void_p), raw[i].ctypes.data_as(C.c_void_p), N_COLS)
        values[name] = torch.from_numpy(np.stack([q2a.dequantize_row(t, r, N_COLS) for r in raw]))
        reps = (args.vocab + DISTINCT - 1) // DISTINCT
        tables[name] = q2a.QuantTable(torch.from_numpy(raw).cuda().repeat(reps, 1)[:args.vocab].contiguous(), t, N_COLS)
    ids = rng.integers(0, args.vocab, size=args.rows).astype(np.int64)
    ids_dev = torch.from_numpy(ids).cuda()
    report = torch.zeros(4, dtype=torch.int32, device="cuda")
    src_q = q2a.embeds_src(ids_dev.data_ptr(), 8, args.rows, -1, report_ptr=report.data_ptr())

    calls, info, keep = {}, {}, []
    for dt_name, dtype, dt in (("bf16", torch.bfloat16, q2a.DT_BF16), ("f32", torch.float32, q2a.DT_F32)):
        es = 2 if dtype == torch.bfloat16 else 4
        reps = (args.vocab + DISTINCT - 1) // DISTINCT
        dense = values["q4_k"].to(dtype).cuda().repeat(reps, 1)[:args.vocab].contiguous()
        out = torch.zeros((args.rows, N_COLS), dtype=dtype, device="cuda")
        dst = q2a.feat_dst(out.data_ptr(), N_COLS, args.rows, dt)
        src_d = q2a.embeds_src(ids_dev.data_ptr(), 8, args.rows, -1, dense.data_ptr(), args.vocab, N_COLS, report.data_ptr())
        keep += [dense, out, dst, src_d]
        written = float(args.rows) * N_COLS * es
        calls[f"{dt_name}/dense"] = lambda s=src_d, d=dst: q2a.test_embed_gather(s, d, N_COLS)
        info[f"{dt_name}/dense"] = dict(read_bytes=written, written_bytes=written, table_bytes=float(args.vocab) * N_COLS * es)
        same = {}
        for name, qt in tables.items():
            calls[f"{dt_name}/{name}"] = lambda q=qt, d=dst: q2a.test_embed_gather_q(src_q, q, d, N_COLS)
            info[f"{dt_name}/{name}"] = dict(read_bytes=float(args.rows) * q2a.quant_row_size(qt.ggml_type, N_COLS), written_bytes=written,
                                             table_bytes=float(qt.vocab) * qt.row_bytes)
            out.zero_()
            calls[f"{dt_name}/{name}"]()   # warm-up, and the check
            torch.cuda.synchronize()
            want = values[name].to(dtype)[torch.from_numpy(ids % DISTINCT)]
            iv = torch.int16 if es == 2 else torch.int32
            same[name] = bool(torch.equal(out.cpu().view(iv), want.view(iv))) and report.cpu().tolist() == [0, 0, 0, 0]
            info[f"{dt_name}/{name}"]["equals_dequantize_row"] = same[name]
        calls[f"{dt_name}/dense"]()
        torch.cuda.synchronize()

    def timed(call):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            call()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / args.reps

    us = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, call in calls.items():
            us[k].append(timed(call))
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    res = {"rows": args.rows, "n_cols": N_COLS, "vocab": args.vocab, "rounds": args.rounds, "launches_per_measurement": args.reps, "cases": {}}
    for k, v in us.items():
        m = med(v)
        res["cases"][k] = dict(info[k], us=[round(t, 1) for t in v], median_us=round(m, 1), spread_us=round(max(v) - min(v), 1),
                               TB_per_s=round((info[k]["read_bytes"] + info[k]["written_bytes"]) / (m * 1e-6) / 1e12, 3))
    for dt_name in ("bf16", "f32"):
        d = res["cases"][f"{dt_name}/dense"]
        for name in TYPES:
            c = res["cases"][f"{dt_name}/{name}"]
            c["over_dense"] = round(c["median_us"] / d["median_us"], 3)
            c["within_margin_of_dense"] = bool(c["median_us"] <= d["median_us"] + max(c["spread_us"], d["spread_us"]))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
