#!/usr/bin/env python3
"""Attention time per step against the per-clip key length (the k_attn_t row).

    python diag/attn_keylen_time.py [--clips 64] [--wt q4_k] [--rounds 4] [--steps 3] [--out FILE]

Full-size model, `--clips` 30 s clips resident in HBM. One process, alternating runs: every round measures, in this
order, the unmasked encode (q2a_encode_device), the padded encode (q2a_encode_device_padded) with every key length
1500, 500 and 250, and the unmasked encode again. The figure is the engine's own per-class timer (q2a_profile_*,
Q2A_PROF_ATTN only: HIP events around the attention launches) in ms per step. The two unmasked measurements of every
round give the run's own spread, the margin for the full-length cost of the key-length instantiation.
Prints one JSON line (and writes it to --out)."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (model generator, clip generator, package path)

PROF_ATTN = 5


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
    import torch
    import q2a

    os.makedirs(args.workdir, exist_ok=True)
    model = bench.make_model(args.wt, args.workdir, min(16, os.cpu_count() or 8))
    eng = q2a.Engine(model, device=0)
    B = args.clips
    eng.reserve(B)
    pcm = torch.from_numpy(bench.synth_clips(0, B)).cuda()
    out = torch.empty((B,) + eng.out_shape, dtype=torch.float32, device="cuda")
    ns = [bench.N_SAMPLES] * B
    lens = [int(x) for x in args.lens.split(",")]
    lib = q2a.lib()
    lib.q2a_profile_enable_mask.argtypes = [C.c_void_p, C.c_uint]
    ms = (C.c_double * 11)()
    cnt = (C.c_int64 * 11)()
    h = C.c_void_p(eng.h)

    def run(key_len):
        if key_len is None:
            eng.encode_device(pcm.data_ptr(), bench.N_SAMPLES, ns, out.data_ptr())
        else:
            eng.encode_device_padded(pcm.data_ptr(), bench.N_SAMPLES, ns, out.data_ptr(), key_len=[key_len] * B)

    def attn_ms(key_len):
        lib.q2a_profile_read(h, ms, cnt, 11, 1)
        for _ in range(args.steps):
            run(key_len)
        torch.cuda.synchronize()
        lib.q2a_profile_read(h, ms, cnt, 11, 1)
        return ms[PROF_ATTN] / args.steps

    for k in [None] + lens:   # warm-up, untimed
        run(k)
    torch.cuda.synchronize()
    lib.q2a_profile_enable_mask(h, 1 << PROF_ATTN)
    order = ["unmasked"] + [f"key_len_{n}" for n in lens] + ["unmasked_again"]
    keys = [None] + lens + [None]
    rows = {name: [] for name in order}
    for _ in range(args.rounds):
        for name, k in zip(order, keys):
            rows[name].append(attn_ms(k))
    lib.q2a_profile_enable_mask(h, 0)
    eng.close()
    un = rows["unmasked"] + rows["unmasked_again"]
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    res = {"clips": B, "wt": args.wt, "steps_per_measurement": args.steps, "rounds": args.rounds,
           "attention_ms_per_step": {k: [round(x, 3) for x in v] for k, v in rows.items()},
           "median_ms": {"unmasked": round(med(un), 3), **{f"key_len_{n}": round(med(rows[f"key_len_{n}"]), 3) for n in lens}},
           "unmasked_spread_ms": round(max(un) - min(un), 3)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
