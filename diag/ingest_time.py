#!/usr/bin/env python3
"""Time of the native-rate ingestion (q2a_ingest_device / _host) next to what it replaces.

    python diag/ingest_time.py [--clips 64] [--seconds 30] [--rounds 5] [--steps 10] [--cpu-clips 8] [--out FILE]

Two cases, `--clips` clips of `--seconds` s resident in HBM: 48 kHz s16 stereo and 44.1 kHz s16 mono. One process,
alternating rounds: every round times, per case, `--steps` ingests between two synchronisations (wall ms per ingest),
and a device-to-device copy of a buffer of the ingest's bytes (read + written) the same way, so the ingest's bytes over
its time stand next to the box's copy bandwidth measured in the same minutes. Medians over the rounds and the spread
(max - min). Then, per case:
  cpu       `--cpu-clips` of the clips through scipy.signal.resample_poly on 16 threads (where scipy imports; else the
            float64 restatement with a precomputed bank is named and skipped), scaled to `--clips`
  host      q2a_ingest_host of all clips (PCIe both ways), once warm, median of 3
The ingest does not depend on the model: the engine is opened on the tiny synthetic model. The encode step it precedes
is bench.py's. Prints one JSON line (and writes it to --out)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen2-audio-whisper-ggml_amd"))

CASES = [("48k_s16_stereo", 48000, 2), ("44k1_s16_mono", 44100, 1)]


def med_spread(xs):
    return {"median": statistics.median(xs), "spread": max(xs) - min(xs), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--cpu-clips", type=int, default=8)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import q2a
    tmp = tempfile.mkdtemp(prefix="q2a_ingest_")
    model = os.path.join(tmp, "tiny-f16.bin")
    subprocess.check_call([q2a.TOOL_PATH, "gen-model", model, "tiny", "f16", "0x51A2", "8"])
    eng = q2a.Engine(model, device=0)
    rng = np.random.default_rng(7)
    cases = {}
    for name, rate, ch in CASES:
        n = int(rate * a.seconds)
        host = [rng.integers(-16384, 16384, (n, ch) if ch > 1 else n, dtype=np.int16) for _ in range(a.clips)]
        dev = [torch.from_numpy(h).cuda() for h in host]
        n_out = q2a.resampled_length(n, rate)
        out = torch.zeros((a.clips, n_out), dtype=torch.float32, device="cuda")
        nbytes = a.clips * (n * ch * 2 + n_out * 4)
        copy_src = torch.zeros(nbytes // 2, dtype=torch.uint8, device="cuda")   # a copy reads and writes its size
        copy_dst = torch.empty_like(copy_src)
        cases[name] = dict(rate=rate, ch=ch, host=host, dev=dev, out=out, nbytes=nbytes, src=copy_src, dst=copy_dst, ms=[], copy_ms=[])
        eng.ingest(dev, [rate] * a.clips, out=out)   # warm: bank, code object
        copy_dst.copy_(copy_src)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for c in cases.values():
            rates = [c["rate"]] * a.clips
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(a.steps):
                eng.ingest(c["dev"], rates, out=c["out"])
            torch.cuda.synchronize()
            c["ms"].append((time.perf_counter() - t) * 1e3 / a.steps)
            t = time.perf_counter()
            for _ in range(a.steps):
                c["dst"].copy_(c["src"])
            torch.cuda.synchronize()
            c["copy_ms"].append((time.perf_counter() - t) * 1e3 / a.steps)
    res = {"clips": a.clips, "seconds": a.seconds, "rounds": a.rounds, "steps": a.steps, "cases": {}}
    try:
        from scipy.signal import resample_poly
    except ImportError:
        resample_poly = None
    for name, c in cases.items():
        r = {"ingest_ms": med_spread(c["ms"]), "copy_same_bytes_ms": med_spread(c["copy_ms"]), "bytes": c["nbytes"]}
        r["ingest_GBps"] = c["nbytes"] / r["ingest_ms"]["median"] / 1e6
        r["copy_GBps"] = c["nbytes"] / r["copy_same_bytes_ms"]["median"] / 1e6
        r["fraction_of_copy_bandwidth"] = r["ingest_GBps"] / r["copy_GBps"]
        L, M = 16000 // np.gcd(16000, c["rate"]), c["rate"] // np.gcd(16000, c["rate"])
        if resample_poly is not None:
            def one(h):
                x = h.astype(np.float32) / 32768 if h.ndim == 1 else (h[:, 0].astype(np.float32) + h[:, 1]) / 65536
                return resample_poly(x, int(L), int(M))
            sub = c["host"][:a.cpu_clips]
            ts = []
            for _ in range(3):
                t = time.perf_counter()
                with ThreadPoolExecutor(16) as ex:
                    list(ex.map(one, sub))
                ts.append((time.perf_counter() - t) * 1e3 * a.clips / len(sub))
            r["cpu_scipy_resample_poly_16_threads_ms_scaled"] = med_spread(ts)
        else:
            r["cpu"] = "scipy does not import here; not measured"
        ts = []
        for _ in range(4):
            t = time.perf_counter()
            eng.ingest_host(c["host"], [c["rate"]] * a.clips)
            ts.append((time.perf_counter() - t) * 1e3)
        r["ingest_host_ms"] = med_spread(ts[1:])
        res["cases"][name] = r
    eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
