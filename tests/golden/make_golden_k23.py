"""Fixtures for Q2_K / Q3_K model files: tests/golden/golden_k23.json + golden_k23*.npz (data only). Follows
make_golden_kq.py (same builds, clips, statistics; runs only where the reference is compiled): everything is quantized
BY THE REFERENCE (`ref_harness quantize-model IN OUT 10|11`); no model file is committed, only hashes.

golden_k23.json   models: SHA-256 of tiny-<wt> and tinyext-<wt>; tiny_<wt>, tiny_<wt>_clip<c>: per pair of reference
                  builds max_rel, rel_l2, rows_max_rel, rows_rel_l2 (clips 0, 101..104, all eight builds)
golden_k23_tiny_<wt>.npz   tiny_<wt>_c<c>_rows: the golden (AVX2) build's output on rows_stride5
golden_k23.npz    ext_<wt>_<i>: the reference's quantized bytes of the hand-made rows of kquant_cases.EXT_TENSORS[i];
                  extdq_<wt>_<i>: the reference's dequantization of those bytes (dequantize_row_q2_K / _q3_K called from a
                  few lines of C linked against the reference build's ggml objects, oracle/_ref/*.o)

usage: python tests/golden/make_golden_k23.py [--workdir DIR] [--threads N]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_kq as gk  # noqa: E402  (sets sys.path for the package and tests/)
import k23_cases as k23  # noqa: E402
import kquant_cases as kc  # noqa: E402
from make_crossbuild import BUILDS, relerr, sha  # noqa: E402
from q2a import ggmlfile  # noqa: E402


def check_ext_cases(mf, wt):
    """The hand-made rows reach the cases the GPU tests are about (k23_cases' docstring)."""
    v = [mf.t(n).kq() for n in kc.EXT_TENSORS]
    if wt == "q2_k":
        assert any(((p["d"][:6] == 0) & (p["dmin"][:6] != 0)).any() for p in v)
        assert any(((p["q"][:6].reshape(6, -1, 16, 16) == 3) & (p["sc"][:6, :, :, None] == 15)).any() for p in v)
    else:
        assert any((p["d"][:6] < 0).any() for p in v)
        assert any(((p["q"][:6].reshape(6, -1, 16, 16) == 0) & (p["sc"][:6, :, :, None] == 0)).any() for p in v)


DEQ_C = r'''
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
void dequantize_row_q2_K(const void * x, float * y, int64_t k);
void dequantize_row_q3_K(const void * x, float * y, int64_t k);
struct ggml_init_params { size_t mem_size; void * mem_buffer; _Bool no_alloc; };
void * ggml_init(struct ggml_init_params p);   /* fills ggml's fp16 -> f32 table, which the dequantizers read */
int main(int argc, char ** argv) {   /* TYPE IN OUT NBLOCKS */
    const int t = atoi(argv[1]), nb = atoi(argv[4]), bb = t == 10 ? 84 : 110;
    struct ggml_init_params ip = { 1 << 20, 0, 0 };
    ggml_init(ip);
    uint8_t * in = malloc((size_t) nb * bb);
    float * out = malloc((size_t) nb * 256 * 4);
    FILE * f = fopen(argv[2], "rb");
    if (!f || fread(in, bb, nb, f) != (size_t) nb) return 1;
    fclose(f);
    if (t == 10) dequantize_row_q2_K(in, out, (int64_t) nb * 256); else dequantize_row_q3_K(in, out, (int64_t) nb * 256);
    f = fopen(argv[3], "wb");
    return !f || fwrite(out, 4, (size_t) nb * 256, f) != (size_t) nb * 256 || fclose(f);
}
'''


def ref_dequant(workdir, wt, raw):
    """The reference's dequantize_row_* of `raw` (whole blocks), from the AVX2 reference build's objects."""
    exe, src = os.path.join(workdir, "ref_deq"), os.path.join(workdir, "ref_deq.c")
    if not os.path.exists(exe):
        with open(src, "w") as f:
            f.write(DEQ_C)
        ref = os.path.join(gk.ROOT, "oracle", BUILDS["avx2"])
        objs = [os.path.join(ref, o) for o in ("ggml-quants.o", "ggml.o", "ggml-aarch64.o", "ggml-alloc.o", "ggml-backend.o")]
        subprocess.check_call(["g++", "-x", "c", src, "-x", "none", *objs, "-fopenmp", "-lm", "-lpthread", "-o", exe])
    bb = 84 if wt == "q2_k" else 110
    i, o = os.path.join(workdir, "deq.in"), os.path.join(workdir, "deq.out")
    raw.tofile(i)
    subprocess.check_call([exe, str(k23.WT_FTYPE[wt]), i, o, str(raw.size // bb)])
    return np.fromfile(o, dtype=np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workdir", default="/tmp/q2a_golden_k23")
    ap.add_argument("--threads", type=int, default=os.cpu_count() or 8)
    args = ap.parse_args()
    os.makedirs(args.workdir, exist_ok=True)
    W = lambda n: os.path.join(args.workdir, n)  # noqa: E731
    with open(os.path.join(HERE, "golden.json")) as f:
        gmeta = json.load(f)
    rows = np.load(os.path.join(HERE, "golden.npz"), allow_pickle=False)["rows_stride5"]
    meta = {"about": "Q2_K / Q3_K fixtures: reference-quantized tiny models, the reference's outputs and its own "
                     "cross-build disagreement (tests/golden/make_golden_k23.py)", "models": {}}
    store = {}
    clips = {}
    for c in gk.TINY_CLIPS:
        clips[c] = W(f"clip{c}.f32")
        subprocess.check_call([gk.TOOL, "synth-clip", clips[c], "480000", str(c)])
    base, ext = W("tiny-f16.bin"), W("tinyext-f16.bin")
    subprocess.check_call([gk.TOOL, "gen-model", base, "tiny", "f16", "0x51A2", str(args.threads)])
    assert sha(base) == gmeta["models"]["tiny-f16"]["sha256"]
    kc.write_ext_model(base, ext)
    for wt in k23.TYPES:
        model, extq = W(f"tiny-{wt}.bin"), W(f"tinyext-{wt}.bin")
        for src, dst in ((base, model), (ext, extq)):
            subprocess.run([gk.ref_exe("avx2"), "quantize-model", src, dst, str(k23.WT_FTYPE[wt])], check=True, capture_output=True)
        meta["models"][f"tiny-{wt}"] = {"sha256": sha(model)}
        meta["models"][f"tinyext-{wt}"] = {"sha256": sha(extq)}
        mf = ggmlfile.read(extq)
        check_ext_cases(mf, wt)
        for i, name in enumerate(kc.EXT_TENSORS):
            t = mf.t(name)
            store[f"ext_{wt}_{i}"] = np.array(t.data[:kc.EXT_ROWS * ggmlfile.row_size(t.type, t.ne[0])])
            store[f"extdq_{wt}_{i}"] = ref_dequant(args.workdir, wt, store[f"ext_{wt}_{i}"]).reshape(kc.EXT_ROWS, t.ne[0])
        for c in gk.TINY_CLIPS:
            finals = {b: gk.ref_encode(b, model, clips[c], W(f"tiny-{wt}-{b}-c{c}.out"), args.threads).reshape(750, -1)
                      for b in BUILDS}
            names = list(finals)
            pairs = {}
            for i, a in enumerate(names):
                for d in names[i + 1:]:
                    mx, l2 = relerr(finals[d], finals[a])
                    rmx, rl2 = relerr(finals[d][rows], finals[a][rows])
                    pairs[f"{a}_vs_{d}"] = {"max_rel": mx, "rel_l2": l2, "rows_max_rel": rmx, "rows_rel_l2": rl2}
            meta[f"tiny_{wt}" if c == 0 else f"tiny_{wt}_clip{c}"] = {"pairs": pairs}
            store[f"tiny_{wt}_c{c}_rows"] = finals["avx2"][rows]
            print("tiny", wt, c, max(p["rows_rel_l2"] for p in pairs.values()), flush=True)
    with open(os.path.join(HERE, "golden_k23.json"), "w") as f:
        json.dump(meta, f, sort_keys=True)
        f.write("\n")
    name_of = lambda k: next((f"golden_k23_tiny_{wt}.npz" for wt in k23.TYPES if k.startswith(f"tiny_{wt}_")), "golden_k23.npz")  # noqa: E731
    for name in {name_of(k) for k in store}:
        np.savez_compressed(os.path.join(HERE, name), **{k: v for k, v in store.items() if name_of(k) == name})


if __name__ == "__main__":
    main()
