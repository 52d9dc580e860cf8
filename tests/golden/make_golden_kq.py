"""Fixtures for Q5_K / Q6_K model files: tests/golden/golden_kq.json + golden_kq*.npz (data only).

Runs only where the reference is compiled (`make -C oracle ref ref-isa ref-clang`, oracle/_ref*/ref_harness). Inputs
come from bin/q2a_tool (the generator and clip bytes of every other fixture, SHA-256 checked against golden.json) and
tests/kquant_cases.py (the hand-made "ext" rows). Everything quantized here is quantized BY THE REFERENCE
(`ref_harness quantize-model IN OUT 13|14`) unless said otherwise; no model file is committed, only hashes.

golden_kq.json
  models      SHA-256 of tiny-q5_k / tiny-q6_k, of the hand-made tinyext-f16 input and of tinyext-q5_k / tinyext-q6_k
              (reference-quantized), and of full-q5_k / full-q6_k (quantized by bin/q2a_tool on its threads — the
              reference's flow is single-threaded; the tool's bytes equal the reference's on the two tiny files)
  clips       SHA-256 of every generated clip
  parent_blobs  SHA-256 of the packed F16 and Q4_K tiny blobs (device layout, compact, bf16) as the commit before
              this fixture packed them: the existing types' blob bytes must not move
  tiny_<wt>, tiny_<wt>_clip<c>   per pair of reference builds: max_rel, rel_l2, rows_max_rel, rows_rel_l2
              (make_crossbuild.py's statistics), clips 0 and 101..104, all eight builds
  <wt>, <wt>_clip<c>             full size (L = 32, D = 1280), clips 0, 101, 102: pair_stats of make_crossbuild.py on the
              golden's 8 192 sampled indices (full_q4_k_c0_idx). Builds: --full-builds (default the builds of
              crossbuild.json's full-size entries but the scalar x86-64 one, which takes ten times as long per
              encode; a build more can only widen a bar, so leaving it out makes the test stricter, not looser)
golden_kq_tiny_<wt>.npz
  tiny_<wt>_c<c>_rows   the golden (AVX2) build's output on rows_stride5
golden_kq.npz
  full_<wt>_c<c>_val    the golden build's full-size output on full_idx
  full_idx              = golden.npz full_q4_k_c0_idx
  ext_<wt>_<i>          the reference's quantized bytes of the hand-made rows of kquant_cases.EXT_TENSORS[i]

usage: python tests/golden/make_golden_kq.py [--workdir DIR] [--threads N] [--skip-full] [--full-builds a,b,c]
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PKG = os.path.join(ROOT, "qwen2-audio-whisper-ggml_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import kquant_cases as kc  # noqa: E402
from make_crossbuild import BUILDS, pair_stats, relerr, sha  # noqa: E402
from q2a import ggmlfile  # noqa: E402

TOOL = os.path.join(PKG, "bin", "q2a_tool")
TINY_CLIPS = [0, 101, 102, 103, 104]
FULL_CLIPS = [0, 101, 102]
TYPES = ["q5_k", "q6_k"]
# q2a.pack_model of tiny-f16 / tiny-q4_k, recorded on the commit before Q5_K / Q6_K support (it cannot be regenerated
# from a later one): "<wt>" device layout, "<wt>_compact" transport form, "<wt>_bf16" the bf16 contract's layout
PARENT_BLOBS = {
    "f16": "dbe4a6b10d3c6b587c949ce119227770ae340916b76fabd2dcc773b5296dd072",
    "f16_compact": "9e0e7c8b9aac332f308b5bedc3898ab042b8b80106abfc49eb6118ec0d2c687c",
    "f16_bf16": "4499e0be750925c0f76c576b71d76c5d455fc8b3214d1cfc79a0a93d4280d54e",
    "q4_k": "1373fe695c03f2d18514c9e1222f087dd24acfa21eb909a567126acf35f995f1",
    "q4_k_compact": "61cd505764e3dd695bcc2406173f1534941d4698d89e3dbcd17fbdb0fb40fc15",
    "q4_k_bf16": "eb80a8f201279a02cbe486f2fe202ea17994e51acf2561814372c9c07c5d3648",
}


def ref_exe(build):
    return os.path.join(ROOT, "oracle", BUILDS[build], "ref_harness")


def ref_quantize(src, dst, wt):
    subprocess.run([ref_exe("avx2"), "quantize-model", src, dst, str(kc.WT_FTYPE[wt])], check=True, capture_output=True)


def ref_encode(build, model, clip, out, threads):
    if os.path.exists(out) and os.path.getmtime(out) >= os.path.getmtime(model):   # an earlier run's output, same model file
        return np.fromfile(out, dtype=np.float32)
    subprocess.run([ref_exe(build), "encode", model, clip, out, str(threads), "1"], check=True, capture_output=True)
    return np.fromfile(out, dtype=np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workdir", default="/tmp/q2a_golden_kq")
    ap.add_argument("--threads", type=int, default=os.cpu_count() or 8)
    ap.add_argument("--skip-full", action="store_true", help="keep the full-size entries of an existing fixture")
    ap.add_argument("--full-builds", default="avx2,avx512,avx2-fma,clang-avx2,clang-avx512,sse42")
    args = ap.parse_args()
    os.makedirs(args.workdir, exist_ok=True)
    W = lambda n: os.path.join(args.workdir, n)  # noqa: E731
    with open(os.path.join(HERE, "golden.json")) as f:
        gmeta = json.load(f)
    gold = dict(np.load(os.path.join(HERE, "golden.npz"), allow_pickle=False))
    jpath = os.path.join(HERE, "golden_kq.json")
    meta = json.load(open(jpath)) if os.path.exists(jpath) else {}
    store = {}
    for f in sorted(glob.glob(os.path.join(HERE, "golden_kq*.npz"))):
        store.update(np.load(f, allow_pickle=False))
    meta["about"] = ("Q5_K / Q6_K fixtures: reference-quantized tiny models, the reference's outputs and its own "
                     "cross-build disagreement (tests/golden/make_golden_kq.py)")
    meta.setdefault("models", {})
    meta.setdefault("clips", {})
    meta["parent_blobs"] = PARENT_BLOBS

    def save():
        with open(jpath, "w") as f:
            json.dump(meta, f, indent=1, sort_keys=True)
        for name in {kc.kq_npz_name(k) for k in store}:   # (no committed file above 1 MiB: one file per tiny type)
            np.savez_compressed(os.path.join(HERE, name), **{k: v for k, v in store.items() if kc.kq_npz_name(k) == name})

    clips = {}
    for c in sorted(set(TINY_CLIPS + FULL_CLIPS)):
        clips[c] = W(f"clip{c}.f32")
        if not os.path.exists(clips[c]):
            subprocess.check_call([TOOL, "synth-clip", clips[c], "480000", str(c)])
        meta["clips"][str(c)] = {"n_samples": 480000, "sha256": sha(clips[c])}
    assert meta["clips"]["0"]["sha256"] == gmeta["clips"]["0"]["sha256"]

    # ---- tiny models, reference-quantized; the hand-made ext model
    base = W("tiny-f16.bin")
    if not os.path.exists(base):
        subprocess.check_call([TOOL, "gen-model", base, "tiny", "f16", "0x51A2", str(args.threads)])
    assert sha(base) == gmeta["models"]["tiny-f16"]["sha256"]
    ext = W("tinyext-f16.bin")
    kc.write_ext_model(base, ext)
    meta["models"]["tinyext-f16"] = {"sha256": sha(ext)}
    rows = gold["rows_stride5"]
    for wt in TYPES:
        model, extq = W(f"tiny-{wt}.bin"), W(f"tinyext-{wt}.bin")
        ref_quantize(base, model, wt)
        ref_quantize(ext, extq, wt)
        meta["models"][f"tiny-{wt}"] = {"sha256": sha(model)}
        meta["models"][f"tinyext-{wt}"] = {"sha256": sha(extq)}
        mf = ggmlfile.read(extq)
        for i, name in enumerate(kc.EXT_TENSORS):
            t = mf.t(name)
            rs = ggmlfile.row_size(t.type, t.ne[0])
            store[f"ext_{wt}_{i}"] = np.array(t.data[:kc.EXT_ROWS * rs])
        for c in TINY_CLIPS:
            finals = {b: ref_encode(b, model, clips[c], W(f"tiny-{wt}-{b}-c{c}.out"), args.threads).reshape(750, -1)
                      for b in BUILDS}
            names = list(finals)
            ent = {"pairs": {}}
            for i, a in enumerate(names):
                for d in names[i + 1:]:
                    mx, l2 = relerr(finals[d], finals[a])
                    rmx, rl2 = relerr(finals[d][rows], finals[a][rows])
                    ent["pairs"][f"{a}_vs_{d}"] = {"max_rel": mx, "rel_l2": l2, "rows_max_rel": rmx, "rows_rel_l2": rl2}
            meta[f"tiny_{wt}" if c == 0 else f"tiny_{wt}_clip{c}"] = ent
            store[f"tiny_{wt}_c{c}_rows"] = finals["avx2"][rows]
            print("tiny", wt, c, max(p["rows_rel_l2"] for p in ent["pairs"].values()), flush=True)
        save()

    # ---- full size
    if not args.skip_full:
        fbase = W("full-f16.bin")
        if not os.path.exists(fbase):
            subprocess.check_call([TOOL, "gen-model", fbase, "full", "f16", "0x51A2", str(args.threads)])
        assert sha(fbase) == gmeta["models"]["full-f16"]["sha256"]
        idx = gold["full_q4_k_c0_idx"]
        store["full_idx"] = idx
        builds = args.full_builds.split(",")
        assert builds[0] == "avx2"
        for wt in TYPES:
            model = W(f"full-{wt}.bin")
            if not os.path.exists(model):
                subprocess.check_call([TOOL, "quantize", fbase, model, wt, str(args.threads)])
            meta["models"][f"full-{wt}"] = {"sha256": sha(model), "quantized_by": "bin/q2a_tool"}
            for c in FULL_CLIPS:
                finals = {}
                for b in builds:
                    t0 = time.time()
                    finals[b] = ref_encode(b, model, clips[c], W(f"full-{wt}-{b}-c{c}.out"), args.threads)
                    print("full", wt, c, b, f"{time.time() - t0:.1f} s", flush=True)
                names = list(finals)
                meta[wt if c == 0 else f"{wt}_clip{c}"] = {
                    "pairs": {f"{a}_vs_{d}": pair_stats(finals[d], finals[a], idx)
                              for i, a in enumerate(names) for d in names[i + 1:]}}
                store[f"full_{wt}_c{c}_val"] = finals["avx2"].reshape(-1)[idx]
                save()
    save()
    print("wrote", jpath)


if __name__ == "__main__":
    main()
