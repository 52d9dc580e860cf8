/*
 * q2a_encoder.h — C ABI of the MI355X-native Qwen2-Audio encoder hot path (libq2a.so, gfx950).
 *
 * This is the drop-in boundary for the reference's hot path: PCM -> log-mel -> Conv1d x2 + GELU -> 32 pre-LN
 * encoder blocks -> AvgPool1d(2) -> LayerNorm, i.e. what `whisper_full()` computes in the reference
 * (src/qwen2-whisper.cpp:2341-2383: whisper_encoder_output_with_state -> whisper_pcm_to_mel_with_state +
 * whisper_encode_qwen2_internal). Plain pointers and sizes only; no torch types.
 *
 * The reference-named API (whisper_init_from_file_with_params / whisper_full / whisper_pcm_to_mel /
 * whisper_print_emb_enc / whisper_free, include/qwen2-whisper.h:141,446,211,527,203) is layered on top of this
 * in include/q2a_whisper.h and exported from the same library.
 *
 * Threading: one q2a_engine per device per host thread (like one whisper_state, include/qwen2-whisper.h:44-45).
 * Errors: functions return 0 / a non-NULL handle on success; negative q2a_status codes otherwise, with a message
 * retrievable through q2a_last_error(). No call aborts the process.
 */
#ifndef Q2A_ENCODER_H
#define Q2A_ENCODER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct q2a_engine q2a_engine;

typedef enum {
    Q2A_OK = 0,
    Q2A_ERR_IO = -1,           /* model file missing / unreadable */
    Q2A_ERR_FORMAT = -2,       /* bad magic, bad tensor shapes, unsupported ftype */
    Q2A_ERR_HIP = -3,          /* HIP runtime error (no device, launch failure, ...) */
    Q2A_ERR_ARG = -4,          /* invalid argument (sizes, NULL pointers, batch too large) */
    Q2A_ERR_OOM = -5,          /* device allocation failed */
    Q2A_ERR_UNSUPPORTED = -6   /* model variant not implemented on this path */
} q2a_status;

/* per-clip result status written by the encode calls */
#define Q2A_CLIP_ENCODED 0
#define Q2A_CLIP_SKIPPED 1   /* < 1 s of audio after the offset: the reference returns 0 without encoding
                                (qwen2-whisper.cpp:2359-2365); the clip's output rows are left untouched */
#define Q2A_CLIP_FAILED 2    /* the call returned an error before this clip's output reached the caller (host API) */

typedef struct {
    int32_t n_audio_ctx, n_audio_state, n_audio_head, n_audio_layer, n_mels;
    int32_t wtype;          /* ggml type of the linear weights: 0 F32, 1 F16, 12 Q4_K, 13 Q5_K, 14 Q6_K, 8 Q8_0, 2 Q4_0 */
    int32_t n_out;          /* output vectors per clip (n_audio_ctx / 2 = 750) */
    int32_t device;
    int64_t weight_bytes;   /* device bytes of the packed weight blob */
    int64_t workspace_bytes;
    int32_t act;            /* Q2A_ACT_REFERENCE or Q2A_ACT_BF16 (from the blob) */
    int32_t reserved;
} q2a_info;

const char * q2a_last_error(void);

/* Load a reference-format ggml model file (models/convert-pt-to-ggml.py layout) onto HIP device `device`. */
q2a_engine * q2a_open(const char * model_path, int device);

/* Activation contract of an engine (q2a_open_ex / q2a_pack_model_ex):
 *   Q2A_ACT_REFERENCE  the reference's own: activations converted per ggml's vec_dot_type before every weight
 *                      GEMM (fp16 / Q8_K / Q8_0, or the exact fp16 hi/lo split for F32 files), F32-class attention
 *   Q2A_ACT_BF16       mixed precision (BASELINE configs[4]): linear weights dequantized (ggml dequantize_row_*) to
 *                      bf16, inter-op activations (LN outputs, Q/K/V, attention probabilities and output, GELU
 *                      output) in bf16, bf16 MFMA with f32 accumulation; the residual stream, LN statistics,
 *                      softmax and the conv front end stay as in the reference contract. A different numerical
 *                      contract from the reference CPU path: its error is reported separately. */
#define Q2A_ACT_REFERENCE 0
#define Q2A_ACT_BF16 1
q2a_engine * q2a_open_ex(const char * model_path, int device, int act);
int64_t q2a_pack_model_ex(const char * model_path, int act, void ** host_blob);

/* Multi-GPU: pack the model into its device layout on the host (rank 0), move the bytes to every rank's device
 * (e.g. one RCCL broadcast over xGMI), then open an engine on the device copy. The blob is self-describing. */
int64_t q2a_pack_model(const char * model_path, void ** host_blob);   /* returns size in bytes, < 0 on error */
void q2a_free_host_blob(void * host_blob);
q2a_engine * q2a_open_device_blob(const void * device_blob, int64_t size, int device);  /* blob not owned */
/* The compact TRANSPORT form of the same blob (what rank 0 broadcasts): the small sections plus every
 * linear weight as the model file's own ggml rows (Q4_K: raw block_q4_K, 144 B per 256 weights, ggml-common.h:282-297)
 * instead of the device layout's expanded operands — 0.37 GB instead of 1.40 GB for the full-size Q4_K model.
 * q2a_open_device_blob accepts it too and expands it on the GPU into an engine-owned device layout that is byte for
 * byte what q2a_pack_model_ex writes on the host. */
int64_t q2a_pack_model_compact(const char * model_path, int act, void ** host_blob);
/* From a blob's first header_bytes (>= 32 KiB) on the host: the device-layout size (return) and the size of the
 * blob as given (*transport_bytes: the compact size for a compact blob). */
int64_t q2a_blob_device_size(const void * host_header, int64_t header_bytes, int64_t * transport_bytes);
/* Expand a compact blob already on device `device` into out_dev (out_bytes >= the device-layout size). */
int q2a_expand_blob(const void * device_blob, int64_t size, void * out_dev, int64_t out_bytes, int device, void * stream);

/* A second engine on the same device sharing `base`'s weights (its own workspace and stream): the analogue of a
 * second whisper_state on one whisper_context. `base` must outlive it. */
q2a_engine * q2a_open_shared(const q2a_engine * base);
/* Encode windows with under 1 s of audio after the offset too (default off: they are skipped, Q2A_CLIP_SKIPPED,
 * like the reference). whisper_full uses it when duration_ms overrides the length check (qwen2-whisper.cpp:2357). */
int q2a_set_force_encode(q2a_engine * e, int on);

void q2a_close(q2a_engine * e);
int q2a_get_info(const q2a_engine * e, q2a_info * info);

/* Reserve device workspace for up to max_clips clips of up to max_samples samples (optional; grown on demand). */
int q2a_reserve(q2a_engine * e, int max_clips, int64_t max_samples);

/* Encode n_clips independent clips whose PCM (16 kHz mono f32) is already in device memory:
 *   pcm_dev    [n_clips][pcm_stride] floats, clip c has n_samples[c] valid samples (host array)
 *   offset_ms  whisper_full_params.offset_ms (window start = offset_ms / 10 mel frames)
 *   out_dev    [n_clips][n_out][n_audio_state] f32 (embd_enc of each clip)
 *   status     host array [n_clips] (Q2A_CLIP_*), may be NULL
 *   stream     hipStream_t to run on, or NULL: the legacy default stream 0 itself (the work starts after everything
 *              queued there before the call, and work queued there afterwards starts after it) — the same rule for
 *              every device-pointer entry point below and q2a_projector_apply. The call is asynchronous w.r.t. the
 *              host except for the small per-batch metadata upload: synchronise (the given stream, or stream 0)
 *              before reading out_dev on the host.
 * Audio longer than 30 s is truncated to one 30 s window, as in the reference (qwen2-whisper.cpp:2366-2372). */
int q2a_encode_device(q2a_engine * e, const float * pcm_dev, int64_t pcm_stride, const int32_t * n_samples,
                      int n_clips, int offset_ms, float * out_dev, int32_t * status, void * stream);

/* Same with host buffers in and out (PCIe transfers included; synchronous). out_host [n_clips][n_out][D]. */
int q2a_encode_host(q2a_engine * e, const float * const * pcm, const int32_t * n_samples, int n_clips,
                    int offset_ms, float * out_host, int32_t * status);

/* Per-clip window offsets (milliseconds, host array [n_clips]) instead of one offset_ms: e.g. the consecutive 30 s
 * windows of a long recording passed as n_clips rows that all point at the same PCM (pcm_stride 0 on the device
 * variant). Each window's log-mel is normalised over the whole recording, exactly as whisper_full(offset_ms = k *
 * 30000) on that recording would (the reference itself only ever encodes the first window). */
int q2a_encode_device_ex(q2a_engine * e, const float * pcm_dev, int64_t pcm_stride, const int32_t * n_samples,
                         const int32_t * offsets_ms, int n_clips, float * out_dev, int32_t * status, void * stream);
int q2a_encode_host_ex(q2a_engine * e, const float * const * pcm, const int32_t * n_samples, const int32_t * offsets_ms,
                       int n_clips, int offset_ms, float * out_host, int32_t * status);

/* ---- clips shorter than 30 s: padding-aware encode ----------------------------------------------------------
 * The entry points above follow the reference: every clip is a full 30 s window and every query attends to all
 * n_audio_ctx keys, padding included (the reference's graph has no mask). Qwen2-Audio itself masks the padded key
 * positions in every encoder layer and keeps only the valid output frames; the entry points below do that.
 *
 * q2a_valid_lengths: the valid encoder positions (enc_len) and output vectors (out_len) of a clip of n_samples samples
 * encoded from offset_ms. Pure host arithmetic (also exported from libq2a_host.so):
 *   n_len_org = 1 + (n_samples - 200) / 160                        (the mel frames the reference computes)
 *   frames    = clamp(n_len_org - offset_ms / 10, 1, 2 * n_audio_ctx)
 *   enc_len   = (frames - 1) / 2 + 1                                (conv2, stride 2)
 *   out_len   = enc_len / 2                                         (AvgPool1d(2))
 * Either output pointer may be NULL. Q2A_ERR_ARG for a negative argument or n_audio_ctx = 0. */
int q2a_valid_lengths(int n_samples, int offset_ms, int n_audio_ctx, int32_t * enc_len, int32_t * out_len);

/* q2a_encode_device_ex with per-clip key lengths: in every encoder block clip c's queries attend to keys
 * 0 .. key_len[c]-1 only (rows past it of K and V are never read).
 *   offsets_ms  host array [n_clips], or NULL (0 for every clip)
 *   key_len     host array [n_clips], 1 <= key_len[c] <= n_audio_ctx (else Q2A_ERR_ARG, before anything is launched),
 *               or NULL: q2a_valid_lengths' enc_len of each clip
 *   out_len     host array [n_clips], may be NULL: key_len[c] / 2 valid output vectors, 0 for a skipped clip
 *   out_dev     [n_clips][n_out][n_audio_state] f32: rows >= out_len[c] of clip c are written as zeros (a skipped
 *               clip's rows are all zeros)
 * Everything else is as in q2a_encode_device_ex (same front end, GEMMs and LayerNorms over all n_audio_ctx rows: the
 * padded rows are computed and ignored). Reference activation contract only: Q2A_ERR_UNSUPPORTED for Q2A_ACT_BF16. */
int q2a_encode_device_padded(q2a_engine * e, const float * pcm_dev, int64_t pcm_stride, const int32_t * n_samples,
                             const int32_t * offsets_ms, const int32_t * key_len, int n_clips, float * out_dev,
                             int32_t * out_len, int32_t * status, void * stream);
/* Same with host buffers in and out (like q2a_encode_host_ex; synchronous). */
int q2a_encode_host_padded(q2a_engine * e, const float * const * pcm, const int32_t * n_samples, const int32_t * offsets_ms,
                           const int32_t * key_len, int n_clips, float * out_host, int32_t * out_len, int32_t * status);

/* ---- variable-length encode: the encoder blocks run on the valid rows only --------------------------------------
 * The padded entry points above still run every GEMM, LayerNorm and quantizer over all n_audio_ctx rows of every clip.
 * The entry points below pack the valid rows of all clips into one [M_tot][n_audio_state] residual stream after the
 * front end (which still runs over full windows), run the n_audio_layer blocks on those M_tot rows, and pool, normalise
 * and scatter them into the same [n_clips][n_out][n_audio_state] output. They return the padded entry points' bytes:
 * rows are independent everywhere but in the attention, every GEMM configuration sums K in the same order, and the
 * attention's 16-query blocks are carried along whole (below).
 *
 * q2a_varlen_rows: the rows clip c occupies in the packed stream, and where they start (host arithmetic; also exported
 * from libq2a_host.so):
 *   seg_rows[c]    = key_len[c] == 0 ? 0 : min(round_up(key_len[c], 16), n_audio_ctx)
 *   row_start[0]   = 0, row_start[c+1] = row_start[c] + seg_rows[c]         (row_start has n_clips + 1 entries)
 * key_len[c] in 0 .. n_audio_ctx (0: a clip that is not encoded). Returns M_tot = row_start[n_clips], < 0
 * (Q2A_ERR_ARG) on error. 16: the attention kernel decides its lazy re-base per block of 16 queries, so the rows
 * between a clip's length and the end of its last partly valid block (the front end's output for the padding, carried
 * through the layers) travel with the clip — at most 15 rows, computed as queries, never read as keys.
 *
 * Not covered: the whisper_* API, q2a_group_*, the ggml backend and the bf16 activation contract
 * (Q2A_ERR_UNSUPPORTED); the front end is not restricted to the valid frames. The output of these entry points is not
 * packed: q2a_audio_features_* below return the valid rows alone, one clip after the other. */
int64_t q2a_varlen_rows(const int32_t * key_len, int n_clips, int n_audio_ctx, int32_t * row_start);

/* q2a_encode_device_padded / q2a_encode_host_padded on the packed rows: the same arguments, checks, out_len, status
 * and output bytes (a batch of skipped clips only: zeros, Q2A_OK, no block is launched). The engine keeps a second
 * residual buffer from the first such call on (counted in q2a_info.workspace_bytes). */
int q2a_encode_device_varlen(q2a_engine * e, const float * pcm_dev, int64_t pcm_stride, const int32_t * n_samples,
                             const int32_t * offsets_ms, const int32_t * key_len, int n_clips, float * out_dev,
                             int32_t * out_len, int32_t * status, void * stream);
int q2a_encode_host_varlen(q2a_engine * e, const float * const * pcm, const int32_t * n_samples, const int32_t * offsets_ms,
                           const int32_t * key_len, int n_clips, float * out_host, int32_t * out_len, int32_t * status);

/* log-mel of one clip (whisper_pcm_to_mel semantics): writes [n_mels][n_len] into mel_out (capacity
 * mel_cap floats) and *n_len. Runs the same kernels as the encoder on the engine's device. */
int q2a_pcm_to_mel(q2a_engine * e, const float * pcm, int n_samples, float * mel_out, int64_t mel_cap, int * n_len);

/* ---- encode from log-mel features instead of PCM ------------------------------------------------------------
 * The reference's second way in: whisper_set_mel + whisper_encode (include/qwen2-whisper.h:228-250,
 * src/qwen2-whisper.cpp:2264-2286, 3281-3308). The caller's mel is f32, already normalised: the values
 * q2a_pcm_to_mel / whisper_pcm_to_mel return and transformers' WhisperFeatureExtractor produces as input_features
 * (clamp to max - 8, then (x + 4) / 4). Clip c is [n_mels][ld] with n_len[c] <= ld frames; its encoder window is
 * frames seek[c] .. seek[c] + 2 n_audio_ctx - 1, and window frames at or past n_len[c] are ZEROS (the reference clears
 * the window and copies what exists) — not the value the PCM path's padding takes. Nothing at or past frame n_len[c] of
 * a row is read. There is no 1 s rule at this level (whisper_encode has none): every clip is encoded, Q2A_CLIP_ENCODED.
 * One kernel writes the conv1 operand from the caller's array (no mel scratch, no clip maximum); everything behind it
 * is the PCM entry points' path, so mel = q2a_pcm_to_mel(pcm), seek = offset_ms / 10 returns their bytes.
 *
 * q2a_mel_valid_lengths: q2a_valid_lengths for n_len frames encoded from frame seek (host arithmetic, also exported
 * from libq2a_host.so):
 *   frames  = clamp(n_len - seek, 1, 2 * n_audio_ctx);  enc_len = (frames - 1) / 2 + 1;  out_len = enc_len / 2
 * Either output pointer may be NULL. Q2A_ERR_ARG for n_len < 1, seek < 0 or n_audio_ctx <= 0. */
enum { Q2A_ENCODE_PLAIN = 0, Q2A_ENCODE_PADDED = 1, Q2A_ENCODE_VARLEN = 2 };
int q2a_mel_valid_lengths(int n_len, int seek, int n_audio_ctx, int32_t * enc_len, int32_t * out_len);

/* kind         Q2A_ENCODE_PLAIN: q2a_encode_device_ex behind the mel (all n_audio_ctx keys; key_len and out_len are
 *              not read or written); Q2A_ENCODE_PADDED / Q2A_ENCODE_VARLEN: q2a_encode_device_padded / _varlen behind
 *              it (Q2A_ERR_UNSUPPORTED for Q2A_ACT_BF16, nothing written)
 * mel_dev      device f32, clip c at mel_dev + c * clip_stride, [n_mels][ld]; ld, seek and the pointer need no
 *              alignment beyond a float's
 * clip_stride  floats between clips: >= n_mels * ld, or 0: every clip reads the same array (the windows of one
 *              recording at different seeks)
 * n_len        host [n_clips], 1 <= n_len[c] <= ld
 * seek         host [n_clips], seek[c] >= 0 (at or past n_len[c]: an all-zero window), or NULL: 0 for every clip
 * key_len      host [n_clips], 1 <= key_len[c] <= n_audio_ctx, or NULL: q2a_mel_valid_lengths' enc_len of each clip
 * out_dev, out_len, status, stream   as in q2a_encode_device_padded (no clip is skipped)
 * Every argument is checked before anything is launched (Q2A_ERR_ARG). */
int q2a_encode_device_mel(q2a_engine * e, int kind, const float * mel_dev, int64_t clip_stride, int64_t ld,
                          const int32_t * n_len, const int32_t * seek, const int32_t * key_len, int n_clips,
                          float * out_dev, int32_t * out_len, int32_t * status, void * stream);
/* Same with host buffers in and out (synchronous): mel[c] is clip c's [n_mels][n_len[c]] (ld = n_len[c]). Only the
 * window columns of each row are copied to the device; chunks, overlap and Q2A_CLIP_FAILED as in q2a_encode_host_ex. */
int q2a_encode_host_mel(q2a_engine * e, int kind, const float * const * mel, const int32_t * n_len, const int32_t * seek,
                        const int32_t * key_len, int n_clips, float * out_host, int32_t * out_len, int32_t * status);

/* ---- one process, several GPUs (ncclCommInitAll + a host thread per device) -----------------------
 * Replaces the single-device choice of whisper_backend_init_gpu (qwen2-whisper.cpp:1217-1279) for batches of
 * independent clips, and is what whisper_full_parallel (declared, never defined, include/qwen2-whisper.h:464-469)
 * runs on when more than one device is visible (include/q2a_whisper.h). */
typedef struct q2a_group q2a_group;
int q2a_device_count(void);   /* visible HIP devices (0 when none) */
/* Open one engine per device of devices[0..n_devices) (n_devices = 0: every visible device). The model is packed
 * once on the host into its compact transport form, uploaded to devices[0] and sent to the others by ONE
 * ncclBroadcast over xGMI (RCCL communicators from ncclCommInitAll); each device expands its copy into the device
 * layout. act: Q2A_ACT_REFERENCE / Q2A_ACT_BF16. NULL on error (q2a_last_error). */
q2a_group * q2a_group_open(const char * model_path, const int * devices, int n_devices, int act);
/* The same over an engine that is already open (its weights, activation contract and device): base's device must be
 * in devices[0..n_devices) (n_devices = 0: base's device first, then every other visible device). base's own
 * device-layout weights are the root of the ONE ncclBroadcast (no second pack of the model file, no second replica on
 * base's device: that device's group engine shares base's weights, q2a_open_shared); every other device keeps the
 * replica it received. base must outlive the group. NULL on error (q2a_last_error). */
q2a_group * q2a_group_open_with(q2a_engine * base, const int * devices, int n_devices);
void q2a_group_close(q2a_group * g);
int q2a_group_size(const q2a_group * g);
q2a_engine * q2a_group_engine(q2a_group * g, int i);   /* the engine of the group's i-th device (owned by the group) */
/* The contiguous clip range [*first, *first + *count) the group gives its i-th device out of n_clips: near-equal,
 * the first n_clips % n_devices ranges one clip longer. Pure host arithmetic. */
int q2a_group_split(int n_clips, int n_devices, int i, int * first, int * count);
/* q2a_encode_host_ex over the group: every device encodes its clip range on its own host thread (no collective on
 * the data path); outputs and statuses land at the clips' own positions. offsets_ms may be NULL (offset_ms for all).
 * On error the first failing device's code is returned; its clips and every clip whose output never reached
 * out_host report Q2A_CLIP_FAILED. */
int q2a_group_encode_host(q2a_group * g, const float * const * pcm, const int32_t * n_samples, const int32_t * offsets_ms,
                          int n_clips, int offset_ms, float * out_host, int32_t * status);
/* Start-up cost of q2a_group_open: host pack, H2D + broadcast, per-device expand (seconds), transport bytes
 * (q2a_group_open_with: pack 0, the broadcast, the engines' open; the device-layout bytes broadcast). */
int q2a_group_setup_times(const q2a_group * g, double * pack_s, double * broadcast_s, double * open_s, int64_t * blob_bytes);

/* ---- per-kernel timing (HIP events recorded on the launch stream around every kernel of a class) ---- */
enum {
    Q2A_PROF_MEL = 0, Q2A_PROF_CONV1, Q2A_PROF_CONV2, Q2A_PROF_LN, Q2A_PROF_GEMM_QKV, Q2A_PROF_ATTN,
    Q2A_PROF_QUANT, Q2A_PROF_GEMM_O, Q2A_PROF_GEMM_FC1, Q2A_PROF_GEMM_FC2, Q2A_PROF_POOL, Q2A_PROF_CLASSES
};
int q2a_profile_enable(q2a_engine * e, int on);
/* time only the classes whose bit (1 << Q2A_PROF_*) is set (0 = off): fewer event pairs in a timed loop */
int q2a_profile_enable_mask(q2a_engine * e, unsigned mask);
/* accumulated milliseconds and launch counts per class (waits for the recorded events); reset != 0 clears */
int q2a_profile_read(q2a_engine * e, double * ms, int64_t * counts, int n, int reset);

/* ---- kernel-level entry points (device pointers), used by the parity tests ------------------------------ */
/* Y[M][N] = X[M][K] . W[N][K]^T for one linear weight of the loaded model (layer `layer`, which = 0 qkv
 * (raw, no bias/scale), 1 out_proj, 2 fc1, 3 fc2), with ggml's activation conversion of X (fp16 / Q8_K / Q8_0). */
int q2a_test_linear(q2a_engine * e, int layer, int which, const float * x_dev, int M, float * y_dev, void * stream);
/* One encoder block in place on X [n_clips*T][D] (f32, device). */
int q2a_test_block(q2a_engine * e, int layer, float * x_dev, int n_clips, void * stream);
/* Same, also copying the four GEMM A operands of the block as the MFMA consumed them into taps[0..3] (device,
 * 2-byte elements, NULL entries skipped): LN1 -> QKV [M][D], attention -> O [M][D], LN2 -> fc1 [M][D], GELU -> fc2
 * [M][F] (fp16 values for F16 files; Q8_K / Q8_0 integer codes held in fp16 for quantized files). Per-layer
 * divergence trace against the reference's own intermediates (diag/layer_trace.py). */
int q2a_test_block_taps(q2a_engine * e, int layer, float * x_dev, int n_clips, void * const * taps, void * stream);
/* Front end only: PCM [n_clips][pcm_stride] (device) -> log-mel -> conv1 + GELU -> conv2 + GELU -> + positions, the
 * first block's input X [n_clips*T][D] f32 (device) — the reference's embd_conv + pe (qwen2-whisper.cpp:1892-2005). */
int q2a_test_frontend(q2a_engine * e, const float * pcm_dev, int64_t pcm_stride, const int32_t * n_samples, int n_clips,
                      float * x_dev, void * stream);
/* The same from log-mel (q2a_encode_device_mel's mel_dev, clip_stride, ld, n_len, seek and checks): the ingest kernel
 * in place of the mel kernels, then the same conv launches. */
int q2a_test_frontend_mel(q2a_engine * e, const float * mel_dev, int64_t clip_stride, int64_t ld, const int32_t * n_len,
                          const int32_t * seek, int n_clips, float * x_dev, void * stream);
/* AvgPool1d(2) + final LayerNorm only: X [n_clips*T][D] f32 (device) -> out [n_clips][T/2][D] f32 (device)
 * (qwen2-whisper.cpp:2157-2181). */
int q2a_test_pool_ln(q2a_engine * e, const float * x_dev, int n_clips, float * out_dev, void * stream);
/* Q4_K files: how fc1's output reaches fc2 as Q8_K codes — 0 (default) fp16 pre-activation + GELU inside the
 * quantizer, 1 GELU in the fc1 epilogue + quantizer, 2 GELU + Q8_K fused into the fc1 epilogue. All three give
 * identical codes (tests/test_gpu_parity.py::test_deferred_gelu_equals_epilogue_gelu); a test hook, not a tuning knob. */
int q2a_test_fc1_path(q2a_engine * e, int path);
/* One activation conversion — the kernels that write a weight GEMM's A operand — on caller rows, launched with the
 * arguments and dispatch of the encoder block and q2a_test_linear. The engine supplies the device, the stream and the
 * GELU table only: M and K are free (any model file serves), within the launchers' own limits.
 *   producer  Q2A_OPERAND_LN         LayerNorm(x; g, b) + conversion: x f32 [M][K], g, b f32 [K], K % 4 == 0, K <= 2048;
 *                                    mode 0 fp16, 1 Q8_K, 2 Q8_0, 3 the F32 files' split [M][3K] = hi | lo | hi, 4 bf16
 *             Q2A_OPERAND_QUANT_F32  quantizer of f32 rows x [M][K] (the O-projection operand; K > 2048: the 1024-wide
 *                                    segments of the fc2 operand), mode 1 or 2, K % 256 == 0, K <= 8192
 *             Q2A_OPERAND_QUANT_H16  the same on fp16 rows x [M][K]
 *             Q2A_OPERAND_GELU_Q8K   GELU table + Q8_K of fp16 pre-activation rows x [M][K], mode 1, M * K < 2^31
 *   out       [M][K] 2-byte elements (mode 3: [M][3K]): fp16 / bf16 values, or the integer codes held in fp16
 *   dy        modes 1, 2: the block scales, block-major f32 [K/256 or K/32][ld], block bf of row m at dy[bf * ld + m]
 *   aext      mode 1: the block-sum operand, fp16 [K/256][ld][16] — for each of the 8 32-wide sub-blocks the pair
 *             (hi, lo), bsum32 = 64 hi + lo, 0 <= lo < 64
 *   ld        leading dimension of dy and aext, >= M
 * Nothing outside rows 0 .. M-1 of out, dy and aext is written. g, b, dy, aext may be NULL where the mode has no use
 * for them. Q2A_ERR_ARG for anything else. */
enum { Q2A_OPERAND_LN = 0, Q2A_OPERAND_QUANT_F32 = 1, Q2A_OPERAND_QUANT_H16 = 2, Q2A_OPERAND_GELU_Q8K = 3 };
int q2a_test_operand(q2a_engine * e, int producer, int mode, const void * x_dev, int M, int K, const float * g_dev,
                     const float * b_dev, void * out_dev, float * dy_dev, void * aext_dev, int ld, void * stream);
/* One weight GEMM of the encoder block with the block's own fused epilogue, on caller rows and into caller buffers.
 * x_dev [M][K] f32 becomes the GEMM operand as in q2a_test_linear; the GEMM arguments come from the helpers run_block
 * itself uses, with only the output pointers replaced by out[] — the kernel stores straight into the caller's memory,
 * so a store outside rows 0 .. M-1 lands in the caller's guard rows.
 *   which, epi                 out[]
 *   0, Q2A_TEST_EPI_QKV        reference contract: Q hi, Q lo, K hi, K lo, V hi, V lo, fp16 [M][D] each (Q scaled as in
 *                              the block); bf16 contract: Q, K bf16 [M][D] and V^T bf16 [clips][H][64][TP]
 *   1 | 3, Q2A_TEST_EPI_RESID  one f32 [M][D] buffer: the residual on entry, (acc + bias) + residual on exit (in place)
 *   2, Q2A_TEST_EPI_GELU_H     fp16 (bf16 contract: bf16) [M][F]; F32 files [M][3F] with the copy at column 2F
 *   2, Q2A_TEST_EPI_PRE_H      fp16 [M][F]: Q4_K / Q5_K / Q6_K files (fc1 path 0)
 *   2, Q2A_TEST_EPI_GELU_Q8K   codes fp16 [M][F], d f32 [F/256][ld], block sums fp16 [F/256][ld][16] as in
 *                              q2a_test_operand; ld % 256 == 0, ld >= M; only where fc1 path 2 takes it (Q4_K-layout
 *                              weights at a row count of the 8-phase wide tiles)
 * ld is read for GELU_Q8K only. Q2A_ERR_ARG for every combination the block never launches on this engine (PRE_H on
 * an F16 file, QKV with which != 0, ...). */
enum { Q2A_TEST_EPI_QKV = 0, Q2A_TEST_EPI_RESID = 1, Q2A_TEST_EPI_GELU_H = 2, Q2A_TEST_EPI_GELU_Q8K = 6, Q2A_TEST_EPI_PRE_H = 7 };
int q2a_test_gemm_epi(q2a_engine * e, int layer, int which, int epi, const float * x_dev, int M, void * const * out,
                      int ld, void * stream);
/* The tile regime the GEMM launcher picks for that GEMM at M rows on this engine's device (the launcher's own
 * decision function, nothing is launched), or Q2A_ERR_ARG where q2a_test_gemm_epi would return it. */
enum {
    Q2A_REGIME_NONE = -1,             /* no kernel for these arguments */
    Q2A_REGIME_NARROW = 0,            /* 64x128 tiles, 8 waves (few rows) */
    Q2A_REGIME_128 = 1,               /* 128x128 tiles, 4 waves */
    Q2A_REGIME_128x256 = 2,           /* 128x256 tiles, 8 waves (block-quantized weights, many rows) */
    Q2A_REGIME_256 = 3,               /* 256x256 tiles without the 8-phase pipeline (fp16 / bf16, odd K-step count) */
    Q2A_REGIME_PIPE8 = 4,             /* 8-phase 256x256 tiles, one grid */
    Q2A_REGIME_PIPE8_PERSISTENT = 5,  /* 8-phase persistent workgroups walking a tile list */
    Q2A_REGIME_PIPE8_TAIL = 6,        /* 8-phase whole rounds + 128x128 tiles on the rows of the partial round */
    Q2A_REGIME_FIXED = 7              /* one configuration whatever M: Q6_K (128x128), the conv GEMMs' exact tiles */
};
int q2a_test_gemm_regime(q2a_engine * e, int which, int epi, int M);
/* Attention only: q,k,v [n_clips*T][D] f32 (q already scaled), out [n_clips*T][D] f32.
 * Every operand enters the kernel as an fp16 pair hi = fp16(x), lo = fp16(x - hi) (q after the log2 e factor), which
 * carries 22 bits only while x - hi stays above fp16's 2^-24 spacing. Against float64 the F32-class bar (2e-5 max-rel,
 * 5e-6 rel-L2) was measured to hold with q, k and v elements of typical magnitude 2^-4 .. 2^4 and to end at typical
 * magnitude 2^-8 (v: rel-L2 4.5e-6; q or k: up to 1.7e-5); at 2^-12 the result is that of a one-term fp16 kernel
 * (7e-5 .. 2.6e-4). The window belongs to each operand by itself, whatever the scores: Q*2^-8 with K*2^8 leaves it.
 * Nothing rescales the operands (tests/test_gpu_attention_edges.py::test_scale_window). */
int q2a_test_attention(q2a_engine * e, const float * q_dev, const float * k_dev, const float * v_dev, int n_clips,
                       float * out_dev, void * stream);
/* q2a_test_attention / q2a_test_block with per-clip key lengths (host array [n_clips], 1 <= key_len[c] <= n_audio_ctx,
 * uploaded by the call): the key-length instantiation of the attention kernel. Reference activation contract only. */
int q2a_test_attention_len(q2a_engine * e, const float * q_dev, const float * k_dev, const float * v_dev, int n_clips,
                           const int32_t * key_len, float * out_dev, void * stream);
int q2a_test_block_len(q2a_engine * e, int layer, float * x_dev, int n_clips, const int32_t * key_len, void * stream);
/* The same two on packed rows (q2a_varlen_rows over key_len, 1 <= key_len[c] <= n_audio_ctx): q, k, v, out and x are
 * [M_tot][D]; the packed instantiation of the attention kernel. Rows behind M_tot are not touched. */
int q2a_test_attention_varlen(q2a_engine * e, const float * q_dev, const float * k_dev, const float * v_dev, int n_clips,
                              const int32_t * key_len, float * out_dev, void * stream);
int q2a_test_block_varlen(q2a_engine * e, int layer, float * x_dev, int n_clips, const int32_t * key_len, void * stream);

/* ---- downstream consumer: the Qwen2-Audio multi-modal projector ------------------------
 * audio_features = Linear(d_model -> text hidden size, bias)(embd_enc) — transformers' Qwen2AudioMultiModalProjector
 * (modeling_qwen2_audio.py), the step after the reference's path ends at embd_enc (qwen2-whisper.cpp:2185; the
 * reference has no projector). Weights: a projector file in the ggml container (multi_modal_projector.linear.weight
 * [d_out][d_in] F16 / Q4_K / Q5_K / Q6_K / Q8_0 / Q4_0, .bias [d_out] F32; bin/q2a_tool gen-projector + quantize). Numerics: a ggml
 * MUL_MAT of that weight type (activations per vec_dot_type, exact products, fp32 accumulation) + bias in f32.
 * d_out % 128 == 0; d_in % 256 == 0 (F16 weights: % 64), else q2a_projector_open fails. */
typedef struct q2a_projector q2a_projector;
q2a_projector * q2a_projector_open(const char * path, int device);
void q2a_projector_close(q2a_projector * p);
int q2a_projector_get_dims(const q2a_projector * p, int * d_in, int * d_out, int * wtype);
/* y_dev [rows][d_out] f32 = x_dev [rows][d_in] f32 (device) projected; asynchronous on `stream` (NULL = own stream).
 * A projector handle owns ONE workspace (the quantized activation operand): calls on one handle must be ordered on one
 * stream (or the caller synchronises between streams); use one handle per stream for concurrent projections. */
int q2a_projector_apply(q2a_projector * p, const float * x_dev, int64_t rows, float * y_dev, void * stream);

/* ---- audio features in one call: the valid output rows of every clip, packed, through the projector ----------------
 * What Qwen2AudioForConditionalGeneration scatters into the text embeddings: audio_features = the projector applied to
 * the valid rows of embd_enc only, one clip after the other. These entry points are q2a_encode_device_varlen /
 * q2a_encode_device_mel(kind = Q2A_ENCODE_VARLEN) up to and including the encoder blocks; one kernel then pools and
 * normalises the valid rows of the packed stream and writes them packed — as f32 (embd) and / or straight as the
 * projector GEMM's activation operand — and the projector's GEMM writes feat. No padded [n_clips][n_out][D] buffer, no
 * gather, no second pass over the f32 rows. The bytes are those of the composition: feat = q2a_projector_apply of the
 * concatenated rows out[c][0 .. out_len[c]-1] of q2a_encode_device_varlen, embd those rows themselves.
 *
 * q2a_packed_out_rows: where clip c's rows lie (host arithmetic; also exported from libq2a_host.so):
 *   out_start[0] = 0, out_start[c+1] = out_start[c] + key_len[c] / 2          (out_start has n_clips + 1 entries)
 * key_len[c] in 0 .. n_audio_ctx (0: a clip that is not encoded). Returns N_tot = out_start[n_clips], Q2A_ERR_ARG for a
 * length outside the range, n_clips < 0 or n_audio_ctx <= 0. */
int64_t q2a_packed_out_rows(const int32_t * key_len, int n_clips, int n_audio_ctx, int32_t * out_start);

/*   p           the projector, or NULL: feat_dev must then be NULL and only the packed embd_enc is written
 *   feat_dev    [rows_cap][d_out] f32, required with p (Q2A_ERR_ARG without it)
 *   embd_dev    [rows_cap][n_audio_state] f32, or NULL (both outputs NULL: Q2A_ERR_ARG)
 *   rows_cap    rows the output arrays hold; N_tot <= rows_cap or Q2A_ERR_ARG (n_clips * n_out always suffices)
 *   out_len     host [n_clips], may be NULL: clip c has out_len[c] = key_len[c] / 2 rows (0 for a skipped clip), rows
 *               out_start[c] .. out_start[c+1]-1 of feat_dev / embd_dev; rebuild out_start as the prefix sum of out_len,
 *               or with q2a_packed_out_rows from the key lengths passed in
 * pcm_dev / mel_dev and their arguments, key_len (NULL: the derived lengths), status, the 1 s rule (PCM only) and stream
 * are those of q2a_encode_device_varlen / q2a_encode_device_mel. Every check — theirs, the output arguments above, p on
 * the engine's device with d_in = n_audio_state (Q2A_ERR_ARG), the reference activation contract (Q2A_ERR_UNSUPPORTED) —
 * is made before anything is launched or written. Rows at or past N_tot are never written; with no valid row at all
 * (every clip skipped, or every key length 1) the call returns Q2A_OK and launches nothing behind the metadata upload.
 * The activation operand lives in p's workspace: q2a_projector_apply's one-stream rule covers these calls too.
 * Not covered: the whisper_* API, q2a_group_*, the ggml backend. (fp16 / bf16 output, and rows placed where the caller
 * wants them: the q2a_*_to calls below.) */
int q2a_audio_features_device(q2a_engine * e, q2a_projector * p, const float * pcm_dev, int64_t pcm_stride,
                              const int32_t * n_samples, const int32_t * offsets_ms, const int32_t * key_len, int n_clips,
                              float * feat_dev, float * embd_dev, int64_t rows_cap, int32_t * out_len, int32_t * status,
                              void * stream);
int q2a_audio_features_device_mel(q2a_engine * e, q2a_projector * p, const float * mel_dev, int64_t clip_stride, int64_t ld,
                                  const int32_t * n_len, const int32_t * seek, const int32_t * key_len, int n_clips,
                                  float * feat_dev, float * embd_dev, int64_t rows_cap, int32_t * out_len, int32_t * status,
                                  void * stream);
/* Same with host buffers in and out (synchronous): pcm as in q2a_encode_host_varlen, mel as in q2a_encode_host_mel;
 * feat_host / embd_host [rows_cap][...] receive the rows of all clips in clip order. Clips go through the device path in
 * chunks of up to 64; on an error, clips whose rows did not reach the caller report Q2A_CLIP_FAILED and out_len 0. */
int q2a_audio_features_host(q2a_engine * e, q2a_projector * p, const float * const * pcm, const int32_t * n_samples,
                            const int32_t * offsets_ms, const int32_t * key_len, int n_clips, float * feat_host, float * embd_host,
                            int64_t rows_cap, int32_t * out_len, int32_t * status);
int q2a_audio_features_host_mel(q2a_engine * e, q2a_projector * p, const float * const * mel, const int32_t * n_len,
                                const int32_t * seek, const int32_t * key_len, int n_clips, float * feat_host, float * embd_host,
                                int64_t rows_cap, int32_t * out_len, int32_t * status);
/* ---- audio features as f32 / fp16 / bf16, stored in place into the consumer's rows --------------------------------------
 * Qwen2AudioForConditionalGeneration casts audio_features to the language model's dtype and masked_scatters them into
 * inputs_embeds at the audio-token positions. The _to calls do both in the projector GEMM's epilogue: every value is the
 * f32 call's value fl32(acc + bias[n]) — same tile regime, same K order, same accumulators — rounded once more, to
 * nearest even, for the 16-bit types, and stored at row row_map[m] of the destination. No cast pass, no indexed copy,
 * no f32 temporary. */
enum { Q2A_DT_F32 = 0, Q2A_DT_F16 = 1, Q2A_DT_BF16 = 2 };
typedef struct {
    void * base;      /* device; 16-byte aligned */
    int64_t ld;       /* elements between rows, >= d_out, ld * element size a multiple of 16 */
    int64_t n_rows;   /* rows the destination holds (<= INT32_MAX) */
    int32_t dtype;    /* Q2A_DT_* */
    int32_t reserved; /* 0 */
} q2a_feat_dst;
/* q2a_projector_apply with that epilogue (same operand conversion, workspace and one-stream rule): packed row m of
 * x_dev goes to destination row row_map_dev[m] (device int32 [rows]; NULL: row m, rows <= n_rows required), element
 * (r, n) at base + (r * ld + n) * element size. A row with r < 0 or r >= n_rows is not stored — whatever the map holds,
 * nothing outside [0, n_rows) x [0, d_out) is written; columns d_out .. ld-1 of a row are never written. Q2A_ERR_ARG
 * for a NULL or misaligned base, ld < d_out, ld * element size % 16 != 0, an unknown dtype, reserved != 0, n_rows
 * outside 0 .. INT32_MAX. */
int q2a_projector_apply_to(q2a_projector * p, const float * x_dev, int64_t rows, const q2a_feat_dst * dst,
                           const int32_t * row_map_dev, void * stream);
/* The Q2A_REGIME_* the projector's GEMM takes at `rows` rows on p's device: the launcher's own decision function,
 * nothing is launched. One answer for q2a_projector_apply and q2a_projector_apply_to. Q2A_ERR_ARG for bad arguments. */
int q2a_projector_regime(q2a_projector * p, int64_t rows);
/* q2a_feat_rows: the destination rows of a call (host arithmetic; also exported from libq2a_host.so). Clip c's out_len[c]
 * rows go to destination rows clip_row[c] .. clip_row[c] + out_len[c] - 1 (the contiguous run of audio tokens the
 * processor emits per clip); clip_row NULL: packed, clip after clip from row 0. A clip with out_len[c] = 0 is ignored,
 * whatever its clip_row. Returns N_tot = sum of out_len and fills row_map (may be NULL) for the packed rows 0 .. N_tot-1.
 * Q2A_ERR_ARG, with nothing written, for a negative out_len or start, a range past n_rows, two non-empty ranges that
 * overlap, out_len NULL with n_clips > 0, n_clips < 0, n_rows < 0 or N_tot > INT32_MAX. */
int64_t q2a_feat_rows(const int32_t * out_len, const int32_t * clip_row, int n_clips, int64_t n_rows, int32_t * row_map);
/* q2a_audio_features_device / _device_mel with dst and clip_row (host [n_clips], or NULL: packed) in place of feat_dev and
 * rows_cap. p and dst are required. embd_dev (optional) still receives the packed f32 rows, against its own
 * embd_rows_cap. Every check of the f32 calls, q2a_projector_apply_to's checks of dst and q2a_feat_rows' checks of the
 * ranges (over the clips that are encoded) are made before anything is launched or written. The device row map is built
 * inside the call by one small kernel from the call's single metadata upload (clip_row rides in it) and lives in p's
 * workspace; with clip_row NULL there is no map and no extra launch. Reference activation contract only
 * (Q2A_ERR_UNSUPPORTED otherwise). The host variants stay f32. */
int q2a_audio_features_device_to(q2a_engine * e, q2a_projector * p, const float * pcm_dev, int64_t pcm_stride,
                                 const int32_t * n_samples, const int32_t * offsets_ms, const int32_t * key_len, int n_clips,
                                 const q2a_feat_dst * dst, const int32_t * clip_row, float * embd_dev, int64_t embd_rows_cap,
                                 int32_t * out_len, int32_t * status, void * stream);
int q2a_audio_features_device_mel_to(q2a_engine * e, q2a_projector * p, const float * mel_dev, int64_t clip_stride, int64_t ld,
                                     const int32_t * n_len, const int32_t * seek, const int32_t * key_len, int n_clips,
                                     const q2a_feat_dst * dst, const int32_t * clip_row, float * embd_dev,
                                     int64_t embd_rows_cap, int32_t * out_len, int32_t * status, void * stream);
/* ---- inputs_embeds on the device: the audio rows placed by input_ids, the text rows gathered ----------------------------
 * The model does inputs_embeds = embed_tokens(input_ids), then masked_scatter(input_ids == audio_token_id, audio_features):
 * the k-th feature row goes to the k-th audio token, wherever it is. The calls below do that on the device from the
 * input_ids the pipeline already holds there: one compaction (two small kernels: a count per chunk of 2048 tokens, then
 * the places; stable, deterministic, no workgroup waits for another) writes the row map of the projector GEMM's row-map
 * epilogue into p's workspace, and one gather kernel copies the text rows out of the embedding table. No copy of
 * input_ids to the host, no run-finding, no separate embedding pass; audio tokens need not form one run per clip. */
typedef struct {
    const void * input_ids;    /* device [n_tokens], int32 or int64 (aligned to its width); int64 ids are compared on
                                  all 64 bits */
    int32_t ids_width;         /* 4 or 8 */
    int32_t reserved;          /* 0 */
    int64_t n_tokens;          /* must equal dst->n_rows; 1 .. 2^24 */
    int64_t audio_token_id;
    const void * embed_table;  /* device [vocab][table_ld] of dst's dtype, 16-byte aligned, table_ld >= d_out,
                                  table_ld * element size % 16 == 0; NULL: text rows are left untouched (vocab and
                                  table_ld are then not read) */
    int64_t vocab, table_ld;   /* vocab >= 1 */
    int32_t * report_dev;      /* device int32[4] or NULL: audio tokens found, feature rows of the call,
                                  text ids outside [0, vocab), flags (bit 0: found != rows, bit 1: bad ids) */
} q2a_embeds_src;
/* The row map of these calls, on the host (pure arithmetic; also exported from libq2a_host.so): row_map[k] = the flat
 * position of the k-th id equal to audio_token_id for k < min(count, map_cap), -1 for count <= k < map_cap. Returns
 * count, the number found, even where it exceeds map_cap. Q2A_ERR_ARG, with nothing written, for a width other than
 * 4 / 8, n_tokens outside 0 .. INT32_MAX, a NULL ids_host with n_tokens > 0, map_cap < 0 or row_map NULL with
 * map_cap > 0. */
int64_t q2a_audio_token_rows(const void * ids_host, int32_t ids_width, int64_t n_tokens, int64_t audio_token_id,
                             int32_t * row_map, int64_t map_cap);
/* q2a_projector_apply_to with the map derived from src (feature row k of x_dev to the k-th audio token's row), and the
 * gather: for every position t, input_ids[t] == audio_token_id leaves row t to the GEMM; 0 <= id < vocab copies row id
 * of the table to row t (d_out elements, a byte copy in 16-byte pieces); any other id stores nothing and is counted.
 * Columns d_out .. ld-1 of a row are never written. When the audio tokens found differ from `rows`, the first
 * min(found, rows) pairs are placed, further feature rows are dropped (map entry -1), further audio positions keep what
 * they held, and the report says so (HF raises there). Every check — q2a_projector_apply_to's, and of src: non-NULL,
 * input_ids non-NULL and aligned, ids_width, reserved, n_tokens in range and equal to dst->n_rows, and with a table its
 * alignment, table_ld and vocab — is made before anything is launched or written (Q2A_ERR_ARG). The compaction and the
 * gather run on the call's stream in front of the GEMM; the map, the chunk counts (and the report words when
 * report_dev is NULL) live in p's workspace. */
int q2a_projector_apply_ids(q2a_projector * p, const float * x_dev, int64_t rows, const q2a_feat_dst * dst,
                            const q2a_embeds_src * src, void * stream);
/* q2a_audio_features_device_to / _device_mel_to with src in place of clip_row: a finished inputs_embeds in one call. The
 * _to calls' own checks (no clip ranges: the map comes from input_ids) and q2a_projector_apply_ids' checks of src are
 * made before anything is launched or written. The GEMM is the _to call's with that map: same operand, M, N, K, hence
 * the same tile regime and the same bits as q2a_audio_features_device_mel_to given row_map = the audio positions. With no
 * valid audio row at all (N_tot = 0) no encoder kernel runs, but the gather does and the report is written
 * ({found, 0, bad ids, flags}). The three small launches are booked under the engine's pool profile class. */
int q2a_inputs_embeds_device(q2a_engine * e, q2a_projector * p, const float * pcm_dev, int64_t pcm_stride,
                             const int32_t * n_samples, const int32_t * offsets_ms, const int32_t * key_len, int n_clips,
                             const q2a_feat_dst * dst, const q2a_embeds_src * src, float * embd_dev, int64_t embd_rows_cap,
                             int32_t * out_len, int32_t * status, void * stream);
int q2a_inputs_embeds_device_mel(q2a_engine * e, q2a_projector * p, const float * mel_dev, int64_t clip_stride, int64_t ld,
                                 const int32_t * n_len, const int32_t * seek, const int32_t * key_len, int n_clips,
                                 const q2a_feat_dst * dst, const q2a_embeds_src * src, float * embd_dev,
                                 int64_t embd_rows_cap, int32_t * out_len, int32_t * status, void * stream);
/* Test hooks. q2a_test_audio_token_rows: the compaction exactly as these calls launch it (map and chunk counts in p's
 * workspace, sized for n_feat rows, 0 <= n_feat <= 2^28), then the n_feat map words copied to row_map_out_dev (device
 * int32 [n_feat]; nothing behind them is written); report_dev (device int32[4], required) receives
 * {found, n_feat, 0, found != n_feat}. q2a_test_embed_gather: the gather alone into dst (d_out columns; src's and dst's
 * checks as above, a table and report_dev required); the report is {0, 0, bad ids, bad ids ? 2 : 0}. */
int q2a_test_audio_token_rows(q2a_projector * p, const void * ids_dev, int32_t ids_width, int64_t n_tokens,
                              int64_t audio_token_id, int64_t n_feat, int32_t * row_map_out_dev, int32_t * report_dev,
                              void * stream);
int q2a_test_embed_gather(const q2a_embeds_src * src, const q2a_feat_dst * dst, int32_t d_out, void * stream);
/* Test hook: the pool kernel of these calls alone, with the engine's final-LayerNorm weights, on caller rows.
 *   x_dev      packed [M_tot][n_audio_state] f32 (q2a_varlen_rows over key_len, 1 <= key_len[c] <= n_audio_ctx)
 *   embd_dev   [N_tot][n_audio_state] f32 (q2a_packed_out_rows over key_len), or NULL
 *   codes_dev, dy_dev, aext_dev, ld   the operand of `mode` (0 fp16, 1 Q8_K, 2 Q8_0) for those N_tot rows in
 *              q2a_test_operand's layouts, ld >= N_tot; codes_dev NULL: no operand is written
 * The checks of q2a_test_block_varlen; nothing outside rows 0 .. N_tot-1 of any output is written. */
int q2a_test_pool_operand(q2a_engine * e, int mode, const float * x_dev, int n_clips, const int32_t * key_len, float * embd_dev,
                          void * codes_dev, float * dy_dev, void * aext_dev, int ld, void * stream);

#ifdef __cplusplus
}
#endif
#endif /* Q2A_ENCODER_H */
