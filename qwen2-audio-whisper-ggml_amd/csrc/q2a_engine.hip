// q2a_engine.hip — host orchestration of the MI355X encoder path behind the C ABI (include/q2a_encoder.h).
//
// Replaces whisper_full -> whisper_encoder_output_with_state (src/qwen2-whisper.cpp:2341-2383):
// log_mel_spectrogram (:2575) + whisper_encode_qwen2_internal (:2241) with its conv graph (:1892) and encoder
// graph (:1954), for a BATCH of independent clips in one pass. No ggml graph build / sched split / allocator at
// run time: the model is packed once into a device blob and every intermediate lives in a workspace reserved
// for the batch size, so a batch is ~11 launches per layer on one stream (capturable into a hipGraph).
#include "q2a_encoder.h"
#include "q2a_blob.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>

using namespace q2a_blob;

namespace {
thread_local std::string g_err;
}

void q2a_blob::set_err(const char * fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}

namespace {

__global__ void k_split_hilo(const float * x, q2a_half * hi, q2a_half * lo, int64_t n, float scale) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float v = x[i] * scale;
    asm volatile("" : "+v"(v));   // rounded to f32 before the split, as the QKV epilogue (no one-step fp16 rounding)
    const _Float16 h = (_Float16) v;
    hi[i] = h;
    lo[i] = (_Float16) (v - (float) h);
}

__global__ void k_to_half(const float * x, q2a_half * y, int64_t n) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = (_Float16) x[i];
}

__global__ void k_to_bf16(const float * x, q2a_half * y, int64_t n) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = __builtin_bit_cast(_Float16, (__bf16) x[i]);
}

// F32-weight activation operand: x [M][K] f32 -> [hi | lo | hi] rows of 3K fp16
__global__ void k_split3(const float * x, q2a_half * y, int K, int64_t n) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t m = i / K;
    const int k = (int) (i - m * K);
    const float v = x[i];
    const _Float16 h = (_Float16) v;
    q2a_half * o = y + m * 3 * K + k;
    o[0] = h;
    o[K] = (_Float16) (v - (float) h);
    o[2 * K] = h;
}

hipError_t launch_split3(const float * x, q2a_half * y, int K, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_split3, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, s, x, y, K, n);
    return hipGetLastError();
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// engine
// ------------------------------------------------------------------------------------------------
struct q2a_engine {
    int device = 0;
    hipStream_t stream = nullptr;
    blob_header h;
    dims d;
    int wtype = 0, blk = 0;   // blk: the activation quantizer's block (blk_of), 0 under the bf16 contract
    bool f32 = false;        // all-F32 model file: fp16 hi/lo split operands, GEMM K tripled (kx = 3)
    int kx = 1;
    bool bf16 = false;       // bf16-activation mode (Q2A_ACT_BF16): bf16 weights and inter-op activations
    int gblk = 0;            // the GEMM launcher's blk: blk, Q2A_BLK_Q6K for Q6_K weights, or Q2A_BLK_BF16
    uint8_t * blob = nullptr;
    bool own_blob = false;
    int64_t blob_size = 0;

    // workspace (capacity)
    int cap_clips = 0;
    void * ws = nullptr;
    size_t ws_bytes = 0;
    // host API (q2a_encode_host*): a copy stream and two sets of pinned + device staging buffers, so the PCIe copies
    // of one chunk of clips run beside the encode of the neighbouring chunk (host_pipe)
    struct host_buf {
        float * pin_in = nullptr; float * pin_out = nullptr; float * d_in = nullptr; float * d_out = nullptr;
        size_t in_cap = 0, out_cap = 0;   // floats
        hipEvent_t h2d = nullptr, comp = nullptr, d2h = nullptr;
    };
    hipStream_t copy_stream = nullptr;
    host_buf hb[2];
    int32_t * meta = nullptr;        // device: the per-clip metadata of a call, addressed through meta_rows
    int32_t * meta_host = nullptr;   // pinned, the same layout: written and uploaded by upload_meta alone
    hipEvent_t meta_evt = nullptr;   // last async upload out of meta_host (host rewrites wait on it)
    float * mel = nullptr;
    q2a_half * xc1 = nullptr;
    q2a_half * y1 = nullptr;
    float * X = nullptr;
    float * Xp = nullptr;            // packed residual stream of the variable-length encode, [xp_clips * T][D]: its own
    int xp_clips = 0;                //   allocation, made by the first such call (ensure_packed)
    q2a_half * actD = nullptr;
    q2a_half * actF = nullptr;
    float * dyD = nullptr;
    float * dyF = nullptr;
    q2a_half * aextD = nullptr;
    q2a_half * aextF = nullptr;
    q2a_half *qh = nullptr, *ql = nullptr, *kh = nullptr, *kl = nullptr, *vt = nullptr;
    q2a_half * vtl = nullptr;        // V^T lo image, when the attention build reads one (q2a_attention_wants_vlo)
    float * attF = nullptr;
    float * hF = nullptr;
    float * part = nullptr;          // split-K partials of the small-tile residual GEMMs (NULL: big batches)
    int2 * frange = nullptr;         // per mel filter: non-zero bin-group range (computed once from the blob)
    int TP = 0;
    int dy_ld = 0;
    bool force_encode = false;   // encode windows with under 1 s of audio too (whisper_full with duration_ms set)
    // Q4_K fc1 -> fc2 operand path (q2a_test_fc1_path; the three produce identical Q8_K codes):
    //   0 (default) fc1 writes its fp16 pre-activation, the Q8_K quantizer applies the GELU table on the way
    //   1 GELU in the fc1 epilogue, then the fp16-input quantizer
    //   2 GELU + Q8_K quantization fused into the fc1 epilogue (8-phase tiles only)
    int fc1_path = 0;
    // q2a_test_block_taps: device buffers receiving the GEMM A operands of one block (LN1 -> QKV, attention -> O,
    // LN2 -> fc1, GELU -> fc2) as they were fed to the MFMA, for the per-layer divergence trace (NULL: off)
    void * taps[4] = {nullptr, nullptr, nullptr, nullptr};

    // optional per-kernel-class timing with HIP events on the launch stream (q2a_profile_*)
    bool prof = false;
    struct rec { int cls; hipEvent_t a, b; };
    std::vector<rec> pending;
    std::vector<hipEvent_t> pool;
    unsigned prof_mask = ~0u;        // classes timed when prof is on (bit = Q2A_PROF_*)
    double prof_ms[Q2A_PROF_CLASSES] = {};
    int64_t prof_n[Q2A_PROF_CLASSES] = {};

    template <class P> P g(int i) const { return (P) (blob + h.goff[i]); }
    template <class P> P lv(int l, int i) const { return (P) (blob + h.loff[l][i]); }
    const uint64_t * mat(int l, int w) const { return h.loff[l] + L_MAT0 + w * A_COUNT; }
};

// the multi-modal projector (q2a_projector_*, below): one linear weight in q2a_pack_linear's layout, its bias, and one
// workspace for the activation operand of a call
struct q2a_projector {
    int device = 0;
    hipStream_t stream = nullptr;
    int d_in = 0, d_out = 0, wtype = 0, blk = 0, gblk = 0;   // blk: activation block, gblk: the GEMM's block mode
    void * wdev = nullptr;          // q2a_pack_linear layout
    uint64_t off[A_COUNT] = {};
    float * bias = nullptr;
    void * ws = nullptr;            // A operand [rows][d_in] fp16 | dy [d_in/blk][MP] | aext [d_in/256][MP][16]
                                    // | row map [MP] | chunk counts, 4 report words (calls with input_ids)
    size_t ws_bytes = 0;
    const uint16_t * gelu = nullptr;   // the GEMM's table argument (unused by STORE_F, kept valid)
};

namespace {

// A NULL `stream` argument of the device-pointer entry points (q2a_encode_device*, q2a_test_*, q2a_projector_apply)
// means the caller's legacy default stream (stream 0, torch's default stream): the work is issued ON it, so it starts
// after everything already queued there and everything queued there afterwards starts after it; inputs written and
// outputs read on stream 0 need no extra synchronisation. (Round 5 ran it on the handle's own stream between two
// cross-stream events: 0.2 ms per encode at one clip, diag/null_stream_ab.py, profiles/r06e_null_stream.jsonl.)
inline hipStream_t call_stream(const void * stream) { return (hipStream_t) stream; }

// The per-clip metadata of a call, on the device (e->meta) and pinned on the host (e->meta_host): five rows of the
// call's B entries, then row_start with B + 1 entries (the packed layout of the variable-length encode) and out_start
// with B + 1 entries (the packed output layout of the audio-feature calls, which alone upload it), and behind that
// (`end`, where the f32 audio-feature calls' copy stops) clip_row with B entries: the first destination row of every
// clip, uploaded by the q2a_audio_features_device*_to calls alone. clip_max is written on the device (the mel kernel's
// running maximum); every other row comes from the host through upload_meta.
constexpr size_t meta_words(int B) { return (size_t) B * 8 + 2; }
struct meta_rows {
    int32_t *nsamp, *seek, *clip_ok, *clip_max, *key_len, *row_start, *out_start, *end, *clip_row, *end_to;
    meta_rows(int32_t * p, int B)
        : nsamp(p), seek(p + B), clip_ok(p + 2 * B), clip_max(p + 3 * B), key_len(p + 4 * B), row_start(p + 5 * B),
          out_start(p + 6 * B + 1), end(p + 7 * B + 2), clip_row(end), end_to(p + meta_words(B)) {}
};

// The one writer of meta_host. It waits until the previous upload has left the pinned buffer (a queued copy may still
// read it), lets `fill` write the host rows first .. last (a failing `fill` uploads nothing), copies exactly those words
// to the same rows of e->meta on s, and records the event the next writer waits on.
template <class Fill>
int upload_meta(q2a_engine * e, int B, int32_t * meta_rows::*first, int32_t * meta_rows::*last, hipStream_t s, Fill fill) {
    const meta_rows host(e->meta_host, B), dev(e->meta, B);
    HIP_TRY(hipEventSynchronize(e->meta_evt));
    if (int rc = fill(host)) return rc;
    HIP_TRY(hipMemcpyAsync(dev.*first, host.*first, (size_t) (host.*last - host.*first) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(e->meta_evt, s));
    return Q2A_OK;
}

int engine_init(q2a_engine * e, int device) {
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) { set_err("device %d not available (%d devices)", device, n); return Q2A_ERR_HIP; }
    e->device = device;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&e->meta_evt, hipEventDisableTiming));
    return Q2A_OK;
}

int engine_adopt_header(q2a_engine * e) {
    if (const char * why = header_problem(e->h)) { set_err("%s", why); return Q2A_ERR_FORMAT; }
    e->d = dims_of(e->h.hp);
    e->wtype = e->h.wtype;
    e->blk = e->h.blk;
    e->f32 = e->wtype == Q2A_TYPE_F32;
    e->bf16 = e->h.act == Q2A_ACT_BF16;
    e->kx = e->f32 && !e->bf16 ? 3 : 1;
    e->gblk = e->bf16 ? Q2A_BLK_BF16 : gblk_of(e->wtype);
    e->TP = ((e->d.T + 63) / 64) * 64;
    return Q2A_OK;
}

void free_ws(q2a_engine * e) {
    if (e->ws) (void) hipFree(e->ws);
    if (e->meta_host) (void) hipHostFree(e->meta_host);
    if (e->Xp) (void) hipFree(e->Xp);
    e->ws = nullptr; e->meta_host = nullptr; e->Xp = nullptr;
    e->cap_clips = 0; e->ws_bytes = 0; e->xp_clips = 0;
}

void free_host_bufs(q2a_engine * e) {
    if (e->copy_stream) (void) hipStreamSynchronize(e->copy_stream);
    for (auto & b : e->hb) {
        if (b.pin_in) (void) hipHostFree(b.pin_in);
        if (b.pin_out) (void) hipHostFree(b.pin_out);
        if (b.d_in) (void) hipFree(b.d_in);
        if (b.d_out) (void) hipFree(b.d_out);
        for (hipEvent_t ev : {b.h2d, b.comp, b.d2h}) if (ev) (void) hipEventDestroy(ev);
        b = q2a_engine::host_buf{};
    }
    if (e->copy_stream) (void) hipStreamDestroy(e->copy_stream);
    e->copy_stream = nullptr;
}

// staging for host-API chunks of up to `clips` clips of `maxn` samples (grows; never shrinks)
int ensure_host_bufs(q2a_engine * e, int clips, int64_t maxn) {
    if (!e->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
    const size_t in = (size_t) clips * maxn, out = (size_t) clips * e->d.TO * e->d.D;
    for (auto & b : e->hb) {
        if (!b.h2d) {
            HIP_TRY(hipEventCreateWithFlags(&b.h2d, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&b.comp, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&b.d2h, hipEventDisableTiming));
        }
        if (in > b.in_cap || out > b.out_cap) {
            HIP_TRY(hipStreamSynchronize(e->copy_stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
        }
        if (in > b.in_cap) {
            if (b.pin_in) (void) hipHostFree(b.pin_in);
            if (b.d_in) (void) hipFree(b.d_in);
            b.pin_in = nullptr; b.d_in = nullptr; b.in_cap = 0;
            HIP_TRY(hipHostMalloc((void **) &b.pin_in, in * 4, hipHostMallocDefault));
            HIP_TRY(hipMalloc((void **) &b.d_in, in * 4));
            b.in_cap = in;
        }
        if (out > b.out_cap) {
            if (b.pin_out) (void) hipHostFree(b.pin_out);
            if (b.d_out) (void) hipFree(b.d_out);
            b.pin_out = nullptr; b.d_out = nullptr; b.out_cap = 0;
            HIP_TRY(hipHostMalloc((void **) &b.pin_out, out * 4, hipHostMallocDefault));
            HIP_TRY(hipMalloc((void **) &b.d_out, out * 4));
            b.out_cap = out;
        }
    }
    return Q2A_OK;
}

int reserve(q2a_engine * e, int B) {
    if (B <= e->cap_clips) return Q2A_OK;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());   // earlier calls may have run on any caller stream (or stream 0)
    if (e->ws) { (void) hipFree(e->ws); e->ws = nullptr; }
    if (e->meta_host) { (void) hipHostFree(e->meta_host); e->meta_host = nullptr; }
    const dims & d = e->d;
    const int64_t BT = (int64_t) B * d.T;
    const bool quant = e->blk != 0;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~size_t(255); return o; };
    const size_t o_meta = take(meta_words(B) * 4);
    const size_t o_mel = take((size_t) B * d.M * d.TM * 4);
    const size_t o_xc1 = take((size_t) B * (d.TM + 2) * 3 * d.M * 2);
    const size_t o_y1 = take((size_t) B * (d.TM + 1) * d.D * 2 * (e->f32 ? 2 : 1));
    const size_t o_X = take((size_t) BT * d.D * 4);
    const size_t o_actD = take((size_t) BT * d.D * 2 * e->kx);
    const size_t o_actF = take((size_t) BT * d.F * 2 * e->kx);
    const size_t o_qh = take((size_t) BT * d.D * 2);
    const size_t o_ql = take((size_t) BT * d.D * 2);
    const size_t o_kh = take((size_t) BT * d.D * 2);
    const size_t o_kl = take((size_t) BT * d.D * 2);
    const size_t o_vt = take((size_t) B * d.H * 64 * e->TP * 2);
    const bool vlo = !e->bf16 && q2a_attention_wants_vlo();
    const size_t o_vtl = vlo ? take((size_t) B * d.H * 64 * e->TP * 2) : 0;
    size_t o_dyD = 0, o_dyF = 0, o_aD = 0, o_aF = 0, o_att = 0, o_hF = 0, o_part = 0;
    // split-K partials of the small-tile residual GEMMs (O-proj, fc2): up to 4 x [rows][D] f32. Sized for every
    // row count that takes the small-tile path (M <= 26 112 at D = 1280), whatever the capacity, so whether a
    // batch splits never depends on what the engine encoded before
    const int64_t split_rows = std::min<int64_t>(BT, 32768);
    const bool split = !q2a_gemm_wide_tiles((int) split_rows, d.D, e->gblk);
    if (split) o_part = take((size_t) 4 * split_rows * d.D * 4);
    const int64_t MP = (BT + 255) / 256 * 256;   // padded row stride of the block-major scale arrays
    e->dy_ld = (int) MP;
    if (quant) {
        o_dyD = take((size_t) MP * (d.D / 32) * 4);
        o_dyF = take((size_t) MP * (d.F / 32) * 4);
        o_aD = take((size_t) MP * (d.D / 256 + 1) * 16 * 2);
        o_aF = take((size_t) MP * (d.F / 256 + 1) * 16 * 2);
        o_att = take((size_t) BT * d.D * 4);
        o_hF = take((size_t) BT * d.F * 4);
    } else if (e->f32) {
        o_att = take((size_t) BT * d.D * 4);
    }
    void * ws = nullptr;
    if (hipMalloc(&ws, off) != hipSuccess) {
        (void) hipGetLastError();
        set_err("workspace allocation of %.2f GB for %d clips failed", off / 1e9, B);
        return Q2A_ERR_OOM;
    }
    HIP_TRY(hipMemsetAsync(ws, 0, off, e->stream));   // zero pad rows (xc1 rows 0/last, y1 row 0, V^T tail)
    HIP_TRY(hipHostMalloc((void **) &e->meta_host, meta_words(B) * 4, hipHostMallocDefault));
    uint8_t * b = (uint8_t *) ws;
    e->ws = ws; e->ws_bytes = off; e->cap_clips = B;
    e->meta = (int32_t *) (b + o_meta);
    e->mel = (float *) (b + o_mel);
    e->xc1 = (q2a_half *) (b + o_xc1);
    e->y1 = (q2a_half *) (b + o_y1);
    e->X = (float *) (b + o_X);
    e->actD = (q2a_half *) (b + o_actD);
    e->actF = (q2a_half *) (b + o_actF);
    e->qh = (q2a_half *) (b + o_qh); e->ql = (q2a_half *) (b + o_ql);
    e->kh = (q2a_half *) (b + o_kh); e->kl = (q2a_half *) (b + o_kl);
    e->vt = (q2a_half *) (b + o_vt);
    e->vtl = vlo ? (q2a_half *) (b + o_vtl) : nullptr;
    e->part = split ? (float *) (b + o_part) : nullptr;
    if (quant) {
        e->dyD = (float *) (b + o_dyD); e->dyF = (float *) (b + o_dyF);
        e->aextD = (q2a_half *) (b + o_aD); e->aextF = (q2a_half *) (b + o_aF);
        e->attF = (float *) (b + o_att); e->hF = (float *) (b + o_hF);
    } else if (e->f32) {
        e->attF = (float *) (b + o_att);
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    return Q2A_OK;
}

q2a_gemm_args gemm_base(const q2a_engine * e, int l, int which, const q2a_half * A, int M) {
    q2a_gemm_args a;
    memset(&a, 0, sizeof(a));
    int N, K;
    mat_dims(e->d, which, N, K);
    const uint64_t * m = e->mat(l, which);
    a.A = A; a.lda = (int64_t) K * e->kx; a.a_rpg = M; a.a_gstride = 0; a.a_step = 1;
    a.W = (const q2a_half *) (e->blob + m[A_W]); a.ldw = (int64_t) K * e->kx;
    a.M = M; a.N = N; a.K = K * e->kx;
    a.gelu_tab = e->g<const uint16_t *>(G_GELU);
    a.gelu_c = e->g<const uint16_t *>(G_GELU_C);
    a.T = e->d.T; a.D = e->d.D; a.H = e->d.H; a.TP = e->TP;
    if (e->blk) {
        a.nblk = K / e->blk;
        a.dx = (const float *) (e->blob + m[A_DX]);
        a.dy = K == e->d.D ? e->dyD : e->dyF;
        a.dy_ld = e->dy_ld;
        if (e->gblk == Q2A_BLK_Q6K) {
            a.sc = (const float *) (e->blob + m[A_SC]);
        } else if (e->blk == 256) {
            a.dmin = (const float *) (e->blob + m[A_DMIN]);
            a.wext = (const q2a_half *) (e->blob + m[A_WEXT]);
            a.beta = (const float *) (e->blob + m[A_BETA]);
            a.gamma = (const float *) (e->blob + m[A_GAMMA]);
            a.aext = K == e->d.D ? e->aextD : e->aextF;
        }
    }
    return a;
}

hipEvent_t prof_event(q2a_engine * e) {
    if (!e->pool.empty()) { hipEvent_t ev = e->pool.back(); e->pool.pop_back(); return ev; }
    hipEvent_t ev = nullptr;
    (void) hipEventCreate(&ev);
    return ev;
}

// Launch `call` on stream s; when profiling, bracket it with an event pair attributed to class cls.
#define PLAUNCH(e, s, cls, call)                                                      \
    do {                                                                              \
        q2a_engine::rec r_{cls, nullptr, nullptr};                                    \
        const bool on_ = (e)->prof && (((e)->prof_mask >> (cls)) & 1);                 \
        if (on_) { r_.a = prof_event(e); r_.b = prof_event(e); (void) hipEventRecord(r_.a, s); } \
        hipError_t e_ = (call);                                                       \
        if (e_ != hipSuccess) {                                                       \
            set_err("%s: %s", #call, hipGetErrorString(e_));                        \
            return Q2A_ERR_HIP;                                                       \
        }                                                                             \
        if (on_) { (void) hipEventRecord(r_.b, s); (e)->pending.push_back(r_); }      \
    } while (0)

int ln_mode(const q2a_engine * e) { return e->bf16 ? 4 : e->f32 ? 3 : e->blk == 0 ? 0 : e->blk == 256 ? 1 : 2; }

#define LAUNCH(x)                                                                     \
    do {                                                                              \
        hipError_t e_ = (x);                                                          \
        if (e_ != hipSuccess) {                                                       \
            set_err("%s: %s", #x, hipGetErrorString(e_));                           \
            return Q2A_ERR_HIP;                                                       \
        }                                                                             \
    } while (0)

// the residual rows an encoder block runs on: the windows X [B*T][D] (M = B * T), or with row_start the packed stream
// of a variable-length encode (q2a_varlen_rows), X [M][D] with clip c's rows row_start[c] .. row_start[c+1]-1
struct block_rows {
    int B, M;
    float * X;
    const int32_t * key_len;     // device [B]: per-clip key lengths of the attention, NULL = all T keys
    const int32_t * row_start;   // device [B + 1], NULL = windows
    int r_max;                   // the longest packed segment (host)
    int N_out;                   // packed output rows (q2a_packed_out_rows), where the call lays them out (host)
};

// the attention of `rows`: packed rows take the packed kernel, key lengths alone the key-length one, neither the plain one
hipError_t launch_attention(q2a_attn_args & at, const block_rows & rows, hipStream_t s) {
    at.key_len = rows.key_len;
    at.row_start = rows.row_start;
    at.r_max = rows.r_max;
    return rows.row_start ? q2a_launch_attention_varlen(at, s) : rows.key_len ? q2a_launch_attention_len(at, s) : q2a_launch_attention(at, s);
}

// ---- the four weight GEMMs of a block: their arguments, built here for run_block and for q2a_test_gemm_epi alike
// (outputs into the workspace; the hook replaces the output pointers only)
q2a_gemm_args qkv_gemm(const q2a_engine * e, int l, int M) {
    q2a_gemm_args a = gemm_base(e, l, 0, e->actD, M);
    a.bias = e->lv<const float *>(l, L_BQKV);
    a.qh = e->qh; a.ql = e->ql; a.kh = e->kh; a.kl = e->kl; a.vt = e->vt; a.vtl = e->vtl;
    a.v_rows = e->bf16 ? 0 : 1;   // reference contract: V hi / lo row-major like K (bf16 contract: V^T)
    // ggml_scale(Q, 1/sqrt(dh)) (:2054); the reference-contract attention also wants log2(e) folded in (its
    // softmax runs in log2 units): one f32 multiply by fl(log2 e)/8, 2^-3 being exact
    a.qscale = (1.0f / sqrtf((float) (e->d.D / e->d.H))) * (e->bf16 ? 1.0f : Q2A_LOG2E);
    return a;
}

// the O projection (which 1) and fc2 (which 3): (acc + bias) + X in place on the residual rows X
q2a_gemm_args resid_gemm(const q2a_engine * e, int l, int which, int M, float * X) {
    q2a_gemm_args a = gemm_base(e, l, which, which == 1 ? e->actD : e->actF, M);
    a.bias = e->lv<const float *>(l, which == 1 ? L_BO : L_B2);
    a.outF = X; a.ldo = e->d.D;
    a.part = e->part; a.split_stride = (int64_t) M * e->d.D;
    return a;
}

// fc1: which epilogue the block launches at M rows under fc1 path `path` (q2a_test_fc1_path), and its arguments
int fc1_epi(const q2a_engine * e, int M, int path) {
    const int mode = ln_mode(e);
    if (mode == 0 || mode == 3 || mode == 4) return Q2A_EPI_GELU_H;
    if (mode == 1 && path == 2 && q2a_gemm_wide_tiles(M, e->d.F, e->gblk) &&
        q2a_gemm_pipe8(gemm_base(e, 0, 2, e->actD, M), e->gblk))   // (never Q6_K: its mode has no 8-phase kernel)
        return Q2A_EPI_GELU_Q8K;
    return mode == 1 && path != 1 ? Q2A_EPI_PRE_H : Q2A_EPI_GELU_H;
}

q2a_gemm_args fc1_gemm(const q2a_engine * e, int l, int M, int epi) {
    const dims & d = e->d;
    const int mode = ln_mode(e);
    q2a_gemm_args a = gemm_base(e, l, 2, e->actD, M);
    a.bias = e->lv<const float *>(l, L_B1);
    if (mode == 0 || mode == 3 || mode == 4) {
        // F32 weights: the GELU output is exactly fp16 (LUT), so the fc2 operand is [h | 0 | h] (middle third
        // stays zero from the workspace memset) against [W2h | W2h | W2l]
        a.outH = e->actF; a.ldo = (int64_t) d.F * e->kx; a.o_rpg = M; a.o_gstride = 0; a.o_off = 0;
        a.o_dup = mode == 3 ? 2 * d.F : 0;
    } else if (epi == Q2A_EPI_GELU_Q8K) {
        // fused fc1 + GELU + Q8_K quantization of the fc2 input (one Q8_K block per 256-column tile)
        a.outH = e->actF; a.ldo = d.F; a.qdy = e->dyF; a.qaext = e->aextF;
    } else {
        // the fp16 pre-activation (Q2A_EPI_PRE_H) or the GELU output, exactly fp16-valued (LUT), for the quantizer
        a.outH = (q2a_half *) e->hF; a.ldo = d.F; a.o_rpg = M; a.o_gstride = 0; a.o_off = 0;
    }
    return a;
}

// one pre-LN encoder block on the M rows of `rows` (qwen2-whisper.cpp:2014-2155). Everything but the attention is a
// function of M alone (rows are independent); dy_ld stays the workspace's stride.
int run_block(q2a_engine * e, int l, const block_rows & rows, hipStream_t s) {
    const dims & d = e->d;
    const int M = rows.M;
    float * X = rows.X;
    const int mode = ln_mode(e);
    auto tap = [&](int i, const q2a_half * src, int K) -> hipError_t {
        if (!e->taps[i]) return hipSuccess;
        return hipMemcpyAsync(e->taps[i], src, (size_t) M * K * e->kx * 2, hipMemcpyDeviceToDevice, s);
    };
    q2a_ln_args ln{X, M, d.D, e->lv<const float *>(l, L_LN1W), e->lv<const float *>(l, L_LN1B), mode, e->actD, e->dyD, e->aextD, e->dy_ld};
    PLAUNCH(e, s, Q2A_PROF_LN, q2a_launch_layernorm(ln, s));
    LAUNCH(tap(0, e->actD, d.D));
    {
        const q2a_gemm_args a = qkv_gemm(e, l, M);
        PLAUNCH(e, s, Q2A_PROF_GEMM_QKV, q2a_launch_gemm(a, Q2A_EPI_QKV, e->gblk, s));
    }
    {
        q2a_attn_args at{e->qh, e->ql, e->kh, e->kl, e->vt, rows.B, d.T, d.D, d.H, e->TP, nullptr, nullptr, e->bf16 ? 1 : 0};
        at.vtl = e->vtl;
        at.v_rows = e->bf16 ? 0 : 1;
        if (mode == 0 || mode == 4) at.outH = e->actD; else at.outF = e->attF;
        PLAUNCH(e, s, Q2A_PROF_ATTN, launch_attention(at, rows, s));
        if (mode == 3) {
            const int64_t n = (int64_t) M * d.D;
            PLAUNCH(e, s, Q2A_PROF_QUANT, launch_split3(e->attF, e->actD, d.D, n, s));
        } else if (mode == 1 || mode == 2) {
            q2a_quant_args qa{e->attF, nullptr, M, d.D, mode, e->actD, e->dyD, e->aextD, e->dy_ld};
            PLAUNCH(e, s, Q2A_PROF_QUANT, q2a_launch_quant_act(qa, s));
        }
    }
    LAUNCH(tap(1, e->actD, d.D));
    {
        const q2a_gemm_args a = resid_gemm(e, l, 1, M, X);
        PLAUNCH(e, s, Q2A_PROF_GEMM_O, q2a_launch_gemm(a, Q2A_EPI_RESID, e->gblk, s));
    }
    q2a_ln_args ln2{X, M, d.D, e->lv<const float *>(l, L_LN2W), e->lv<const float *>(l, L_LN2B), mode, e->actD, e->dyD, e->aextD, e->dy_ld};
    PLAUNCH(e, s, Q2A_PROF_LN, q2a_launch_layernorm(ln2, s));
    LAUNCH(tap(2, e->actD, d.D));
    {
        const int epi = fc1_epi(e, M, e->fc1_path);
        const q2a_gemm_args a = fc1_gemm(e, l, M, epi);
        // the fused epilogue is a Q4_K-layout kernel (blk); every other fc1 launch goes by the engine's GEMM mode
        PLAUNCH(e, s, Q2A_PROF_GEMM_FC1, q2a_launch_gemm(a, epi, epi == Q2A_EPI_GELU_Q8K ? e->blk : e->gblk, s));
        if (epi == Q2A_EPI_PRE_H) {
            // fc1 wrote its fp16 pre-activation (plain stores); the Q8_K quantizer of the fc2 input applies the
            // GELU table from LDS on the way (same codes as the GELU epilogue + quantizer below)
            PLAUNCH(e, s, Q2A_PROF_QUANT, q2a_launch_gelu_quant_q8k(a.outH, M, d.F, e->g<const uint16_t *>(G_GELU), e->actF,
                                                                   e->dyF, e->aextF, e->dy_ld, s));
        } else if (epi == Q2A_EPI_GELU_H && (mode == 1 || mode == 2)) {
            // GELU output is exactly fp16-valued (LUT): keep it as fp16, then quantize for fc2
            q2a_quant_args qa{nullptr, a.outH, M, d.F, mode, e->actF, e->dyF, e->aextF, e->dy_ld};
            PLAUNCH(e, s, Q2A_PROF_QUANT, q2a_launch_quant_act(qa, s));
        }
    }
    LAUNCH(tap(3, e->actF, d.F));
    {
        const q2a_gemm_args a = resid_gemm(e, l, 3, M, X);
        PLAUNCH(e, s, Q2A_PROF_GEMM_FC2, q2a_launch_gemm(a, Q2A_EPI_RESID, e->gblk, s));
    }
    return Q2A_OK;
}

int ensure_frange(q2a_engine * e, hipStream_t s) {
    if (e->frange) return Q2A_OK;
    if (hipMalloc((void **) &e->frange, (size_t) e->d.M * sizeof(int2)) != hipSuccess) {
        (void) hipGetLastError();
        e->frange = nullptr;
        set_err("filter-range allocation failed");
        return Q2A_ERR_OOM;
    }
    LAUNCH(q2a_launch_filter_ranges(e->g<const float *>(G_FILT), e->d.M, 201, e->frange, s));
    return Q2A_OK;
}

// the mel kernel's arguments for the B clips described by the device rows `dev` (after ensure_frange)
q2a_mel_args mel_args(const q2a_engine * e, const float * pcm, int64_t stride, const meta_rows & dev, int B, int max_frames) {
    const dims & d = e->d;
    q2a_mel_args ma;
    ma.pcm = pcm; ma.pcm_stride = stride; ma.n_samples = dev.nsamp; ma.seek = dev.seek; ma.n_clips = B;
    ma.n_mel = d.M; ma.n_bins = 201; ma.n_frames_win = d.TM; ma.max_frames = max_frames;
    ma.filters = e->g<const float *>(G_FILT); ma.tab = e->g<const float *>(G_TAB);
    ma.frange = e->frange;
    ma.mel = e->mel; ma.clip_max = dev.clip_max; ma.xc1 = e->xc1; ma.xc_f32 = e->f32 ? 1 : 0;
    return ma;
}

// The clips of a call: B clips in device memory, clip c at data + c * stride (stride 0: every clip reads the same
// array), and host arrays of B entries. PCM (pcm_input): len[c] samples, encoded from offs[c] ms (offs NULL: offset_ms
// for every clip). Log-mel (mel_input): the caller's normalised mel [n_mels][ld] with len[c] frames, encoded from frame
// seek[c] (NULL: 0). A host entry point describes its clips the same way with data NULL (host_clips).
struct clip_input {
    bool mel;
    int B;
    const float * data;
    int64_t stride;
    const int32_t * len;
    const int32_t * offs;       // PCM
    int offset_ms;
    int64_t ld;                 // log-mel
    const int32_t * seek;
};
clip_input pcm_input(const float * pcm, int64_t stride, const int32_t * n_samples, int B, const int32_t * offs, int offset_ms = 0) {
    clip_input in{};
    in.B = B; in.data = pcm; in.stride = stride; in.len = n_samples; in.offs = offs; in.offset_ms = offset_ms;
    return in;
}
clip_input mel_input(const float * mel, int64_t clip_stride, int64_t ld, const int32_t * n_len, const int32_t * seek, int B) {
    clip_input in{};
    in.mel = true; in.B = B; in.data = mel; in.stride = clip_stride; in.len = n_len; in.ld = ld; in.seek = seek;
    return in;
}

// Where a call's result goes, exactly one of: the windows out [B][TO][D] (window_sink); the valid output rows of all
// clips packed (q2a_packed_out_rows) as f32 into embd [rows_cap][D] and / or, through the projector, into feat
// [rows_cap][d_out] (packed_sink); the features as dst's type into dst's rows, clip c's from row clip_row[c] on (host
// [B]; NULL: packed), embd [rows_cap][D] still the packed f32 rows (rows_sink); or into dst's rows where ids->input_ids
// holds the audio token, the text rows gathered from ids->embed_table (ids_sink). All but the first are the
// audio-feature tail of a variable-length encode.
struct out_sink {
    enum { WINDOWS, PACKED, ROWS, IDS } kind;
    float * out;
    float * feat;
    float * embd;               // NULL: not written
    int64_t rows_cap;
    const q2a_feat_dst * dst;
    const int32_t * clip_row;
    const q2a_embeds_src * ids;
    bool features() const { return kind != WINDOWS; }
    bool to_dst() const { return kind == ROWS || kind == IDS; }
};
out_sink window_sink(float * out) {
    out_sink k{};
    k.kind = out_sink::WINDOWS; k.out = out;
    return k;
}
out_sink packed_sink(float * feat, float * embd, int64_t rows_cap) {
    out_sink k{};
    k.kind = out_sink::PACKED; k.feat = feat; k.embd = embd; k.rows_cap = rows_cap;
    return k;
}
out_sink rows_sink(const q2a_feat_dst * dst, const int32_t * clip_row, float * embd, int64_t rows_cap) {
    out_sink k{};
    k.kind = out_sink::ROWS; k.dst = dst; k.clip_row = clip_row; k.embd = embd; k.rows_cap = rows_cap;
    return k;
}
out_sink ids_sink(const q2a_feat_dst * dst, const q2a_embeds_src * ids, float * embd, int64_t rows_cap) {
    out_sink k{};
    k.kind = out_sink::IDS; k.dst = dst; k.ids = ids; k.embd = embd; k.rows_cap = rows_cap;
    return k;
}

// mel + conv frontend: PCM or log-mel -> X [B*T][D] (conv graph qwen2-whisper.cpp:1892-1952 + pe add :2005); the same
// conv launches after either mel producer. The per-clip lengths and seeks are in the call's device rows.
int run_frontend(q2a_engine * e, const clip_input & in, int max_frames, hipStream_t s) {
    const dims & d = e->d;
    const int B = in.B;
    const meta_rows dev(e->meta, B);
    if (in.mel) {
        const q2a_mel_ingest_args ia{in.data, in.stride, in.ld, dev.nsamp, dev.seek, B, d.M, d.TM, e->xc1, e->f32 ? 1 : 0};
        PLAUNCH(e, s, Q2A_PROF_MEL, q2a_launch_mel_ingest(ia, s));
    } else {
        LAUNCH(hipMemsetAsync(dev.clip_max, 0x80, (size_t) B * 4, s));
        if (int rc = ensure_frange(e, s)) return rc;
        const q2a_mel_args ma = mel_args(e, in.data, in.stride, dev, B, max_frames);
        PLAUNCH(e, s, Q2A_PROF_MEL, q2a_launch_mel(ma, s));
    }
    const int P1 = 3, P2 = e->f32 ? 2 : 1;   // operand parts per mel row / per conv1 output row
    // both convs sum each 64-deep K-step's MFMA partial in f64 (Q2A_BLK_EXACT): within rounding of the exact dot
    // product, where a plain f32 MFMA chain carried twice the reference builds' own conv error
    {   // conv1: implicit GEMM, A row t = xc1 rows t..t+2 of its clip (3 x P1 x M halves), K = 3 P1 M
        q2a_gemm_args a;
        memset(&a, 0, sizeof(a));
        a.A = e->xc1; a.lda = P1 * d.M; a.a_rpg = d.TM; a.a_gstride = d.TM + 2; a.a_step = 1;
        a.W = e->g<const q2a_half *>(G_CONV1_W); a.ldw = 3 * P1 * d.M;
        a.M = B * d.TM; a.N = d.D; a.K = 3 * P1 * d.M;
        a.bias = e->g<const float *>(G_CONV1_B);
        a.outH = e->y1; a.ldo = (int64_t) P2 * d.D; a.o_rpg = d.TM; a.o_gstride = d.TM + 1; a.o_off = 1;
        a.o_dup = e->f32 ? d.D : 0;
        a.gelu_tab = e->g<const uint16_t *>(G_GELU);
        a.gelu_c = e->g<const uint16_t *>(G_GELU_C);
        PLAUNCH(e, s, Q2A_PROF_CONV1, q2a_launch_gemm(a, Q2A_EPI_GELU_H, Q2A_BLK_EXACT, s));
    }
    {   // conv2 (stride 2): A row t = y1 rows 2t..2t+2 (inputs 2t-1..2t+1), K = 3D; + pe
        q2a_gemm_args a;
        memset(&a, 0, sizeof(a));
        a.A = e->y1; a.lda = (int64_t) P2 * d.D; a.a_rpg = d.T; a.a_gstride = d.TM + 1; a.a_step = 2;
        a.W = e->g<const q2a_half *>(G_CONV2_W); a.ldw = 3 * P2 * d.D;
        a.M = B * d.T; a.N = d.D; a.K = 3 * P2 * d.D;
        a.bias = e->g<const float *>(G_CONV2_B);
        a.outF = e->X; a.ldo = d.D; a.pe = e->g<const float *>(G_PE); a.T = d.T;
        a.gelu_tab = e->g<const uint16_t *>(G_GELU);
        a.gelu_c = e->g<const uint16_t *>(G_GELU_C);
        PLAUNCH(e, s, Q2A_PROF_CONV2, q2a_launch_gemm(a, Q2A_EPI_CONV2, Q2A_BLK_EXACT, s));
    }
    return Q2A_OK;
}

// the three encode families: q2a_encode_device / _host (all T keys), the padded entry points (per-clip key lengths in
// the attention, the blocks on all B*T rows) and the variable-length ones (the blocks on the packed valid rows)
enum encode_kind { ENC_PLAIN, ENC_PADDED, ENC_PACKED };

// whisper_encoder_output_with_state's too-short rule (:2356-2365) for a clip of n samples encoded from frame seek
bool clip_has_window(const q2a_engine * e, int n, int seek) {
    const int n_len_org = 1 + (n + 200 - 400) / 160;   // mel.n_len_org (:2613), C truncation
    return n > 200 && (e->force_encode || !(n_len_org < seek + 100));
}

// What a call derives from each clip, in one host pass that checks nothing (the range checks are prepare_meta's): the
// frame its window starts at, and whether it is encoded (PCM: the too-short rule; log-mel: always). features_check,
// prepare_meta and the out_len of encode() all read these.
struct clip_facts {
    std::vector<int32_t> seek;
    std::vector<uint8_t> ok;
};
clip_facts resolve_clips(const q2a_engine * e, const clip_input & in) {
    clip_facts f;
    f.seek.resize(in.B);
    f.ok.resize(in.B);
    for (int i = 0; i < in.B; ++i) {
        f.seek[i] = in.mel ? (in.seek ? in.seek[i] : 0) : (in.offs ? in.offs[i] : in.offset_ms) / 10;
        f.ok[i] = in.mel || clip_has_window(e, in.len[i], f.seek[i]);
    }
    return f;
}

// the packed layout of a call (host): q2a_varlen_rows over the clips' key lengths, with no rows for a clip whose
// clip_ok entry is 0 (clip_ok NULL: every clip has rows). Writes row_start (rows.B + 1 entries), rows.M (0: no clip is
// encoded) and rows.r_max; with out_start (rows.B + 1 entries) also the packed output layout of the same lengths
// (q2a_packed_out_rows) and rows.N_out
int packed_layout_of(const q2a_engine * e, const int32_t * key_len, const int32_t * clip_ok, int32_t * row_start, block_rows & rows,
                     int32_t * out_start = nullptr) {
    const int B = rows.B;
    std::vector<int32_t> kl(key_len, key_len + B);
    if (clip_ok)
        for (int c = 0; c < B; ++c) if (!clip_ok[c]) kl[c] = 0;
    const int64_t m = q2a_varlen_rows(kl.data(), B, e->d.T, row_start);
    const int64_t n = out_start ? q2a_packed_out_rows(kl.data(), B, e->d.T, out_start) : 0;
    if (m < 0 || n < 0) { set_err("key lengths outside 0..%d", e->d.T); return Q2A_ERR_ARG; }
    rows.N_out = (int) n;
    rows.M = (int) m;
    rows.r_max = 0;
    for (int c = 0; c < B; ++c) rows.r_max = std::max(rows.r_max, row_start[c + 1] - row_start[c]);
    return Q2A_OK;
}

// per-clip metadata (host): whisper_encoder_output_with_state's seek / too-short logic (:2356-2365), uploaded in one
// copy with what the kind adds: 3 B words (plain), 5 B with the key lengths (padded), 6 B + 1 with their packed layout
// (packed), 7 B + 2 with the packed output layout behind it (the audio-feature tail). `rows` receives what the blocks
// of the call run on.
int prepare_meta(q2a_engine * e, encode_kind kind, const clip_input & in, const clip_facts & f, const int32_t * kl, const out_sink & sink,
                 int32_t * status, hipStream_t s, int & max_frames, block_rows & rows) {
    const int B = in.B;
    const meta_rows dev(e->meta, B);
    rows = block_rows{B, B * e->d.T, e->X, kind == ENC_PLAIN ? nullptr : dev.key_len, nullptr, 0};
    max_frames = 0;
    const auto last = kind == ENC_PLAIN ? &meta_rows::clip_max : kind == ENC_PADDED ? &meta_rows::row_start
                      : !sink.features() ? &meta_rows::out_start : sink.clip_row ? &meta_rows::end_to : &meta_rows::end;
    return upload_meta(e, B, &meta_rows::nsamp, last, s, [&](const meta_rows & mh) -> int {
        if (in.mel && in.stride != 0 && in.stride < e->d.M * in.ld) { set_err("clip_stride %lld below n_mels * ld", (long long) in.stride); return Q2A_ERR_ARG; }
        for (int i = 0; i < B; ++i) {
            if (f.seek[i] < 0) { set_err("clip %d: negative offset", i); return Q2A_ERR_ARG; }
            const int n = in.len[i];
            // (log-mel: n is n_len, into the nsamp row. PCM: at most the stride, unless the clips share one array)
            if (in.mel ? n < 1 || n > in.ld : n < 0 || (in.stride > 0 && n > in.stride)) {
                if (in.mel) set_err("clip %d: n_len %d outside 1..ld", i, n); else set_err("clip %d: bad n_samples %d", i, n);
                return Q2A_ERR_ARG;
            }
            const bool ok = f.ok[i];
            mh.nsamp[i] = ok ? n : 0;
            mh.seek[i] = f.seek[i];
            mh.clip_ok[i] = ok ? 1 : 0;
            if (status) status[i] = ok ? Q2A_CLIP_ENCODED : Q2A_CLIP_SKIPPED;
            max_frames = std::max(max_frames, (int) (((int64_t) mh.nsamp[i] + 480000) / 160));
            // the clip_max row lies between clip_ok and the key lengths, inside the copy: it is device-written, and
            // run_frontend resets it after this copy on the same stream, to the value uploaded here
            if (kind != ENC_PLAIN) { mh.clip_max[i] = (int32_t) 0x80808080u; mh.key_len[i] = kl[i]; }
            if (sink.clip_row) mh.clip_row[i] = sink.clip_row[i];
        }
        if (kind != ENC_PACKED) return Q2A_OK;
        rows.X = e->Xp;
        rows.row_start = dev.row_start;
        // a clip that is not encoded has no rows
        return packed_layout_of(e, mh.key_len, mh.clip_ok, mh.row_start, rows, sink.features() ? mh.out_start : nullptr);
    });
}

// the rows of a test hook: the windows, for ENC_PADDED with key lengths (host array, checked) uploaded into the key_len
// row, for ENC_PACKED with their packed layout behind them in the same copy (every clip has rows; rows.X is left to the
// caller, the attention hook has no residual stream)
int hook_rows(q2a_engine * e, encode_kind kind, const int32_t * key_len, int B, hipStream_t s, block_rows & rows,
              bool out_layout = false /* ENC_PACKED: the packed output layout too */) {
    const meta_rows dev(e->meta, B);
    rows = block_rows{B, B * e->d.T, e->X, nullptr, nullptr, 0};
    if (kind == ENC_PLAIN) return Q2A_OK;
    if (e->bf16) { set_err("key lengths: reference activation contract only"); return Q2A_ERR_UNSUPPORTED; }
    for (int c = 0; c < B; ++c)
        if (key_len[c] < 1 || key_len[c] > e->d.T) { set_err("clip %d: key_len %d outside 1..%d", c, key_len[c], e->d.T); return Q2A_ERR_ARG; }
    const bool packed = kind == ENC_PACKED;
    rows.key_len = dev.key_len;
    if (packed) { rows.X = nullptr; rows.row_start = dev.row_start; }
    const auto last = !packed ? &meta_rows::row_start : out_layout ? &meta_rows::end : &meta_rows::out_start;
    return upload_meta(e, B, &meta_rows::key_len, last, s, [&](const meta_rows & mh) -> int {
        memcpy(mh.key_len, key_len, (size_t) B * 4);
        return packed ? packed_layout_of(e, key_len, nullptr, mh.row_start, rows, out_layout ? mh.out_start : nullptr) : Q2A_OK;
    });
}

// out [B][TO][D]: rows >= key_len[c] / 2 of clip c (every row of a clip that was not encoded) := 0
__global__ void k_zero_tail_rows(float * out, const int32_t * key_len, const int32_t * clip_ok, int TO, int D) {
    const int c = blockIdx.y;
    const int n4 = TO * D / 4, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int valid = clip_ok[c] ? key_len[c] / 2 : 0;
    if (i * 4 / D >= valid) ((float4 *) (out + (int64_t) c * TO * D))[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}
hipError_t launch_zero_tail_rows(float * out, const int32_t * key_len, const int32_t * clip_ok, int B, int TO, int D, hipStream_t s) {
    if (D % 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_zero_tail_rows, dim3((unsigned) ((TO * D / 4 + 255) / 256), (unsigned) B), dim3(256), 0, s, out, key_len, clip_ok, TO, D);
    return hipGetLastError();
}

// the per-clip key lengths of a padded or variable-length encode: the caller's (checked), or the enc_len of
// q2a_valid_lengths (PCM) / q2a_mel_valid_lengths (log-mel)
int key_lens(const q2a_engine * e, const clip_input & in, const int32_t * key_len, std::vector<int32_t> & kl) {
    kl.resize(in.B);
    for (int c = 0; c < in.B; ++c) {
        if (key_len) {
            kl[c] = key_len[c];
            if (kl[c] < 1 || kl[c] > e->d.T) { set_err("clip %d: key_len %d outside 1..%d", c, kl[c], e->d.T); return Q2A_ERR_ARG; }
        } else if ((in.mel ? q2a_mel_valid_lengths(in.len[c], in.seek ? in.seek[c] : 0, e->d.T, &kl[c], nullptr)
                           : q2a_valid_lengths(in.len[c], in.offs ? in.offs[c] : in.offset_ms, e->d.T, &kl[c], nullptr)) != Q2A_OK) {
            set_err(in.mel ? "clip %d: bad n_len %d or seek" : "clip %d: bad n_samples %d or offset", c, in.len[c]);
            return Q2A_ERR_ARG;
        }
    }
    return Q2A_OK;
}

// ---- variable-length encode: the blocks run on the valid rows only ------------------------------
// the packed residual buffer, for as many clips as the workspace holds (its own allocation: engines that never run a
// variable-length encode do not pay for it)
int ensure_packed(q2a_engine * e) {
    if (e->Xp && e->xp_clips >= e->cap_clips) return Q2A_OK;
    HIP_TRY(hipDeviceSynchronize());   // earlier calls may still read the old buffer, on any stream
    if (e->Xp) { (void) hipFree(e->Xp); e->Xp = nullptr; e->xp_clips = 0; }
    const size_t bytes = (size_t) e->cap_clips * e->d.T * e->d.D * 4;
    if (hipMalloc((void **) &e->Xp, bytes) != hipSuccess) {
        (void) hipGetLastError();
        e->Xp = nullptr;
        set_err("packed residual allocation of %.2f GB for %d clips failed", bytes / 1e9, e->cap_clips);
        return Q2A_ERR_OOM;
    }
    e->xp_clips = e->cap_clips;
    return Q2A_OK;
}

// rows 0 .. seg_rows[c]-1 of clip c's window X [B][T][D] -> packed rows row_start[c] .. of Xp (whole rows, float4)
__global__ void k_gather_rows(const float * X, float * Xp, const int32_t * row_start, int T, int D) {
    const int c = blockIdx.y;
    const int r0 = row_start[c], n4 = (row_start[c + 1] - r0) * (D / 4);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    ((float4 *) (Xp + (int64_t) r0 * D))[i] = ((const float4 *) (X + (int64_t) c * T * D))[i];
}
hipError_t launch_gather_rows(const float * X, float * Xp, const int32_t * row_start, int B, int T, int D, int r_max, hipStream_t s) {
    if (D % 4 || r_max <= 0 || r_max > T) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_gather_rows, dim3((unsigned) (((int64_t) r_max * (D / 4) + 255) / 256), (unsigned) B), dim3(256), 0, s,
                       X, Xp, row_start, T, D);
    return hipGetLastError();
}

// the key-length kinds exist for the reference activation contract only
int lens_supported(const q2a_engine * e, encode_kind kind) {
    if (kind == ENC_PLAIN || !e->bf16) return Q2A_OK;
    set_err("%s: reference activation contract only", kind == ENC_PADDED ? "padded encode" : "variable-length encode");
    return Q2A_ERR_UNSUPPORTED;
}

// ---- the projector's GEMM: q2a_projector_apply and the audio-feature tail of encode() build it here ---------------
// the activation operand of a call of `rows` rows, in the handle's one workspace: A [rows][d_in] 2-byte elements, and for
// the block-quantized weights d [d_in/blk][ld] and (Q8_K) the block sums [d_in/256][ld][16], ld = rows rounded up to 256
struct proj_operand {
    q2a_half * A;
    float * dy;
    q2a_half * aext;
    int ld;
    int32_t * map;   // device row map [rows] of a _to call with clip_row (proj_workspace with_map), else NULL
    // a call with input_ids (proj_workspace ids_tokens > 0; it has the map too): the compaction's count per chunk, and
    // four report words for a caller that passes no report_dev
    int32_t * chunk_count;
    int32_t * report;
};
// the conversion the weight type asks for: 0 fp16, 1 Q8_K, 2 Q8_0 (q2a_ln_args' modes)
int proj_mode(const q2a_projector * p) { return p->blk == 0 ? 0 : p->blk == 256 ? 1 : 2; }

// grows the workspace (after everything queued on s: calls on one handle are ordered on one stream) and cuts it up
int proj_workspace(q2a_projector * p, int64_t rows, hipStream_t s, proj_operand & o, bool with_map = false, int64_t ids_tokens = 0) {
    with_map = with_map || ids_tokens > 0;
    const int K = p->d_in, blk = p->blk;
    const int64_t MP = (rows + 255) / 256 * 256;
    const size_t a_bytes = ((size_t) rows * K * 2 + 255) & ~size_t(255);
    const size_t dy_bytes = blk ? ((size_t) (K / blk) * MP * 4 + 255) & ~size_t(255) : 0;
    const size_t ae_bytes = blk == 256 ? (size_t) (K / 256 + 1) * MP * 32 : 0;   // (Q6_K: written by the quantizer, unread)
    const size_t map_bytes = with_map ? (size_t) MP * 4 : 0;
    const size_t cc_bytes = ids_tokens > 0 ? (((size_t) (ids_tokens + Q2A_IDS_CHUNK - 1) / Q2A_IDS_CHUNK * 4 + 255) & ~size_t(255)) : 0;
    const size_t need = a_bytes + dy_bytes + ae_bytes + map_bytes + cc_bytes + (ids_tokens > 0 ? 256 : 0);
    if (need > p->ws_bytes) {
        HIP_TRY(hipStreamSynchronize(s));
        if (p->ws) (void) hipFree(p->ws);
        p->ws = nullptr; p->ws_bytes = 0;
        if (hipMalloc(&p->ws, need) != hipSuccess) { (void) hipGetLastError(); set_err("projector workspace of %zu bytes", need); return Q2A_ERR_OOM; }
        p->ws_bytes = need;
    }
    o.A = (q2a_half *) p->ws;
    o.dy = (float *) ((char *) p->ws + a_bytes);
    o.aext = (q2a_half *) ((char *) p->ws + a_bytes + dy_bytes);
    o.ld = (int) MP;
    o.map = with_map ? (int32_t *) ((char *) p->ws + a_bytes + dy_bytes + ae_bytes) : nullptr;
    o.chunk_count = ids_tokens > 0 ? (int32_t *) ((char *) p->ws + a_bytes + dy_bytes + ae_bytes + map_bytes) : nullptr;
    o.report = ids_tokens > 0 ? (int32_t *) ((char *) p->ws + a_bytes + dy_bytes + ae_bytes + map_bytes + cc_bytes) : nullptr;
    return Q2A_OK;
}

// y [M][d_out] f32 = operand o (M rows) . W^T + bias
q2a_gemm_args proj_gemm(const q2a_projector * p, int M, const proj_operand & o, float * y) {
    const int K = p->d_in, N = p->d_out, blk = p->blk;
    q2a_gemm_args a;
    memset(&a, 0, sizeof(a));
    const char * w = (const char *) p->wdev;
    a.A = o.A; a.lda = K; a.a_rpg = M; a.a_gstride = 0; a.a_step = 1;
    a.W = (const q2a_half *) (w + p->off[A_W]); a.ldw = K;
    a.M = M; a.N = N; a.K = K;
    a.outF = y; a.ldo = N;
    a.bias = p->bias; a.store_bias = 1;
    a.gelu_tab = p->gelu;
    if (blk) {
        a.nblk = K / blk;
        a.dx = (const float *) (w + p->off[A_DX]);
        a.dy = o.dy; a.dy_ld = o.ld;
        if (p->gblk == Q2A_BLK_Q6K) {
            a.sc = (const float *) (w + p->off[A_SC]);
        } else if (blk == 256) {
            a.dmin = (const float *) (w + p->off[A_DMIN]);
            a.wext = (const q2a_half *) (w + p->off[A_WEXT]);
            a.beta = (const float *) (w + p->off[A_BETA]);
            a.gamma = (const float *) (w + p->off[A_GAMMA]);
            a.aext = o.aext;
        }
    }
    return a;
}

// y = the same GEMM with the row-map epilogue: row m of the operand to row row_map[m] (NULL: m) of dst, in dst's type
q2a_gemm_args proj_gemm_to(const q2a_projector * p, int M, const proj_operand & o, const q2a_feat_dst & dst, const int32_t * row_map) {
    q2a_gemm_args a = proj_gemm(p, M, o, nullptr);
    a.out_rows = dst.base; a.out_ld = dst.ld; a.n_rows = (int) dst.n_rows; a.out_dt = dst.dtype; a.row_map = row_map;
    return a;
}

// a feature destination against the projector's d_out (include/q2a_encoder.h, q2a_feat_dst)
int feat_dst_check_cols(int d_out, const q2a_feat_dst * dst) {
    const int es = dst->dtype == Q2A_DT_F32 ? 4 : (dst->dtype == Q2A_DT_F16 || dst->dtype == Q2A_DT_BF16) ? 2 : 0;
    if (!es || dst->reserved != 0) { set_err("feature destination: dtype %d, reserved %d", dst->dtype, dst->reserved); return Q2A_ERR_ARG; }
    if (!dst->base || ((uintptr_t) dst->base & 15)) { set_err("feature destination: base must be 16-byte aligned"); return Q2A_ERR_ARG; }
    if (dst->ld < d_out || (dst->ld * es) % 16 != 0) {
        set_err("feature destination: ld %lld with d_out %d (ld * %d bytes must be a multiple of 16)", (long long) dst->ld, d_out, es);
        return Q2A_ERR_ARG;
    }
    if (dst->n_rows < 0 || dst->n_rows > INT32_MAX) { set_err("feature destination: n_rows %lld", (long long) dst->n_rows); return Q2A_ERR_ARG; }
    return Q2A_OK;
}

int feat_dst_check(const q2a_projector * p, const q2a_feat_dst * dst) {
    if (!p || !dst) { set_err("feature destination: it goes with a projector, and both are required"); return Q2A_ERR_ARG; }
    return feat_dst_check_cols(p->d_out, dst);
}

// ---- inputs_embeds: the row map from input_ids and the text-row gather (q2a_embeds.hip) ---------------------------
int dt_size(int dtype) { return dtype == Q2A_DT_F32 ? 4 : 2; }

// a q2a_embeds_src against a checked destination of d_out columns (include/q2a_encoder.h)
int embeds_src_check(const q2a_embeds_src * src, const q2a_feat_dst & dst, int d_out) {
    if (!src) { set_err("inputs_embeds: src is required"); return Q2A_ERR_ARG; }
    if ((src->ids_width != 4 && src->ids_width != 8) || src->reserved != 0) {
        set_err("inputs_embeds: ids_width %d, reserved %d", src->ids_width, src->reserved);
        return Q2A_ERR_ARG;
    }
    if (!src->input_ids || ((uintptr_t) src->input_ids & (uintptr_t) (src->ids_width - 1))) {
        set_err("inputs_embeds: input_ids must be non-NULL and aligned to ids_width");
        return Q2A_ERR_ARG;
    }
    if (src->n_tokens < 1 || src->n_tokens > Q2A_IDS_MAX_TOKENS || src->n_tokens != dst.n_rows) {
        set_err("inputs_embeds: n_tokens %lld (1 .. 2^24) with a destination of %lld rows", (long long) src->n_tokens, (long long) dst.n_rows);
        return Q2A_ERR_ARG;
    }
    if (src->embed_table) {
        const int es = dt_size(dst.dtype);
        if (((uintptr_t) src->embed_table & 15) || src->table_ld < d_out || (src->table_ld * es) % 16 != 0 || src->vocab < 1) {
            set_err("inputs_embeds: embedding table: 16-byte aligned, table_ld %lld >= d_out %d with table_ld * %d bytes a multiple of 16, vocab %lld >= 1",
                    (long long) src->table_ld, d_out, es, (long long) src->vocab);
            return Q2A_ERR_ARG;
        }
    }
    return Q2A_OK;
}

q2a_ids_args ids_args(const void * ids, int width, int64_t n_tokens, int64_t audio_id, int n_feat, const proj_operand & o, int32_t * report) {
    return {ids, width, n_tokens, audio_id, n_feat, o.chunk_count, o.map, report ? report : o.report};
}

// the text rows of a checked src into dst (nothing without a table); the report words 2 and 3 must already be written
hipError_t launch_embeds_gather(const q2a_embeds_src & src, const q2a_feat_dst & dst, int d_out, int32_t * report, hipStream_t s) {
    if (!src.embed_table) return hipSuccess;
    const int es = dt_size(dst.dtype);
    const q2a_embed_gather_args ga{src.input_ids, src.ids_width, src.n_tokens, src.audio_token_id, src.embed_table, src.vocab,
                                   src.table_ld * es, dst.base, dst.ld * es, (int64_t) d_out * es, report};
    return q2a_launch_embed_gather(ga, s);
}

// map[n] = clip_row[c] + (n - out_start[c]) for the packed output rows n of clip c: the device row map of a _to call,
// from the rows of the call's one metadata upload
__global__ void k_feat_row_map(const int32_t * out_start, const int32_t * clip_row, int32_t * map) {
    const int c = blockIdx.y, n0 = out_start[c], len = out_start[c + 1] - n0;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < len) map[n0 + j] = clip_row[c] + j;
}
hipError_t launch_feat_row_map(const int32_t * out_start, const int32_t * clip_row, int32_t * map, int B, int max_len, hipStream_t s) {
    if (B <= 0 || max_len <= 0 || !map) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_feat_row_map, dim3((unsigned) ((max_len + 255) / 256), (unsigned) B), dim3(256), 0, s, out_start, clip_row, map);
    return hipGetLastError();
}

// the checks of the audio-feature tail, made before anything is launched or written: the outputs, the projector, and the
// packed rows against rows_cap (the clips the too-short rule skips have none); for the _to form the destination and
// q2a_feat_rows' checks of the clips' ranges in it, rows_cap then bounding embd alone
int features_check(const q2a_engine * e, const clip_facts & f, const int32_t * kl, const out_sink & k, const q2a_projector * proj) {
    if (k.to_dst()) {
        if (int rc = feat_dst_check(proj, k.dst)) return rc;
        if (k.kind == out_sink::IDS)
            if (int rc = embeds_src_check(k.ids, *k.dst, proj->d_out)) return rc;
    } else {
        if (!k.feat && !k.embd) { set_err("audio features: feat and embd are both NULL"); return Q2A_ERR_ARG; }
        if (proj ? !k.feat : k.feat != nullptr) { set_err("audio features: feat goes with a projector, and only with one"); return Q2A_ERR_ARG; }
    }
    if (proj && (proj->device != e->device || proj->d_in != e->d.D)) {
        set_err("audio features: projector on device %d with d_in %d, engine on device %d with n_audio_state %d", proj->device,
                proj->d_in, e->device, e->d.D);
        return Q2A_ERR_ARG;
    }
    const int B = (int) f.ok.size();
    std::vector<int32_t> ol(B);
    int64_t n_tot = 0;
    for (int i = 0; i < B; ++i) {
        ol[i] = f.ok[i] ? kl[i] / 2 : 0;
        n_tot += ol[i];
    }
    if (k.kind == out_sink::IDS) {
        // (no clip ranges: the k-th feature row goes where the k-th audio token is, a row without one is dropped)
        if (n_tot > (1 << 30) / 4) { set_err("audio features: %lld output rows", (long long) n_tot); return Q2A_ERR_ARG; }
    } else if (k.kind == out_sink::ROWS && q2a_feat_rows(ol.data(), k.clip_row, B, k.dst->n_rows, nullptr) < 0) {
        set_err("audio features: a clip's destination rows start below 0, end past n_rows %lld, or overlap another clip's",
                (long long) k.dst->n_rows);
        return Q2A_ERR_ARG;
    }
    if (k.to_dst() && !k.embd) return Q2A_OK;   // (rows_cap bounds embd alone)
    if (n_tot > k.rows_cap) { set_err("audio features: %lld output rows, rows_cap %lld", (long long) n_tot, (long long) k.rows_cap); return Q2A_ERR_ARG; }
    return Q2A_OK;
}

// One encode of any kind: metadata, front end, the L blocks, pool + final LayerNorm into out [B][TO][D].
// ENC_PADDED: the attention of every block masks keys >= kl[c] and output rows >= kl[c] / 2 (every row of a skipped
// clip) are zeros; everything else runs over all B*T rows as in ENC_PLAIN, which leaves a skipped clip's rows alone.
// ENC_PACKED: after the front end (full windows, unchanged) the valid rows of every clip (each rounded up to the
// attention's 16-query block) are gathered into one [M_tot][D] stream, the blocks run on those M_tot rows, and the pool
// reads them back into out, zeros past each clip's valid length. Row for row the padded encode's operations: the same
// bytes.
// ENC_PACKED with a feature sink (q2a_audio_features_*, q2a_inputs_embeds_*): the same up to and including the blocks;
// then the pool kernel writes the valid output rows alone, packed (q2a_packed_out_rows), as f32 and / or as the
// projector GEMM's A operand, and that GEMM writes the features.
// kl: the checked key lengths (ENC_PADDED, ENC_PACKED). out_len: NULL, or the clips' valid output rows (the same
// kinds). status: NULL, or Q2A_CLIP_* per clip.
int encode(q2a_engine * e, encode_kind kind, const clip_input & in, const int32_t * kl, const out_sink & sink, q2a_projector * proj,
           int32_t * out_len, int32_t * status, hipStream_t s) {
    const dims & d = e->d;
    const int B = in.B;
    const bool feats = sink.features();
    if (B <= 0 || !in.data || !in.len || (feats ? kind != ENC_PACKED : !sink.out) || (kind != ENC_PLAIN && !kl)) { set_err("invalid arguments"); return Q2A_ERR_ARG; }
    if (in.offset_ms < 0) { set_err("offset_ms must be >= 0"); return Q2A_ERR_ARG; }
    int rc = lens_supported(e, kind);
    if (rc) return rc;
    const clip_facts facts = resolve_clips(e, in);
    if (feats && (rc = features_check(e, facts, kl, sink, proj))) return rc;
    HIP_TRY(hipSetDevice(e->device));
    if ((rc = reserve(e, B))) return rc;
    if (kind == ENC_PACKED && (rc = ensure_packed(e))) return rc;
    int max_frames = 0;
    block_rows rows;
    if ((rc = prepare_meta(e, kind, in, facts, kl, sink, status, s, max_frames, rows))) return rc;
    const meta_rows dev(e->meta, B);
    if (kind != ENC_PLAIN && out_len)
        for (int i = 0; i < B; ++i) out_len[i] = facts.ok[i] ? kl[i] / 2 : 0;
    // the projector's operand buffers, before the first launch (growing them waits for the stream)
    proj_operand po{nullptr, nullptr, nullptr, 0};
    const q2a_embeds_src * ids = sink.ids;
    if (feats && proj && (rows.N_out > 0 || ids) &&
        (rc = proj_workspace(proj, rows.N_out, s, po, sink.clip_row != nullptr, ids ? ids->n_tokens : 0))) return rc;
    if (ids) {
        // the inputs_embeds form: the row map from input_ids (and the report), then the text rows; they run whether or
        // not the call has a feature row
        int32_t * report = ids->report_dev ? ids->report_dev : po.report;
        PLAUNCH(e, s, Q2A_PROF_POOL, q2a_launch_audio_token_rows(ids_args(ids->input_ids, ids->ids_width, ids->n_tokens, ids->audio_token_id,
                                                                          rows.N_out, po, report), s));
        if (ids->embed_table) PLAUNCH(e, s, Q2A_PROF_POOL, launch_embeds_gather(*ids, *sink.dst, proj->d_out, report, s));
    }
    // (packed with every clip skipped: no rows, nothing to run; the pool kernel below writes the zeros. The
    // audio-feature tail writes valid rows only: without any, nothing is launched behind the metadata)
    if (feats ? rows.N_out > 0 : kind != ENC_PACKED || rows.M > 0) {
        if ((rc = run_frontend(e, in, max_frames, s))) return rc;
        if (kind == ENC_PACKED)
            PLAUNCH(e, s, Q2A_PROF_POOL, launch_gather_rows(e->X, e->Xp, dev.row_start, B, d.T, d.D, rows.r_max, s));
        for (int l = 0; l < d.L; ++l)
            if ((rc = run_block(e, l, rows, s))) return rc;
    }
    const float * lnw = e->g<const float *>(G_LNP_W), * lnb = e->g<const float *>(G_LNP_B);
    if (feats) {
        // the valid rows alone, packed: f32 into embd and / or the projector GEMM's A operand straight from the pool
        // kernel's registers, then that GEMM with its bias epilogue into feat
        if (rows.N_out == 0) return Q2A_OK;
        q2a_pool_pack_args pa{e->Xp, B, d.D, rows.N_out, lnw, lnb, dev.row_start, dev.out_start, sink.embd,
                              proj ? proj_mode(proj) : -1, po.A, po.dy, po.aext, po.ld};
        PLAUNCH(e, s, Q2A_PROF_POOL, q2a_launch_pool_pack(pa, s));
        if (sink.to_dst()) {
            // the _to form: the device row map from the uploaded out_start and clip_row (none when packed), then the
            // same GEMM with the row-map epilogue straight into the caller's rows
            if (po.map && !ids) PLAUNCH(e, s, Q2A_PROF_POOL, launch_feat_row_map(dev.out_start, dev.clip_row, po.map, B, d.TO, s));
            LAUNCH(q2a_launch_gemm(proj_gemm_to(proj, rows.N_out, po, *sink.dst, po.map), Q2A_EPI_STORE_ROWS, proj->gblk, s));
        } else if (proj) {
            LAUNCH(q2a_launch_gemm(proj_gemm(proj, rows.N_out, po, sink.feat), Q2A_EPI_STORE_F, proj->gblk, s));
        }
    } else if (kind == ENC_PACKED) {
        q2a_pool_varlen_args pa{e->Xp, B, d.T, d.D, lnw, lnb, sink.out, dev.key_len, dev.row_start};
        PLAUNCH(e, s, Q2A_PROF_POOL, q2a_launch_pool_ln_varlen(pa, s));
    } else {
        q2a_pool_args pa{e->X, B, d.T, d.D, lnw, lnb, sink.out, dev.clip_ok};
        PLAUNCH(e, s, Q2A_PROF_POOL, q2a_launch_pool_ln(pa, s));
        if (kind == ENC_PADDED) PLAUNCH(e, s, Q2A_PROF_POOL, launch_zero_tail_rows(sink.out, dev.key_len, dev.clip_ok, B, d.TO, d.D, s));
    }
    return Q2A_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

const char * q2a_last_error(void) { return g_err.c_str(); }

// (q2a_internal.h) the calling thread's q2a_last_error text, for the library's other translation units
void q2a_internal_set_error(const char * msg) { g_err = msg ? msg : ""; }

int q2a_internal_engine_blob(const q2a_engine * e, const void ** blob, int64_t * bytes, int * device) {
    if (!e || !e->blob || e->h.compact) { set_err("engine holds no device-layout weights"); return Q2A_ERR_ARG; }
    if (blob) *blob = e->blob;
    if (bytes) *bytes = e->blob_size;
    if (device) *device = e->device;
    return Q2A_OK;
}

static int64_t pack_model(const char * path, int act, bool compact, void ** host_blob) {
    if (act != Q2A_ACT_REFERENCE && act != Q2A_ACT_BF16) { set_err("unknown activation mode %d", act); return Q2A_ERR_ARG; }
    std::vector<uint8_t> v;
    const int rc = pack(path, v, act, compact);
    if (rc) return rc;
    void * p = malloc(v.size());
    if (!p) { set_err("host allocation failed"); return Q2A_ERR_OOM; }
    memcpy(p, v.data(), v.size());
    *host_blob = p;
    return (int64_t) v.size();
}

int64_t q2a_pack_model(const char * path, void ** host_blob) { return pack_model(path, Q2A_ACT_REFERENCE, false, host_blob); }
int64_t q2a_pack_model_ex(const char * path, int act, void ** host_blob) { return pack_model(path, act, false, host_blob); }
int64_t q2a_pack_model_compact(const char * path, int act, void ** host_blob) { return pack_model(path, act, true, host_blob); }

int64_t q2a_blob_device_size(const void * host_header, int64_t header_bytes, int64_t * transport_bytes) {
    blob_header h;
    if (!host_header || header_bytes < (int64_t) sizeof(h)) { set_err("invalid arguments"); return Q2A_ERR_ARG; }
    memcpy(&h, host_header, sizeof(h));
    if (const char * why = header_problem(h)) { set_err("%s", why); return Q2A_ERR_FORMAT; }
    if (transport_bytes) *transport_bytes = h.compact ? (int64_t) compact_of(h).total : (int64_t) h.total;
    return (int64_t) h.total;
}

int q2a_expand_blob(const void * dev_blob, int64_t size, void * dev_out, int64_t out_bytes, int device, void * stream) {
    if (!dev_blob || !dev_out || size < (int64_t) HEADER_BYTES) { set_err("invalid arguments"); return Q2A_ERR_ARG; }
    int prev = -1;
    HIP_TRY(hipGetDevice(&prev));
    struct restore { int d; ~restore() { if (d >= 0) (void) hipSetDevice(d); } } rs{prev};   // the caller's device back
    HIP_TRY(hipSetDevice(device));
    blob_header h;
    HIP_TRY(hipMemcpy(&h, dev_blob, sizeof(h), hipMemcpyDeviceToHost));
    if (const char * why = header_problem(h)) { set_err("%s", why); return Q2A_ERR_FORMAT; }
    if (!h.compact) { set_err("not a compact q2a weight blob"); return Q2A_ERR_FORMAT; }
    if ((int64_t) compact_of(h).total != size || out_bytes < (int64_t) h.total) { set_err("blob size mismatch"); return Q2A_ERR_ARG; }
    return expand_blob((const uint8_t *) dev_blob, h, (uint8_t *) dev_out, stream ? (hipStream_t) stream : nullptr);
}

void q2a_free_host_blob(void * p) { free(p); }

q2a_engine * q2a_open(const char * model_path, int device) { return q2a_open_ex(model_path, device, Q2A_ACT_REFERENCE); }

q2a_engine * q2a_open_ex(const char * model_path, int device, int act) {
    if (act != Q2A_ACT_REFERENCE && act != Q2A_ACT_BF16) { set_err("unknown activation mode %d", act); return nullptr; }
    q2a_engine * e = new q2a_engine();
    std::vector<uint8_t> v;
    if (engine_init(e, device) || pack(model_path, v, act)) { q2a_close(e); return nullptr; }
    memcpy(&e->h, v.data(), sizeof(blob_header));
    if (engine_adopt_header(e)) { q2a_close(e); return nullptr; }
    if (hipMalloc((void **) &e->blob, v.size()) != hipSuccess) {
        (void) hipGetLastError();
        set_err("weight allocation of %.2f GB failed", v.size() / 1e9);
        q2a_close(e);
        return nullptr;
    }
    e->own_blob = true;
    e->blob_size = (int64_t) v.size();
    if (hipMemcpy(e->blob, v.data(), v.size(), hipMemcpyHostToDevice) != hipSuccess) {
        set_err("weight upload failed");
        q2a_close(e);
        return nullptr;
    }
    return e;
}

q2a_engine * q2a_open_device_blob(const void * dev_blob, int64_t size, int device) {
    if (!dev_blob || size < (int64_t) HEADER_BYTES) { set_err("invalid blob"); return nullptr; }
    q2a_engine * e = new q2a_engine();
    if (engine_init(e, device)) { q2a_close(e); return nullptr; }
    if (hipMemcpy(&e->h, dev_blob, sizeof(blob_header), hipMemcpyDeviceToHost) != hipSuccess) {
        set_err("cannot read blob header from device");
        q2a_close(e);
        return nullptr;
    }
    if (engine_adopt_header(e)) { q2a_close(e); return nullptr; }   // (validates before any size is derived)
    const int64_t want = e->h.compact ? (int64_t) compact_of(e->h).total : (int64_t) e->h.total;
    if (want != size) {
        set_err("blob size mismatch");
        q2a_close(e);
        return nullptr;
    }
    if (e->h.compact) {   // the transport form: expand into an engine-owned device layout
        const blob_header hc = e->h;
        e->h.compact = 0;
        if (hipMalloc((void **) &e->blob, e->h.total) != hipSuccess) {
            (void) hipGetLastError();
            set_err("weight allocation of %.2f GB failed", e->h.total / 1e9);
            q2a_close(e);
            return nullptr;
        }
        e->own_blob = true;
        e->blob_size = (int64_t) e->h.total;
        if (expand_blob((const uint8_t *) dev_blob, hc, e->blob, e->stream)) { q2a_close(e); return nullptr; }
        return e;
    }
    e->blob = (uint8_t *) dev_blob;
    e->own_blob = false;
    e->blob_size = size;
    return e;
}

q2a_engine * q2a_open_shared(const q2a_engine * base) {
    if (!base) { set_err("invalid arguments"); return nullptr; }
    return q2a_open_device_blob(base->blob, base->blob_size, base->device);
}

int q2a_set_force_encode(q2a_engine * e, int on) {
    if (!e) return Q2A_ERR_ARG;
    e->force_encode = on != 0;
    return Q2A_OK;
}

void q2a_close(q2a_engine * e) {
    if (!e) return;
    (void) hipSetDevice(e->device);
    (void) hipDeviceSynchronize();   // (calls may have run on caller streams or stream 0, not only e->stream)
    free_host_bufs(e);
    free_ws(e);
    for (auto & r : e->pending) { (void) hipEventDestroy(r.a); (void) hipEventDestroy(r.b); }
    for (auto ev : e->pool) (void) hipEventDestroy(ev);
    if (e->own_blob && e->blob) (void) hipFree(e->blob);
    if (e->frange) (void) hipFree(e->frange);
    if (e->meta_evt) (void) hipEventDestroy(e->meta_evt);
    if (e->stream) (void) hipStreamDestroy(e->stream);
    delete e;
}

int q2a_get_info(const q2a_engine * e, q2a_info * info) {
    if (!e || !info) return Q2A_ERR_ARG;
    info->n_audio_ctx = e->d.T; info->n_audio_state = e->d.D; info->n_audio_head = e->d.H;
    info->n_audio_layer = e->d.L; info->n_mels = e->d.M; info->wtype = e->wtype; info->n_out = e->d.TO;
    info->device = e->device; info->weight_bytes = e->blob_size; info->workspace_bytes = (int64_t) e->ws_bytes + (int64_t) e->xp_clips * e->d.T * e->d.D * 4;
    info->act = e->bf16 ? Q2A_ACT_BF16 : Q2A_ACT_REFERENCE;
    info->reserved = 0;
    return Q2A_OK;
}

int q2a_reserve(q2a_engine * e, int max_clips, int64_t max_samples) {
    if (!e || max_clips <= 0) { set_err("invalid arguments"); return Q2A_ERR_ARG; }
    (void) max_samples;
    return reserve(e, max_clips);
}

// the prologue of every encode and feature entry point: arguments, activation contract, and for the key-length kinds
// the key lengths into kl (the caller's, checked, or the input's own valid lengths)
static int call_prologue(q2a_engine * e, encode_kind kind, const clip_input & in, const int32_t * key_len, std::vector<int32_t> & kl) {
    if (!e || !in.len || in.B <= 0) { set_err("invalid arguments"); return Q2A_ERR_ARG; }
    if (int rc = lens_supported(e, kind)) return rc;
    return kind == ENC_PLAIN ? Q2A_OK : key_lens(e, in, key_len, kl);
}

// the `kind` argument of the log-mel entry points (Q2A_ENCODE_*) as the engine's; false: there is no such kind
static bool kind_of(int kind, encode_kind & ek) {
    ek = kind == Q2A_ENCODE_PLAIN ? ENC_PLAIN : kind == Q2A_ENCODE_PADDED ? ENC_PADDED : ENC_PACKED;
    if (kind >= Q2A_ENCODE_PLAIN && kind <= Q2A_ENCODE_VARLEN) return true;
    set_err("invalid arguments");
    return false;
}

// Every device entry point: the prologue, what the sink requires, then the encode on the caller's stream
static int encode_device(q2a_engine * e, encode_kind kind, q2a_projector * p, const clip_input & in, const int32_t * key_len,
                         const out_sink & sink, int32_t * out_len, int32_t * status, void * stream) {
    std::vector<int32_t> kl;
    if (int rc = call_prologue(e, kind, in, key_len, kl)) return rc;
    if (!in.data) { set_err("invalid arguments"); return Q2A_ERR_ARG; }
    // (without dst a _to call would be the f32 one's "embd alone")
    if (sink.to_dst() && !(p && sink.dst)) { set_err("audio features: the _to calls need a projector and a destination"); return Q2A_ERR_ARG; }
    if (sink.kind == out_sink::IDS && !sink.ids) { set_err("inputs_embeds: src is required"); return Q2A_ERR_ARG; }
    return encode(e, kind, in, kind == ENC_PLAIN ? nullptr : kl.data(), sink, p, out_len, status, call_stream(stream));
}

int q2a_encode_device(q2a_engine * e, const float * pcm_dev, int64_t pcm_stride, const int32_t * n_samples,
                      int n_clips, int offset_ms, float * out_dev, int32_t * status, void * stream) {
    return encode_device(e, ENC_PLAIN, nullptr, pcm_input(pcm_dev, pcm_stride, n_samples, n_clips, nullptr, offset_ms), nullptr,
                         window_sink(out_dev), nullptr, status, stream);
}

int q2a_encode_device_ex(q2a_engine * e, const float * pcm_dev, int64_t pcm_stride, const int32_t * n_samples,
                         const int32_t * offsets_ms, int n_clips, float * out_dev, int32_t * status, void * stream) {
    if (!offsets_ms) { set_err("invalid arguments"); return Q2A_ERR_ARG; }
    return encode_device(e, ENC_PLAIN, nullptr, pcm_input(pcm_dev, pcm_stride, n_samples, n_clips, offsets_ms), nullptr,
                         window_sink(out_dev), nullptr, status, stream);
}

int q2a_encode_device_padded(q2a_engine * e, const float * pcm_dev, int64_t pcm_stride, const int32_t * n_samples,
                             const int32_t * offsets_ms, const int32_t * key_len, int n_clips, float * out_dev,
                             int32_t * out_len, int32_t * status, void * stream) {
    return encode_device(e, ENC_PADDED, nullptr, pcm_input(pcm_dev, pcm_stride, n_samples, n_clips, offsets_ms), key_len,
                         window_sink(out_dev), out_len, status, stream);
}

int q2a_encode_device_varlen(q2a_engine * e, const float * pcm_dev, int64_t pcm_stride, const int32_t * n_samples,
                             const int32_t * offsets_ms, const int32_t * key_len, int n_clips, float * out_dev,
                             int32_t * out_len, int32_t * status, void * stream) {
    return encode_device(e, ENC_PACKED, nullptr, pcm_input(pcm_dev, pcm_stride, n_samples, n_clips, offsets_ms), key_len,
                         window_sink(out_dev), out_len, status, stream);
}

int q2a_encode_device_mel(q2a_engine * e, int kind, const float * mel_dev, int64_t clip_stride, int64_t ld,
                          const int32_t * n_len, const int32_t * seek, const int32_t * key_len, int n_clips,
                          float * out_dev, int32_t * out_len, int32_t * status, void * stream) {
    encode_kind ek;
    if (!kind_of(kind, ek)) return Q2A_ERR_ARG;
    return encode_device(e, ek, nullptr, mel_input(mel_dev, clip_stride, ld, n_len, seek, n_clips), key_len, window_sink(out_dev),
                         out_len, status, stream);
}

// ---- audio features: the variable-length encode with its valid output rows packed and projected; the _to form with
// dst and clip_row in place of feat, the inputs_embeds form with src in place of clip_row ---------------------------
int q2a_audio_features_device(q2a_engine * e, q2a_projector * p, const float * pcm_dev, int64_t pcm_stride,
                              const int32_t * n_samples, const int32_t * offsets_ms, const int32_t * key_len, int n_clips,
                              float * feat_dev, float * embd_dev, int64_t rows_cap, int32_t * out_len, int32_t * status,
                              void * stream) {
    return encode_device(e, ENC_PACKED, p, pcm_input(pcm_dev, pcm_stride, n_samples, n_clips, offsets_ms), key_len,
                         packed_sink(feat_dev, embd_dev, rows_cap), out_len, status, stream);
}

int q2a_audio_features_device_mel(q2a_engine * e, q2a_projector * p, const float * mel_dev, int64_t clip_stride, int64_t ld,
                                  const int32_t * n_len, const int32_t * seek, const int32_t * key_len, int n_clips,
                                  float * feat_dev, float * embd_dev, int64_t rows_cap, int32_t * out_len, int32_t * status,
                                  void * stream) {
    return encode_device(e, ENC_PACKED, p, mel_input(mel_dev, clip_stride, ld, n_len, seek, n_clips), key_len,
                         packed_sink(feat_dev, embd_dev, rows_cap), out_len, status, stream);
}

int q2a_audio_features_device_to(q2a_engine * e, q2a_projector * p, const float * pcm_dev, int64_t pcm_stride,
                                 const int32_t * n_samples, const int32_t * offsets_ms, const int32_t * key_len, int n_clips,
                                 const q2a_feat_dst * dst, const int32_t * clip_row, float * embd_dev, int64_t embd_rows_cap,
                                 int32_t * out_len, int32_t * status, void * stream) {
    return encode_device(e, ENC_PACKED, p, pcm_input(pcm_dev, pcm_stride, n_samples, n_clips, offsets_ms), key_len,
                         rows_sink(dst, clip_row, embd_dev, embd_rows_cap), out_len, status, stream);
}

int q2a_audio_features_device_mel_to(q2a_engine * e, q2a_projector * p, const float * mel_dev, int64_t clip_stride, int64_t ld,
                                     const int32_t * n_len, const int32_t * seek, const int32_t * key_len, int n_clips,
                                     const q2a_feat_dst * dst, const int32_t * clip_row, float * embd_dev,
                                     int64_t embd_rows_cap, int32_t * out_len, int32_t * status, void * stream) {
    return encode_device(e, ENC_PACKED, p, mel_input(mel_dev, clip_stride, ld, n_len, seek, n_clips), key_len,
                         rows_sink(dst, clip_row, embd_dev, embd_rows_cap), out_len, status, stream);
}

int q2a_inputs_embeds_device(q2a_engine * e, q2a_projector * p, const float * pcm_dev, int64_t pcm_stride,
                             const int32_t * n_samples, const int32_t * offsets_ms, const int32_t * key_len, int n_clips,
                             const q2a_feat_dst * dst, const q2a_embeds_src * src, float * embd_dev, int64_t embd_rows_cap,
                             int32_t * out_len, int32_t * status, void * stream) {
    return encode_device(e, ENC_PACKED, p, pcm_input(pcm_dev, pcm_stride, n_samples, n_clips, offsets_ms), key_len,
                         ids_sink(dst, src, embd_dev, embd_rows_cap), out_len, status, stream);
}

int q2a_inputs_embeds_device_mel(q2a_engine * e, q2a_projector * p, const float * mel_dev, int64_t clip_stride, int64_t ld,
                                 const int32_t * n_len, const int32_t * seek, const int32_t * key_len, int n_clips,
                                 const q2a_feat_dst * dst, const q2a_embeds_src * src, float * embd_dev,
                                 int64_t embd_rows_cap, int32_t * out_len, int32_t * status, void * stream) {
    return encode_device(e, ENC_PACKED, p, mel_input(mel_dev, clip_stride, ld, n_len, seek, n_clips), key_len,
                         ids_sink(dst, src, embd_dev, embd_rows_cap), out_len, status, stream);
}

// ---- the host entry points -------------------------------------------------------------------------------------
// Their clips: `in` describes them as for a device call (data NULL), ptr[c] is clip c's PCM, or its log-mel
// [n_mels][len[c]] host floats
namespace {
struct host_clips {
    clip_input in;
    const float * const * ptr;
};
// the staged log-mel windows of a chunk as its encode sees them (stage_chunk)
struct chunk_windows {
    std::vector<int32_t> len, seek;
};
}

// checked before any copy (a negative count would be a huge memcpy); a bad clip fails every clip of the call
static int host_clips_check(const host_clips & h, int32_t * status) {
    const clip_input & in = h.in;
    for (int c = 0; c < in.B; ++c) {
        const int n = in.len[c], sk = in.mel && in.seek ? in.seek[c] : 0;
        if (in.mel ? n >= 1 && h.ptr[c] && sk >= 0 : n >= 0 && (n == 0 || h.ptr[c])) continue;
        set_err("clip %d: bad %s (%d, seek %d, %p)", c, in.mel ? "mel" : "samples", n, sk, (const void *) h.ptr[c]);
        if (status) for (int k = 0; k < in.B; ++k) status[k] = Q2A_CLIP_FAILED;
        return Q2A_ERR_ARG;
    }
    return Q2A_OK;
}

// floats per staged clip of the chunk [c0, c0 + n): the longest PCM clip (whole 64s), or one log-mel window
static int64_t stage_stride(const q2a_engine * e, const host_clips & h, int c0, int n) {
    if (h.in.mel) return (int64_t) e->d.M * e->d.TM;
    int64_t maxn = 1;
    for (int c = 0; c < n; ++c) maxn = std::max<int64_t>(maxn, h.in.len[c0 + c]);
    return (maxn + 63) & ~int64_t(63);
}

// one clip's window columns of every mel row -> dst [M][TM], and the window as the encode then sees it: win_len frames
// read from frame win_seek (preset by the caller to 1 and 0)
static void stage_mel_window(float * dst, const float * mel, int64_t n_len, int64_t seek, int M, int TM, int32_t & win_len,
                             int32_t & win_seek) {
    const int w = (int) std::max<int64_t>(0, std::min<int64_t>(n_len - seek, TM));
    // a window behind the last frame has no columns: one (unread) frame at seek 1 makes it all zeros
    if (w > 0) win_len = w; else win_seek = 1;
    for (int j = 0; j < M && w > 0; ++j) memcpy(dst + (int64_t) j * TM, mel + j * n_len + seek, (size_t) w * 4);
}

// The chunk [c0, c0 + n) staged into dst [n][maxn] (host), and the input its encode takes once dst has been copied to
// d_in. PCM: the clips' samples. Log-mel: only the window columns seek .. min(seek + 2 n_ctx, n_len) - 1 of each row, as
// clip c of an array [n][n_mels][2 n_ctx] that the encode reads from frame 0; `win` holds those windows' lengths and
// seeks for as long as the input is used.
static clip_input stage_chunk(const q2a_engine * e, const host_clips & h, int c0, int n, int64_t maxn, float * dst, const float * d_in,
                              chunk_windows & win) {
    const clip_input & in = h.in;
    if (!in.mel) {
        for (int c = 0; c < n; ++c)
            if (in.len[c0 + c] > 0) memcpy(dst + c * maxn, h.ptr[c0 + c], (size_t) in.len[c0 + c] * 4);
        return pcm_input(d_in, maxn, in.len + c0, n, in.offs ? in.offs + c0 : nullptr, in.offset_ms);
    }
    win.len.assign(n, 1);
    win.seek.assign(n, 0);
    for (int c = 0; c < n; ++c)
        stage_mel_window(dst + c * maxn, h.ptr[c0 + c], in.len[c0 + c], in.seek ? in.seek[c0 + c] : 0, e->d.M, e->d.TM, win.len[c], win.seek[c]);
    return mel_input(d_in, maxn, e->d.TM, win.len.data(), win.seek.data(), n);
}

// q2a_encode_host* of any kind (ENC_PACKED: each chunk of clips packed on its own). For the key-length kinds every
// clip's output is copied back (rows past its valid length, and a skipped clip's rows, are zeros).
static int encode_host(q2a_engine * e, encode_kind kind, const host_clips & h, const int32_t * key_len, float * out_host,
                       int32_t * out_len, int32_t * status) {
    std::vector<int32_t> klv;
    if (int rc = call_prologue(e, kind, h.in, key_len, klv)) return rc;
    const int32_t * kl = kind == ENC_PLAIN ? nullptr : klv.data();
    const int n_clips = h.in.B;
    if (!h.ptr || !out_host) { set_err("invalid arguments"); return Q2A_ERR_ARG; }
    if (int rc = host_clips_check(h, status)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    // Chunks of clips through two staging sets: chunk k's host->pinned copy and H2D (copy stream) run while chunk k-1
    // encodes (compute stream), and chunk k-1's D2H + pinned->host copy while chunk k encodes. One chunk below 32
    // clips (nothing to overlap with); else at least two, at most 64 clips each. Clips are independent and every
    // tile regime sums in one K order, so the chunking changes no output bit (batch invariance).
    // Outputs of skipped clips (< 1 s after the offset) are never copied back: the caller's contents stay untouched.
    const int nchunk = n_clips < 32 ? 1 : std::max(2, (n_clips + 63) / 64);
    const int C = (n_clips + nchunk - 1) / nchunk;
    const int64_t maxn = stage_stride(e, h, 0, n_clips);
    chunk_windows win;
    if (int rc = ensure_host_bufs(e, C, maxn)) return rc;
    const size_t per_out = (size_t) e->d.TO * e->d.D;
    // st: what encode reported per clip; pub: what the caller gets — a clip's status is published only once its
    // chunk's outputs reached out_host, so a failure part-way leaves every later clip (and a chunk whose copy-out
    // never ran) at Q2A_CLIP_FAILED rather than a stale "encoded"
    std::vector<int32_t> st(n_clips, Q2A_CLIP_FAILED), pub(n_clips, Q2A_CLIP_FAILED);
    hipStream_t cs = e->copy_stream, s = e->stream;
    int rc = Q2A_OK;
    auto copy_out = [&](int k) {   // chunk k's encoded outputs: pinned -> caller (after its D2H)
        const int c0 = k * C, n = std::min(C, n_clips - c0);
        q2a_engine::host_buf & b = e->hb[k & 1];
        if (hipEventSynchronize(b.d2h) != hipSuccess) return Q2A_ERR_HIP;
        for (int c = 0; c < n; ++c) {
            if (st[c0 + c] == Q2A_CLIP_ENCODED || (kind != ENC_PLAIN && st[c0 + c] == Q2A_CLIP_SKIPPED))
                memcpy(out_host + (c0 + c) * per_out, b.pin_out + c * per_out, per_out * 4);
            pub[c0 + c] = st[c0 + c];
        }
        return Q2A_OK;
    };
    for (int k = 0; k < nchunk && rc == Q2A_OK; ++k) {
        const int c0 = k * C, n = std::min(C, n_clips - c0);
        q2a_engine::host_buf & b = e->hb[k & 1];
        // staging set k&1 was last used by chunk k-2: its H2D must have left pin_in, its D2H must have left d_out
        if (hipEventSynchronize(b.h2d) != hipSuccess) { rc = Q2A_ERR_HIP; break; }
        const clip_input in = stage_chunk(e, h, c0, n, maxn, b.pin_in, b.d_in, win);
        if (hipStreamWaitEvent(cs, b.comp, 0) != hipSuccess ||   // chunk k-2's encode no longer reads d_in
            hipMemcpyAsync(b.d_in, b.pin_in, (size_t) n * maxn * 4, hipMemcpyHostToDevice, cs) != hipSuccess ||
            hipEventRecord(b.h2d, cs) != hipSuccess ||
            hipStreamWaitEvent(s, b.h2d, 0) != hipSuccess ||     // PCM landed
            hipStreamWaitEvent(s, b.d2h, 0) != hipSuccess) {     // chunk k-2's outputs left d_out
            rc = Q2A_ERR_HIP;
            break;
        }
        rc = encode(e, kind, in, kl ? kl + c0 : nullptr, window_sink(b.d_out), nullptr, out_len ? out_len + c0 : nullptr, st.data() + c0, s);
        if (rc) break;
        if (hipEventRecord(b.comp, s) != hipSuccess || hipStreamWaitEvent(cs, b.comp, 0) != hipSuccess ||
            hipMemcpyAsync(b.pin_out, b.d_out, (size_t) n * per_out * 4, hipMemcpyDeviceToHost, cs) != hipSuccess ||
            hipEventRecord(b.d2h, cs) != hipSuccess) {
            rc = Q2A_ERR_HIP;
            break;
        }
        if (k >= 1) rc = copy_out(k - 1);   // runs while chunk k encodes
    }
    if (rc == Q2A_OK) rc = copy_out(nchunk - 1);
    if (hipStreamSynchronize(cs) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        if (rc == Q2A_OK) { set_err("stream error"); rc = Q2A_ERR_HIP; }
    }
    if (rc == Q2A_ERR_HIP && g_err.empty()) set_err("host-path copy failed");
    if (status) for (int c = 0; c < n_clips; ++c) status[c] = pub[c];
    return rc;
}

int q2a_encode_host(q2a_engine * e, const float * const * pcm, const int32_t * n_samples, int n_clips, int offset_ms,
                    float * out_host, int32_t * status) {
    return q2a_encode_host_ex(e, pcm, n_samples, nullptr, n_clips, offset_ms, out_host, status);
}

int q2a_encode_host_ex(q2a_engine * e, const float * const * pcm, const int32_t * n_samples, const int32_t * offsets_ms,
                       int n_clips, int offset_ms, float * out_host, int32_t * status) {
    return encode_host(e, ENC_PLAIN, {pcm_input(nullptr, 0, n_samples, n_clips, offsets_ms, offset_ms), pcm}, nullptr, out_host, nullptr, status);
}

int q2a_encode_host_padded(q2a_engine * e, const float * const * pcm, const int32_t * n_samples, const int32_t * offsets_ms,
                           const int32_t * key_len, int n_clips, float * out_host, int32_t * out_len, int32_t * status) {
    return encode_host(e, ENC_PADDED, {pcm_input(nullptr, 0, n_samples, n_clips, offsets_ms), pcm}, key_len, out_host, out_len, status);
}

int q2a_encode_host_varlen(q2a_engine * e, const float * const * pcm, const int32_t * n_samples, const int32_t * offsets_ms,
                           const int32_t * key_len, int n_clips, float * out_host, int32_t * out_len, int32_t * status) {
    return encode_host(e, ENC_PACKED, {pcm_input(nullptr, 0, n_samples, n_clips, offsets_ms), pcm}, key_len, out_host, out_len, status);
}

int q2a_encode_host_mel(q2a_engine * e, int kind, const float * const * mel, const int32_t * n_len, const int32_t * seek,
                        const int32_t * key_len, int n_clips, float * out_host, int32_t * out_len, int32_t * status) {
    encode_kind ek;
    if (!kind_of(kind, ek)) return Q2A_ERR_ARG;
    return encode_host(e, ek, {mel_input(nullptr, 0, 0, n_len, seek, n_clips), mel}, key_len, out_host, out_len, status);
}

// The audio features of host clips: chunks of up to 64 clips, each staged into device buffers of its own, run through
// the device path on the engine's stream and waited for; a chunk's rows follow the previous chunk's in the caller's
// arrays. A clip's status is published once its chunk's rows reached the caller (Q2A_CLIP_FAILED before).
static int features_host(q2a_engine * e, q2a_projector * p, const host_clips & h, const int32_t * key_len, float * feat, float * embd,
                         int64_t rows_cap, int32_t * out_len, int32_t * status) {
    std::vector<int32_t> klv;
    if (int rc = call_prologue(e, ENC_PACKED, h.in, key_len, klv)) return rc;
    const int32_t * kl = klv.data();
    const int n_clips = h.in.B;
    if (!h.ptr) { set_err("invalid arguments"); return Q2A_ERR_ARG; }
    if (int rc = host_clips_check(h, status)) return rc;
    // the whole batch against rows_cap, before anything is written
    if (int rc = features_check(e, resolve_clips(e, h.in), kl, packed_sink(feat, embd, rows_cap), p)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    const int D = e->d.D, d_out = p ? p->d_out : 0;
    const int C = std::min(n_clips, 64);
    std::vector<int32_t> st(n_clips, Q2A_CLIP_FAILED), ol(n_clips, 0);
    chunk_windows win;
    std::vector<float> stage;
    float * d_in = nullptr, * d_feat = nullptr, * d_embd = nullptr;
    auto release = [&]() {
        for (float ** b : {&d_in, &d_feat, &d_embd}) { if (*b) (void) hipFree(*b); *b = nullptr; }
    };
    hipStream_t s = e->stream;
    int64_t row0 = 0;
    int rc = Q2A_OK;
    for (int c0 = 0; c0 < n_clips && rc == Q2A_OK; c0 += C) {
        const int n = std::min(C, n_clips - c0);
        const int64_t maxn = stage_stride(e, h, c0, n);
        int64_t cap = 1;
        for (int c = 0; c < n; ++c) cap += kl[c0 + c] / 2;
        stage.assign((size_t) n * maxn, 0.f);
        if (hipMalloc((void **) &d_in, stage.size() * 4) != hipSuccess || (p && hipMalloc((void **) &d_feat, (size_t) cap * d_out * 4) != hipSuccess) ||
            (embd && hipMalloc((void **) &d_embd, (size_t) cap * D * 4) != hipSuccess)) {
            (void) hipGetLastError();
            set_err("audio features: staging allocation failed");
            rc = Q2A_ERR_OOM;
            break;
        }
        const clip_input in = stage_chunk(e, h, c0, n, maxn, stage.data(), d_in, win);
        if (hipMemcpyAsync(d_in, stage.data(), stage.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess) { rc = Q2A_ERR_HIP; break; }
        if ((rc = encode(e, ENC_PACKED, in, kl + c0, packed_sink(d_feat, d_embd, cap), p, ol.data() + c0, st.data() + c0, s))) break;
        int64_t rows = 0;
        for (int c = 0; c < n; ++c) rows += ol[c0 + c];
        if ((p && rows && hipMemcpyAsync(feat + row0 * d_out, d_feat, (size_t) rows * d_out * 4, hipMemcpyDeviceToHost, s) != hipSuccess) ||
            (embd && rows && hipMemcpyAsync(embd + row0 * D, d_embd, (size_t) rows * D * 4, hipMemcpyDeviceToHost, s) != hipSuccess) ||
            hipStreamSynchronize(s) != hipSuccess) {
            rc = Q2A_ERR_HIP;
            break;
        }
        release();
        row0 += rows;
        for (int c = 0; c < n; ++c) {
            if (status) status[c0 + c] = st[c0 + c];
            if (out_len) out_len[c0 + c] = ol[c0 + c];
            st[c0 + c] = -1;   // published
        }
    }
    if (rc != Q2A_OK) {
        (void) hipStreamSynchronize(s);
        (void) hipGetLastError();
        if (rc == Q2A_ERR_HIP && g_err.empty()) set_err("audio features: host-path copy failed");
        for (int c = 0; c < n_clips; ++c)
            if (st[c] != -1) { if (status) status[c] = Q2A_CLIP_FAILED; if (out_len) out_len[c] = 0; }
    }
    release();
    return rc;
}

int q2a_audio_features_host(q2a_engine * e, q2a_projector * p, const float * const * pcm, const int32_t * n_samples,
                            const int32_t * offsets_ms, const int32_t * key_len, int n_clips, float * feat_host, float * embd_host,
                            int64_t rows_cap, int32_t * out_len, int32_t * status) {
    return features_host(e, p, {pcm_input(nullptr, 0, n_samples, n_clips, offsets_ms), pcm}, key_len, feat_host, embd_host, rows_cap, out_len, status);
}

int q2a_audio_features_host_mel(q2a_engine * e, q2a_projector * p, const float * const * mel, const int32_t * n_len,
                                const int32_t * seek, const int32_t * key_len, int n_clips, float * feat_host, float * embd_host,
                                int64_t rows_cap, int32_t * out_len, int32_t * status) {
    return features_host(e, p, {mel_input(nullptr, 0, 0, n_len, seek, n_clips), mel}, key_len, feat_host, embd_host, rows_cap, out_len, status);
}

int q2a_pcm_to_mel(q2a_engine * e, const float * pcm, int n_samples, float * mel_out, int64_t mel_cap, int * n_len_out) {
    if (!e || !pcm || !mel_out || !n_len_out || n_samples <= 200) { set_err("invalid arguments"); return Q2A_ERR_ARG; }
    HIP_TRY(hipSetDevice(e->device));
    const dims & d = e->d;
    const int n_len = (int) (((int64_t) n_samples + 480000) / 160);
    if (mel_cap < (int64_t) d.M * n_len) { set_err("mel buffer too small (%d frames)", n_len); return Q2A_ERR_ARG; }
    int rc = reserve(e, 1);
    if (rc) return rc;
    hipStream_t s = e->stream;
    if ((rc = ensure_frange(e, s))) return rc;
    // run the mel kernel with a window covering every frame, in chunks of TM frames
    float * dpcm = nullptr;
    HIP_TRY(hipMalloc((void **) &dpcm, (size_t) n_samples * 4));
    std::vector<float> chunk((size_t) d.M * d.TM);
    const meta_rows dev(e->meta, 1);   // one clip; seek = the chunk's first frame
    const q2a_mel_args ma = mel_args(e, dpcm, n_samples, dev, 1, n_len);
    if (hipMemcpy(dpcm, pcm, (size_t) n_samples * 4, hipMemcpyHostToDevice) != hipSuccess) rc = Q2A_ERR_HIP;
    int32_t cmax = 0;
    for (int f0 = 0; f0 < n_len && rc == Q2A_OK; f0 += d.TM) {
        rc = upload_meta(e, 1, &meta_rows::nsamp, &meta_rows::clip_max, s, [&](const meta_rows & mh) -> int {
            mh.nsamp[0] = n_samples; mh.seek[0] = f0; mh.clip_ok[0] = 1;
            return Q2A_OK;
        });
        if (rc) break;
        if (hipMemsetAsync(dev.clip_max, 0x80, 4, s) != hipSuccess) { rc = Q2A_ERR_HIP; break; }
        if (q2a_launch_mel(ma, s) != hipSuccess) { rc = Q2A_ERR_HIP; break; }
        if (hipMemcpyAsync(chunk.data(), e->mel, chunk.size() * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipMemcpyAsync(&cmax, dev.clip_max, 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess) { rc = Q2A_ERR_HIP; break; }
        const int nf = std::min(d.TM, n_len - f0);
        for (int j = 0; j < d.M; ++j) memcpy(mel_out + (size_t) j * n_len + f0, chunk.data() + (size_t) j * d.TM, (size_t) nf * 4);
    }
    (void) hipFree(dpcm);
    if (rc) { set_err("mel computation failed"); return rc; }
    // clamp + normalise exactly as the reference (:2633-2649) on the host (the device path fuses this into conv1)
    const float mx_f = [&] { int32_t i = cmax; i = i >= 0 ? i : i ^ 0x7fffffff; float f; memcpy(&f, &i, 4); return f; }();
    const double mmax = (double) mx_f - 8.0;
    for (int64_t i = 0; i < (int64_t) d.M * n_len; ++i) {
        float v = mel_out[i];
        if (v < mmax) v = (float) mmax;
        mel_out[i] = (float) ((v + 4.0) / 4.0);
    }
    *n_len_out = n_len;
    return Q2A_OK;
}

int q2a_profile_enable(q2a_engine * e, int on) {
    if (!e) return Q2A_ERR_ARG;
    e->prof = on != 0;
    e->prof_mask = ~0u;
    return Q2A_OK;
}

int q2a_profile_enable_mask(q2a_engine * e, unsigned mask) {
    if (!e) return Q2A_ERR_ARG;
    e->prof = mask != 0;
    e->prof_mask = mask;
    return Q2A_OK;
}

int q2a_profile_read(q2a_engine * e, double * ms, int64_t * counts, int n, int reset) {
    if (!e || n < 0) return Q2A_ERR_ARG;
    HIP_TRY(hipSetDevice(e->device));
    for (auto & r : e->pending) {
        HIP_TRY(hipEventSynchronize(r.b));
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, r.a, r.b));
        e->prof_ms[r.cls] += t;
        e->prof_n[r.cls] += 1;
        e->pool.push_back(r.a);
        e->pool.push_back(r.b);
    }
    e->pending.clear();
    for (int i = 0; i < n && i < Q2A_PROF_CLASSES; ++i) {
        if (ms) ms[i] = e->prof_ms[i];
        if (counts) counts[i] = e->prof_n[i];
    }
    if (reset)
        for (int i = 0; i < Q2A_PROF_CLASSES; ++i) { e->prof_ms[i] = 0; e->prof_n[i] = 0; }
    return Q2A_OK;
}

// x [M][K] f32 (device) -> the A operand of weight `which` in the workspace, by the engine's own mode (ggml's activation
// conversion); dy_ld: the row stride of the block scales the GEMM will read
static int stage_operand(q2a_engine * e, int which, const float * x, int M, int dy_ld, hipStream_t s, q2a_half ** A_out) {
    const dims & d = e->d;
    int N, K;
    mat_dims(d, which, N, K);
    q2a_half * A = K == d.D ? e->actD : e->actF;
    const int mode = ln_mode(e);
    if (mode == 0 || mode == 4) {
        const int64_t n = (int64_t) M * K;
        if (mode == 0) hipLaunchKernelGGL(k_to_half, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, s, x, A, n);
        else hipLaunchKernelGGL(k_to_bf16, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, s, x, A, n);
        LAUNCH(hipGetLastError());
    } else if (mode == 3) {
        const int64_t n = (int64_t) M * K;
        hipLaunchKernelGGL(k_split3, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, s, x, A, K, n);
        LAUNCH(hipGetLastError());
    } else {
        q2a_quant_args qa{x, nullptr, M, K, mode, A, K == d.D ? e->dyD : e->dyF, K == d.D ? e->aextD : e->aextF, dy_ld};
        LAUNCH(q2a_launch_quant_act(qa, s));
    }
    *A_out = A;
    return Q2A_OK;
}

int q2a_test_linear(q2a_engine * e, int layer, int which, const float * x, int M, float * y, void * stream) {
    if (!e || layer < 0 || layer >= e->d.L || which < 0 || which > 3 || M <= 0) return Q2A_ERR_ARG;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = call_stream(stream);
    const dims & d = e->d;
    int rc = reserve(e, (M + d.T - 1) / d.T);
    if (rc) return rc;
    int N, K;
    mat_dims(d, which, N, K);
    q2a_half * A = nullptr;
    if ((rc = stage_operand(e, which, x, M, e->dy_ld, s, &A))) return rc;
    q2a_gemm_args a = gemm_base(e, layer, which, A, M);
    a.outF = y; a.ldo = N;
    LAUNCH(q2a_launch_gemm(a, Q2A_EPI_STORE_F, e->gblk, s));
    return Q2A_OK;
}

static_assert(Q2A_TEST_EPI_QKV == Q2A_EPI_QKV && Q2A_TEST_EPI_RESID == Q2A_EPI_RESID && Q2A_TEST_EPI_GELU_H == Q2A_EPI_GELU_H &&
              Q2A_TEST_EPI_GELU_Q8K == Q2A_EPI_GELU_Q8K && Q2A_TEST_EPI_PRE_H == Q2A_EPI_PRE_H, "public epilogue numbers");

// The block's GEMM `which` with epilogue `epi` at M rows, from run_block's own argument helpers, or false when the
// block never launches that pair on this engine (fc1: under no fc1 path). blk: the launcher mode the block passes.
static bool block_gemm(const q2a_engine * e, int layer, int which, int epi, int M, q2a_gemm_args & a, int & blk) {
    blk = e->gblk;
    if (which == 0 && epi == Q2A_EPI_QKV) { a = qkv_gemm(e, layer, M); return true; }
    if ((which == 1 || which == 3) && epi == Q2A_EPI_RESID) { a = resid_gemm(e, layer, which, M, nullptr); return true; }
    if (which != 2) return false;
    for (int path = 0; path < 3; ++path)
        if (fc1_epi(e, M, path) == epi) {
            a = fc1_gemm(e, layer, M, epi);
            if (epi == Q2A_EPI_GELU_Q8K) blk = e->blk;
            return true;
        }
    return false;
}

int q2a_test_gemm_regime(q2a_engine * e, int which, int epi, int M) {
    if (!e || which < 0 || which > 3 || M <= 0) return Q2A_ERR_ARG;
    HIP_TRY(hipSetDevice(e->device));
    if (int rc = reserve(e, 1)) return rc;   // (the launcher checks the workspace's scale pointers; no-op once reserved)
    q2a_gemm_args a;
    int blk = 0;
    if (!block_gemm(e, 0, which, epi, M, a, blk)) return Q2A_ERR_ARG;
    if (epi == Q2A_EPI_RESID) a.outF = (float *) e->blob;   // (any non-null pointer: the plan reads no output pointer)
    const q2a_gemm_plan pl = q2a_gemm_plan_for(a, epi, blk);
    return pl.regime == Q2A_REGIME_NONE ? Q2A_ERR_ARG : pl.regime;
}

int q2a_test_gemm_epi(q2a_engine * e, int layer, int which, int epi, const float * x, int M, void * const * out, int ld,
                      void * stream) {
    if (!e || layer < 0 || layer >= e->d.L || which < 0 || which > 3 || M <= 0 || !x || !out || !out[0]) return Q2A_ERR_ARG;
    const bool q8k = epi == Q2A_EPI_GELU_Q8K;
    if (q8k && (ld < M || ld % 256 || !out[1] || !out[2])) return Q2A_ERR_ARG;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = call_stream(stream);
    const dims & d = e->d;
    // (the fused Q8_K epilogue writes its scales with the stride it reads the operand's with: ld on both sides)
    int rc = reserve(e, (std::max(M, q8k ? ld : 0) + d.T - 1) / d.T);
    if (rc) return rc;
    q2a_gemm_args a;
    int blk = 0;
    if (!block_gemm(e, layer, which, epi, M, a, blk)) return Q2A_ERR_ARG;
    const int dy_ld = q8k ? ld : e->dy_ld;
    q2a_half * A = nullptr;
    if ((rc = stage_operand(e, which, x, M, dy_ld, s, &A))) return rc;
    a.dy_ld = dy_ld;
    if (epi == Q2A_EPI_QKV) {
        const int n = e->bf16 ? 3 : 6;
        for (int i = 0; i < n; ++i) if (!out[i]) return Q2A_ERR_ARG;
        if (e->bf16) {
            a.qh = (q2a_half *) out[0]; a.kh = (q2a_half *) out[1]; a.vt = (q2a_half *) out[2];
        } else {
            a.qh = (q2a_half *) out[0]; a.ql = (q2a_half *) out[1]; a.kh = (q2a_half *) out[2]; a.kl = (q2a_half *) out[3];
            a.vt = (q2a_half *) out[4]; a.vtl = a.vtl ? (q2a_half *) out[5] : nullptr;
        }
    } else if (epi == Q2A_EPI_RESID) {
        a.outF = (float *) out[0];
    } else {
        a.outH = (q2a_half *) out[0];
        if (q8k) { a.qdy = (float *) out[1]; a.qaext = (q2a_half *) out[2]; }
    }
    LAUNCH(q2a_launch_gemm(a, epi, blk, s));
    return Q2A_OK;
}

// one block in place on x: the windows [n_clips*T][D], or for ENC_PACKED the packed rows [M_tot][D] (q2a_varlen_rows
// over key_len), the variable-length encode's block
static int test_block(q2a_engine * e, encode_kind kind, int layer, float * x, int n_clips, const int32_t * key_len, void * stream) {
    if (!e || layer < 0 || layer >= e->d.L || n_clips <= 0 || (kind != ENC_PLAIN && !key_len) || (kind == ENC_PACKED && !x))
        return Q2A_ERR_ARG;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = call_stream(stream);
    int rc = reserve(e, n_clips);
    if (rc) return rc;
    block_rows rows;
    if ((rc = hook_rows(e, kind, key_len, n_clips, s, rows))) return rc;
    if (kind == ENC_PACKED) {
        if ((rc = ensure_packed(e))) return rc;
        rows.X = e->Xp;
    }
    const size_t bytes = (size_t) rows.M * e->d.D * 4;
    HIP_TRY(hipMemcpyAsync(rows.X, x, bytes, hipMemcpyDeviceToDevice, s));
    if ((rc = run_block(e, layer, rows, s))) return rc;
    HIP_TRY(hipMemcpyAsync(x, rows.X, bytes, hipMemcpyDeviceToDevice, s));
    return Q2A_OK;
}

int q2a_test_block(q2a_engine * e, int layer, float * x, int n_clips, void * stream) {
    return test_block(e, ENC_PLAIN, layer, x, n_clips, nullptr, stream);
}

int q2a_test_block_len(q2a_engine * e, int layer, float * x, int n_clips, const int32_t * key_len, void * stream) {
    return test_block(e, ENC_PADDED, layer, x, n_clips, key_len, stream);
}

int q2a_test_block_varlen(q2a_engine * e, int layer, float * x, int n_clips, const int32_t * key_len, void * stream) {
    return test_block(e, ENC_PACKED, layer, x, n_clips, key_len, stream);
}

int q2a_test_block_taps(q2a_engine * e, int layer, float * x, int n_clips, void * const * taps, void * stream) {
    if (!e || !taps) return Q2A_ERR_ARG;
    for (int i = 0; i < 4; ++i) e->taps[i] = taps[i];
    const int rc = test_block(e, ENC_PLAIN, layer, x, n_clips, nullptr, stream);
    for (int i = 0; i < 4; ++i) e->taps[i] = nullptr;
    return rc;
}

// the front end of the clips `in` (plain metadata, no status) -> x_dev [B*T][D]
static int test_frontend(q2a_engine * e, const clip_input & in, float * x_dev, void * stream) {
    if (!e || !in.data || !in.len || !x_dev || in.B <= 0) return Q2A_ERR_ARG;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = call_stream(stream);
    int rc = reserve(e, in.B);
    if (rc) return rc;
    int max_frames = 0;
    block_rows rows;
    rc = prepare_meta(e, ENC_PLAIN, in, resolve_clips(e, in), nullptr, window_sink(x_dev), nullptr, s, max_frames, rows);
    if (rc) return rc;
    rc = run_frontend(e, in, max_frames, s);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(x_dev, e->X, (size_t) in.B * e->d.T * e->d.D * 4, hipMemcpyDeviceToDevice, s));
    return Q2A_OK;
}

int q2a_test_frontend(q2a_engine * e, const float * pcm_dev, int64_t pcm_stride, const int32_t * n_samples, int n_clips,
                      float * x_dev, void * stream) {
    return test_frontend(e, pcm_input(pcm_dev, pcm_stride, n_samples, n_clips, nullptr), x_dev, stream);   // no offsets
}

int q2a_test_frontend_mel(q2a_engine * e, const float * mel_dev, int64_t clip_stride, int64_t ld, const int32_t * n_len,
                          const int32_t * seek, int n_clips, float * x_dev, void * stream) {
    return test_frontend(e, mel_input(mel_dev, clip_stride, ld, n_len, seek, n_clips), x_dev, stream);
}

int q2a_test_pool_ln(q2a_engine * e, const float * x_dev, int n_clips, float * out_dev, void * stream) {
    if (!e || !x_dev || !out_dev || n_clips <= 0) return Q2A_ERR_ARG;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = call_stream(stream);
    int rc = reserve(e, n_clips);
    if (rc) return rc;
    rc = upload_meta(e, n_clips, &meta_rows::clip_ok, &meta_rows::clip_max, s, [&](const meta_rows & mh) -> int {
        std::fill(mh.clip_ok, mh.clip_max, 1);   // every clip "encoded"
        return Q2A_OK;
    });
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(e->X, x_dev, (size_t) n_clips * e->d.T * e->d.D * 4, hipMemcpyDeviceToDevice, s));
    q2a_pool_args pa{e->X, n_clips, e->d.T, e->d.D, e->g<const float *>(G_LNP_W), e->g<const float *>(G_LNP_B), out_dev,
                     meta_rows(e->meta, n_clips).clip_ok};
    LAUNCH(q2a_launch_pool_ln(pa, s));
    return Q2A_OK;
}

// the audio-feature tail's pool kernel alone, straight from the caller's packed rows into the caller's buffers
int q2a_test_pool_operand(q2a_engine * e, int mode, const float * x_dev, int n_clips, const int32_t * key_len, float * embd_dev,
                          void * codes_dev, float * dy_dev, void * aext_dev, int ld, void * stream) {
    if (!e || !x_dev || n_clips <= 0 || !key_len || mode < 0 || mode > 2) return Q2A_ERR_ARG;
    if (!codes_dev) mode = -1;   // no operand: the f32 rows alone
    if (mode < 0 && !embd_dev) return Q2A_ERR_ARG;
    if ((mode == 1 && (!dy_dev || !aext_dev || e->d.D % 256)) || (mode == 2 && (!dy_dev || e->d.D % 32))) return Q2A_ERR_ARG;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = call_stream(stream);
    int rc = reserve(e, n_clips);
    if (rc) return rc;
    block_rows rows;
    if ((rc = hook_rows(e, ENC_PACKED, key_len, n_clips, s, rows, true))) return rc;
    if (rows.N_out == 0) return Q2A_OK;
    if (mode > 0 && ld < rows.N_out) { set_err("ld %d below the %d output rows", ld, rows.N_out); return Q2A_ERR_ARG; }
    const meta_rows dev(e->meta, n_clips);
    q2a_pool_pack_args pa{x_dev, n_clips, e->d.D, rows.N_out, e->g<const float *>(G_LNP_W), e->g<const float *>(G_LNP_B),
                          dev.row_start, dev.out_start, embd_dev, mode, (q2a_half *) codes_dev, dy_dev, (q2a_half *) aext_dev, ld};
    LAUNCH(q2a_launch_pool_pack(pa, s));
    return Q2A_OK;
}

int q2a_test_fc1_path(q2a_engine * e, int path) {
    if (!e || path < 0 || path > 2) return Q2A_ERR_ARG;
    e->fc1_path = path;
    return Q2A_OK;
}

// one conversion kernel on caller rows, launched exactly as run_block / q2a_test_linear launch it; the engine gives
// the device, the stream and the GELU table only (M and K are the caller's, not the model's)
int q2a_test_operand(q2a_engine * e, int producer, int mode, const void * x, int M, int K, const float * g, const float * b,
                     void * out, float * dy, void * aext, int ld, void * stream) {
    if (!e || !x || !out || M <= 0 || K <= 0 || ld < M) return Q2A_ERR_ARG;
    const bool quant = mode == 1 || mode == 2;
    if (quant && (!dy || (mode == 1 && !aext))) return Q2A_ERR_ARG;
    if (mode == 1 && K % 256) return Q2A_ERR_ARG;
    if (mode == 2 && K % 32) return Q2A_ERR_ARG;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = call_stream(stream);
    if (producer == Q2A_OPERAND_LN) {
        if (mode < 0 || mode > 4 || !g || !b || K % 4 || K > 2048) return Q2A_ERR_ARG;
        q2a_ln_args ln{(const float *) x, M, K, g, b, mode, (q2a_half *) out, dy, (q2a_half *) aext, ld};
        LAUNCH(q2a_launch_layernorm(ln, s));
    } else if (producer == Q2A_OPERAND_QUANT_F32 || producer == Q2A_OPERAND_QUANT_H16) {
        if (!quant || K % 256 || K > 8192) return Q2A_ERR_ARG;
        const bool h16 = producer == Q2A_OPERAND_QUANT_H16;
        q2a_quant_args qa{h16 ? nullptr : (const float *) x, h16 ? (const q2a_half *) x : nullptr, M, K, mode,
                          (q2a_half *) out, dy, (q2a_half *) aext, ld};
        LAUNCH(q2a_launch_quant_act(qa, s));
    } else if (producer == Q2A_OPERAND_GELU_Q8K) {
        if (mode != 1 || (int64_t) M * K >= ((int64_t) 1 << 31)) return Q2A_ERR_ARG;
        LAUNCH(q2a_launch_gelu_quant_q8k((const q2a_half *) x, M, K, e->g<const uint16_t *>(G_GELU), (q2a_half *) out, dy,
                                         (q2a_half *) aext, ld, s));
    } else {
        return Q2A_ERR_ARG;
    }
    return Q2A_OK;
}

// attention only: q, k, v, out are the windows [n_clips*T][D], or for ENC_PACKED the packed rows [M_tot][D]
// (q2a_varlen_rows over key_len)
static int test_attention(q2a_engine * e, encode_kind kind, const float * q, const float * k, const float * v, int n_clips,
                          const int32_t * key_len, float * out, void * stream) {
    if (!e || n_clips <= 0 || (kind != ENC_PLAIN && !key_len) || (kind == ENC_PACKED && (!q || !k || !v || !out))) return Q2A_ERR_ARG;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = call_stream(stream);
    int rc = reserve(e, n_clips);
    if (rc) return rc;
    block_rows rows;
    if ((rc = hook_rows(e, kind, key_len, n_clips, s, rows))) return rc;
    const dims & d = e->d;
    const int64_t n = (int64_t) rows.M * d.D;
    const dim3 g((unsigned) ((n + 255) / 256)), b(256);
    hipLaunchKernelGGL(k_split_hilo, g, b, 0, s, q, e->qh, e->ql, n, Q2A_LOG2E);   // the kernel's log2 units
    hipLaunchKernelGGL(k_split_hilo, g, b, 0, s, k, e->kh, e->kl, n, 1.0f);
    hipLaunchKernelGGL(k_split_hilo, g, b, 0, s, v, e->vt, e->vtl, n, 1.0f);   // V hi / lo row-major (the engine's layout)
    LAUNCH(hipGetLastError());
    q2a_attn_args at{e->qh, e->ql, e->kh, e->kl, e->vt, n_clips, d.T, d.D, d.H, e->TP, nullptr, out};
    at.vtl = e->vtl;
    at.v_rows = 1;
    LAUNCH(launch_attention(at, rows, s));
    return Q2A_OK;
}

int q2a_test_attention(q2a_engine * e, const float * q, const float * k, const float * v, int n_clips, float * out,
                       void * stream) {
    return test_attention(e, ENC_PLAIN, q, k, v, n_clips, nullptr, out, stream);
}

int q2a_test_attention_len(q2a_engine * e, const float * q, const float * k, const float * v, int n_clips,
                           const int32_t * key_len, float * out, void * stream) {
    return test_attention(e, ENC_PADDED, q, k, v, n_clips, key_len, out, stream);
}

int q2a_test_attention_varlen(q2a_engine * e, const float * q, const float * k, const float * v, int n_clips,
                              const int32_t * key_len, float * out, void * stream) {
    return test_attention(e, ENC_PACKED, q, k, v, n_clips, key_len, out, stream);
}

// ---- downstream consumer: the Qwen2-Audio multi-modal projector ---------------------------
// audio_features = Linear(d_model -> text hidden, bias)(embd_enc) (transformers modeling_qwen2_audio.py,
// Qwen2AudioMultiModalProjector; the reference path ends at embd_enc, qwen2-whisper.cpp:2185). Weights from a projector
// file in the ggml container (q2a_write_synthetic_projector layout), run with the encoder's numerics contract for a
// ggml MUL_MAT of that weight type: activations converted per vec_dot_type (fp16 RNE for F16, Q8_K for Q4_K, Q8_0 for
// Q8_0 / Q4_0), exact products, fp32 accumulation in the canonical K order, then + bias in f32 — on the same GEMM.
// (struct q2a_projector and the GEMM arguments: with the engine above, the audio-feature tail of encode() runs them too)
q2a_projector * q2a_projector_open(const char * path, int device) {
    char err[256] = {0};
    q2a_model_file * mf = q2a_model_file_read(path, err, sizeof(err));
    if (!mf) { set_err("projector %s: %s", path ? path : "(null)", err); return nullptr; }
    const q2a_tensor_desc * wt = q2a_model_file_find(mf, "multi_modal_projector.linear.weight");
    const q2a_tensor_desc * bt = q2a_model_file_find(mf, "multi_modal_projector.linear.bias");
    auto fail = [&](int code, const char * msg) -> q2a_projector * {
        set_err("projector %s: %s", path, msg);
        q2a_model_file_free(mf);
        (void) code;
        return nullptr;
    };
    if (!wt || !bt || wt->n_dims != 2 || bt->type != Q2A_TYPE_F32 || bt->ne[0] != wt->ne[1]) return fail(Q2A_ERR_FORMAT, "missing or malformed tensors");
    const int K = (int) wt->ne[0], N = (int) wt->ne[1];
    // (F16 weights: whole 64-deep K-steps suffice — an odd count takes the 256x256 tiles without the 8-phase pipeline)
    if (N % 128 != 0 || K % (wt->type == Q2A_TYPE_F16 ? 64 : 256) != 0)
        return fail(Q2A_ERR_UNSUPPORTED, "d_out must be a multiple of 128, d_in of 256 (F16 weights: of 64)");
    std::vector<uint8_t> packed;
    uint64_t off[A_COUNT];
    if (q2a_pack_linear(mf->data + wt->offset, wt->type, N, K, packed, off) != Q2A_OK)
        return fail(Q2A_ERR_UNSUPPORTED, "weight type not supported (F16, Q4_K, Q5_K, Q6_K, Q8_0, Q4_0)");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) { (void) hipGetLastError(); return fail(Q2A_ERR_HIP, "no such HIP device"); }
    q2a_projector * p = new q2a_projector();
    p->device = device; p->d_in = K; p->d_out = N; p->wtype = wt->type; p->blk = blk_of(wt->type); p->gblk = gblk_of(wt->type);
    for (int i = 0; i < A_COUNT; ++i) p->off[i] = off[i];
    std::vector<uint16_t> gtab(65536);
    q2a_make_gelu_table(gtab.data());
    bool ok = hipSetDevice(device) == hipSuccess && hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking) == hipSuccess &&
              hipMalloc(&p->wdev, packed.size()) == hipSuccess && hipMalloc((void **) &p->bias, (size_t) N * 4) == hipSuccess &&
              hipMalloc((void **) &p->gelu, 65536 * 2) == hipSuccess;
    ok = ok && hipMemcpy(p->wdev, packed.data(), packed.size(), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(p->bias, mf->data + bt->offset, (size_t) N * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy((void *) p->gelu, gtab.data(), 65536 * 2, hipMemcpyHostToDevice) == hipSuccess;
    q2a_model_file_free(mf);
    if (!ok) {
        (void) hipGetLastError();
        set_err("projector %s: device allocation / upload failed", path);
        q2a_projector_close(p);
        return nullptr;
    }
    return p;
}

void q2a_projector_close(q2a_projector * p) {
    if (!p) return;
    (void) hipSetDevice(p->device);
    if (p->stream) (void) hipStreamSynchronize(p->stream);
    if (p->wdev) (void) hipFree(p->wdev);
    if (p->bias) (void) hipFree(p->bias);
    if (p->gelu) (void) hipFree((void *) p->gelu);
    if (p->ws) (void) hipFree(p->ws);
    if (p->stream) (void) hipStreamDestroy(p->stream);
    delete p;
}

int q2a_projector_get_dims(const q2a_projector * p, int * d_in, int * d_out, int * wtype) {
    if (!p) return Q2A_ERR_ARG;
    if (d_in) *d_in = p->d_in;
    if (d_out) *d_out = p->d_out;
    if (wtype) *wtype = p->wtype;
    return Q2A_OK;
}

int q2a_projector_apply(q2a_projector * p, const float * x, int64_t rows, float * y, void * stream) {
    if (!p || !x || !y || rows <= 0 || rows > (1 << 30) / 4) return Q2A_ERR_ARG;
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t s = call_stream(stream);
    const int M = (int) rows, K = p->d_in;
    proj_operand o;
    if (int rc = proj_workspace(p, rows, s, o)) return rc;
    if (p->blk == 0) {
        const int64_t n = (int64_t) M * K;
        hipLaunchKernelGGL(k_to_half, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, s, x, o.A, n);
        LAUNCH(hipGetLastError());
    } else {
        q2a_quant_args qa{x, nullptr, M, K, proj_mode(p), o.A, o.dy, o.aext, o.ld};
        LAUNCH(q2a_launch_quant_act(qa, s));
    }
    LAUNCH(q2a_launch_gemm(proj_gemm(p, M, o, y), Q2A_EPI_STORE_F, p->gblk, s));
    return Q2A_OK;
}

int q2a_projector_apply_to(q2a_projector * p, const float * x, int64_t rows, const q2a_feat_dst * dst, const int32_t * row_map,
                           void * stream) {
    if (!p || !x || !dst || rows <= 0 || rows > (1 << 30) / 4) { set_err("invalid arguments"); return Q2A_ERR_ARG; }
    if (int rc = feat_dst_check(p, dst)) return rc;
    if (!row_map && rows > dst->n_rows) { set_err("feature destination: %lld rows into n_rows %lld", (long long) rows, (long long) dst->n_rows); return Q2A_ERR_ARG; }
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t s = call_stream(stream);
    const int M = (int) rows, K = p->d_in;
    proj_operand o;
    if (int rc = proj_workspace(p, rows, s, o)) return rc;
    if (p->blk == 0) {
        const int64_t n = (int64_t) M * K;
        hipLaunchKernelGGL(k_to_half, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, s, x, o.A, n);
        LAUNCH(hipGetLastError());
    } else {
        q2a_quant_args qa{x, nullptr, M, K, proj_mode(p), o.A, o.dy, o.aext, o.ld};
        LAUNCH(q2a_launch_quant_act(qa, s));
    }
    LAUNCH(q2a_launch_gemm(proj_gemm_to(p, M, o, *dst, row_map), Q2A_EPI_STORE_ROWS, p->gblk, s));
    return Q2A_OK;
}

int q2a_projector_apply_ids(q2a_projector * p, const float * x, int64_t rows, const q2a_feat_dst * dst, const q2a_embeds_src * src,
                            void * stream) {
    if (!p || !x || !dst || rows <= 0 || rows > (1 << 30) / 4) { set_err("invalid arguments"); return Q2A_ERR_ARG; }
    if (int rc = feat_dst_check(p, dst)) return rc;
    if (int rc = embeds_src_check(src, *dst, p->d_out)) return rc;
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t s = call_stream(stream);
    const int M = (int) rows, K = p->d_in;
    proj_operand o;
    if (int rc = proj_workspace(p, rows, s, o, true, src->n_tokens)) return rc;
    int32_t * report = src->report_dev ? src->report_dev : o.report;
    LAUNCH(q2a_launch_audio_token_rows(ids_args(src->input_ids, src->ids_width, src->n_tokens, src->audio_token_id, M, o, report), s));
    LAUNCH(launch_embeds_gather(*src, *dst, p->d_out, report, s));
    if (p->blk == 0) {
        const int64_t n = (int64_t) M * K;
        hipLaunchKernelGGL(k_to_half, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, s, x, o.A, n);
        LAUNCH(hipGetLastError());
    } else {
        q2a_quant_args qa{x, nullptr, M, K, proj_mode(p), o.A, o.dy, o.aext, o.ld};
        LAUNCH(q2a_launch_quant_act(qa, s));
    }
    LAUNCH(q2a_launch_gemm(proj_gemm_to(p, M, o, *dst, o.map), Q2A_EPI_STORE_ROWS, p->gblk, s));
    return Q2A_OK;
}

int q2a_test_audio_token_rows(q2a_projector * p, const void * ids_dev, int32_t ids_width, int64_t n_tokens, int64_t audio_token_id,
                              int64_t n_feat, int32_t * row_map_out_dev, int32_t * report_dev, void * stream) {
    if (!p || !ids_dev || (ids_width != 4 && ids_width != 8) || ((uintptr_t) ids_dev & (uintptr_t) (ids_width - 1)) || n_tokens < 1 ||
        n_tokens > Q2A_IDS_MAX_TOKENS || n_feat < 0 || n_feat > (1 << 30) / 4 || (n_feat > 0 && !row_map_out_dev) || !report_dev) {
        set_err("invalid arguments");
        return Q2A_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t s = call_stream(stream);
    proj_operand o;
    if (int rc = proj_workspace(p, n_feat, s, o, true, n_tokens)) return rc;
    LAUNCH(q2a_launch_audio_token_rows(ids_args(ids_dev, ids_width, n_tokens, audio_token_id, (int) n_feat, o, report_dev), s));
    if (n_feat > 0) HIP_TRY(hipMemcpyAsync(row_map_out_dev, o.map, (size_t) n_feat * 4, hipMemcpyDeviceToDevice, s));
    return Q2A_OK;
}

int q2a_test_embed_gather(const q2a_embeds_src * src, const q2a_feat_dst * dst, int32_t d_out, void * stream) {
    if (!src || !dst || d_out < 1 || !src->embed_table || !src->report_dev) { set_err("invalid arguments"); return Q2A_ERR_ARG; }
    const int es0 = dst->dtype == Q2A_DT_F32 ? 4 : 2;
    if (((int64_t) d_out * es0) % 16 != 0) { set_err("embed gather: d_out %d is no whole number of 16-byte pieces", d_out); return Q2A_ERR_ARG; }
    if (int rc = feat_dst_check_cols(d_out, dst)) return rc;
    if (int rc = embeds_src_check(src, *dst, d_out)) return rc;
    hipStream_t s = call_stream(stream);
    HIP_TRY(hipMemsetAsync(src->report_dev, 0, 16, s));
    LAUNCH(launch_embeds_gather(*src, *dst, d_out, src->report_dev, s));
    return Q2A_OK;
}

int q2a_projector_regime(q2a_projector * p, int64_t rows) {
    if (!p || rows <= 0 || rows > (1 << 30) / 4) { set_err("invalid arguments"); return Q2A_ERR_ARG; }
    HIP_TRY(hipSetDevice(p->device));
    // the plan reads shapes, strides and which scale arrays exist, never memory: the operand pointers need no workspace,
    // only to be non-NULL like a call's
    proj_operand o{(q2a_half *) p->wdev, (float *) p->wdev, (q2a_half *) p->wdev, (int) ((rows + 255) / 256 * 256), nullptr};
    const q2a_gemm_args a = proj_gemm(p, (int) rows, o, nullptr);
    const int rf = q2a_gemm_plan_for(a, Q2A_EPI_STORE_F, p->gblk).regime;
    const int rt = q2a_gemm_plan_for(a, Q2A_EPI_STORE_ROWS, p->gblk).regime;
    if (rf != rt) { set_err("projector regime: the f32 call takes %d, the row-map call %d", rf, rt); return Q2A_ERR_HIP; }
    return rf;
}

}  // extern "C"
