// q2a_format.h — host-side model-file format tooling for the Qwen2-Audio encoder path.
//
// The on-disk layout is the reference's unchanged ggml file (models/convert-pt-to-ggml.py:268-337, read by
// whisper_model_load src/qwen2-whisper.cpp:1350-1872):
//   u32 magic 0x67676d6c | i32 hparams[11] | i32 n_mel, n_fft, f32 filters[n_mel*n_fft] |
//   i32 n_vocab, {u32 len, bytes}* | tensors: {i32 n_dims, i32 name_len, i32 ttype, i32 ne[n_dims], name, data}*
// Quantized files carry ftype + GGML_QNT_VERSION(2)*1000 in hparams[10] (qwen2-whisper.cpp:1414-1416).
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#ifdef __cplusplus
extern "C" {
#endif

// ggml_type ids (ggml/include/ggml.h:357-392) used on this path
enum q2a_ggml_type {
    Q2A_TYPE_F32 = 0,
    Q2A_TYPE_F16 = 1,
    Q2A_TYPE_Q4_0 = 2,
    Q2A_TYPE_Q8_0 = 8,
    Q2A_TYPE_Q2_K = 10,
    Q2A_TYPE_Q3_K = 11,
    Q2A_TYPE_Q4_K = 12,
    Q2A_TYPE_Q5_K = 13,
    Q2A_TYPE_Q6_K = 14,
    Q2A_TYPE_Q8_K = 15,
};

// ggml_ftype ids (ggml/include/ggml.h:411-423)
enum q2a_ggml_ftype {
    Q2A_FTYPE_ALL_F32 = 0,
    Q2A_FTYPE_MOSTLY_F16 = 1,
    Q2A_FTYPE_MOSTLY_Q4_0 = 2,
    Q2A_FTYPE_MOSTLY_Q8_0 = 7,
    Q2A_FTYPE_MOSTLY_Q2_K = 10,
    Q2A_FTYPE_MOSTLY_Q3_K = 11,
    Q2A_FTYPE_MOSTLY_Q4_K = 12,
    Q2A_FTYPE_MOSTLY_Q5_K = 13,
    Q2A_FTYPE_MOSTLY_Q6_K = 14,
};

#define Q2A_FILE_MAGIC 0x67676d6cu
#define Q2A_QNT_VERSION_FACTOR 1000
#define Q2A_QK_K 256
#define Q2A_QK8_0 32
#define Q2A_QK4_0 32

// block layouts (ggml/src/ggml-common.h:143-149, 186-191, 253-280, 282-297, 299-326, 329-335)
typedef struct { uint16_t d; uint8_t qs[16]; } q2a_block_q4_0;           // 18 B / 32 weights
typedef struct { uint16_t d; int8_t qs[32]; } q2a_block_q8_0;            // 34 B / 32 weights
typedef struct { uint8_t scales[16]; uint8_t qs[64]; uint16_t d, dmin; } q2a_block_q2_K;                  // 84 B / 256
typedef struct { uint8_t hmask[32]; uint8_t qs[64]; uint8_t scales[12]; uint16_t d; } q2a_block_q3_K;    // 110 B / 256
typedef struct { uint16_t d, dmin; uint8_t scales[12]; uint8_t qs[128]; } q2a_block_q4_K;  // 144 B / 256
typedef struct { uint16_t d, dmin; uint8_t scales[12]; uint8_t qh[32]; uint8_t qs[128]; } q2a_block_q5_K;  // 176 B / 256
typedef struct { uint8_t ql[128]; uint8_t qh[64]; int8_t scales[16]; uint16_t d; } q2a_block_q6_K;         // 210 B / 256
typedef struct { float d; int8_t qs[256]; int16_t bsums[16]; } q2a_block_q8_K;             // 292 B / 256

// Q2_K / Q3_K field access (dequantize_row_q2_K / _q3_K's indexing, ggml-quants.c:1979-2009, 2327-2375), shared by the
// dequantizer, the quantizers and the blob packer. Weight k of a block: 2-bit pair (k % 128) / 32 of qs[32 (k / 128) +
// k % 32]; Q3_K's third bit is bit k / 32 of hmask[k % 32] (code 0..7, value code - 4); its sub-block scale j = k / 16 is
// 6 bits, the low four in a nibble of scales[j % 8], the high two in scales[8 + j % 4] (0..63, value scale - 32).
static inline int q2a_q2k_code(const q2a_block_q2_K * x, int k) { return (x->qs[32 * (k / 128) + k % 32] >> (2 * ((k % 128) / 32))) & 3; }
static inline int q2a_q3k_code(const q2a_block_q3_K * x, int k) {
    return ((x->qs[32 * (k / 128) + k % 32] >> (2 * ((k % 128) / 32))) & 3) | (((x->hmask[k % 32] >> (k / 32)) & 1) << 2);
}
static inline int q2a_q3k_scale(const q2a_block_q3_K * x, int j) {
    return (j < 8 ? x->scales[j] & 0xF : x->scales[j - 8] >> 4) | (((x->scales[8 + j % 4] >> (2 * (j / 4))) & 3) << 4);
}

// whisper_hparams order as stored (qwen2-whisper.cpp:1374-1384)
typedef struct {
    int32_t n_vocab, n_audio_ctx, n_audio_state, n_audio_head, n_audio_layer;
    int32_t n_text_ctx, n_text_state, n_text_head, n_text_layer, n_mels, ftype;
} q2a_hparams;

// ---- numerics helpers shared with the engine host code -------------------------------------------
uint16_t q2a_fp32_to_fp16(float f);   // IEEE binary16, round-to-nearest-even (== F16C _cvtss_sh(x, 0))
float    q2a_fp16_to_fp32(uint16_t h);
size_t   q2a_row_size(int ggml_type, int64_t ncols);   // bytes of one row (ggml_row_size)

// OCP MXFP8 of 32 consecutive finite values: one e8m0 scale code and 32 e4m3fn bytes. amax = max|x|;
// amax == 0: code 127; else code = max(exponent field of amax - 8, 0), i.e. floor(log2 amax) - 8 + 127 clamped at 0 (the
// upper clamp at 254 cannot bind: a finite f32 gives at most 246). Elements: x * 2^(127 - code) (exact), clamped to
// +-448 (the values of (448, 512) saturate there; below 464 they would round to 448 anyway), rounded to nearest even.
// The device kernels (k_rownorm mode 6, k_quant_mx8) run the same operations; this is the packer's form.
static inline uint8_t q2a_e4m3_rne(float v) {   // |v| <= 448, finite
    uint32_t u;
    memcpy(&u, &v, 4);
    const uint8_t sign = (uint8_t) ((u >> 24) & 0x80);
    u &= 0x7FFFFFFFu;
    float a;
    memcpy(&a, &u, 4);
    if (a < 0.015625f) {   // below 2^-6, the smallest normal: subnormal codes in units of 2^-9 (a * 512 is exact)
        const float t = a * 512.0f + 12582912.0f;   // + 1.5 * 2^23: the f32 add rounds to an integer, to nearest even
        uint32_t q;
        memcpy(&q, &t, 4);
        return (uint8_t) (sign | (q & 0xF));        // 0 .. 8 (8 = the smallest normal)
    }
    const uint32_t r = u + 0x7FFFFu + ((u >> 20) & 1u);   // nearest even at 3 mantissa bits
    return (uint8_t) (sign | (((r >> 20) - (120u << 3)) & 0x7F));   // rebias 127 -> 7
}
static inline void q2a_mx8_quantize_block(const float * x, uint8_t * q, uint8_t * scale) {
    float amax = 0.0f;
    for (int i = 0; i < 32; ++i) { const float a = x[i] < 0 ? -x[i] : x[i]; if (a > amax) amax = a; }
    uint32_t u;
    memcpy(&u, &amax, 4);
    const int ef = (int) (u >> 23);
    const int code = amax == 0.0f ? 127 : (ef > 8 ? ef - 8 : 0);
    const uint32_t iu = (uint32_t) (254 - code) << 23;
    float inv;
    memcpy(&inv, &iu, 4);
    *scale = (uint8_t) code;
    for (int i = 0; i < 32; ++i) {
        float v = x[i] * inv;
        v = v > 448.0f ? 448.0f : v < -448.0f ? -448.0f : v;
        q[i] = q2a_e4m3_rne(v);
    }
}

// ---- deterministic synthetic inputs (SURVEY.md §8d "Synthetic inputs") ----------------------------
uint64_t q2a_splitmix64(uint64_t x);
double   q2a_gauss(uint64_t seed, uint32_t stream, uint64_t index);
// clip c: 0.3 sin(2π(220+37c)t) + 0.1 sin(2π(1000+53c)t) + 0.05 N(0,1), 16 kHz
void q2a_synth_clip(float * out, int64_t n_samples, int clip_index);
// Slaney-normalised mel filterbank [n_mel][n_fft/2+1] (librosa.filters.mel(sr, n_fft, n_mel) semantics)
void q2a_mel_filters_slaney(float * out, int n_mel, int n_fft, int sample_rate);

// Write a synthetic model in the reference layout. ftype 0 = all F32, 1 = F16 (the converter's rules,
// convert-pt-to-ggml.py:309-321). Returns 0 on success.
int q2a_write_synthetic_model(const char * path, const q2a_hparams * hp, uint64_t seed, int n_threads);

// Write a synthetic Qwen2-Audio multi-modal projector file (one Linear d_in -> d_out with bias) in the same ggml
// container (see q2a_format.cpp). ftype 0 = F32 weight, 1 = F16. Returns 0 on success.
int q2a_write_synthetic_projector(const char * path, int d_in, int d_out, int ftype, uint64_t seed);

// Re-quantize a F16/F32 model file the way whisper.cpp's quantize flow does (examples/common-ggml.cpp:41-244
// with to_quant {".*"} and skip {"embed_positions.weight","conv1.bias","conv2.bias"}; only 2-D tensors).
// qtype: Q2A_TYPE_Q2_K / Q3_K / Q4_K / Q5_K / Q6_K / Q8_0 / Q4_0. Byte-identical to
// ggml_quantize_chunk. 0 on success.
int q2a_quantize_model(const char * in_path, const char * out_path, int qtype, int n_threads);

// Row quantizers (ggml "_ref" weight quantizers, byte-exact): k must be a multiple of the block size.
void q2a_quantize_row_q2_K(const float * x, void * y, int64_t k);   // quantize_row_q2_K_ref ggml-quants.c:1909
void q2a_quantize_row_q3_K(const float * x, void * y, int64_t k);   // quantize_row_q3_K_ref ggml-quants.c:2251
void q2a_quantize_row_q4_K(const float * x, void * y, int64_t k);   // quantize_row_q4_K_ref ggml-quants.c:2483
void q2a_quantize_row_q5_K(const float * x, void * y, int64_t k);   // quantize_row_q5_K_ref ggml-quants.c:2676
void q2a_quantize_row_q6_K(const float * x, void * y, int64_t k);   // quantize_row_q6_K_ref ggml-quants.c:2907
void q2a_quantize_row_q8_0(const float * x, void * y, int64_t k);   // quantize_row_q8_0_ref ggml-quants.c:848
void q2a_quantize_row_q4_0(const float * x, void * y, int64_t k);   // quantize_row_q4_0_ref ggml-quants.c:761

// Reference numerics tables (built on the host, compiled without FMA contraction, like the reference):
//   GELU fp16 table (ggml.c:3797-3806): tab[h] = fp16(gelu_f32(fp32(h)))
//   mel tables (whisper_global_cache, qwen2-whisper.cpp:2404-2437): hann[400] | cos[400] | sin[400]
void q2a_make_gelu_table(uint16_t * tab65536);
void q2a_make_mel_tables(float * hann_cos_sin1200);

// ---- model-file reader -----------------------------------------------------------------------------
typedef struct {
    char name[96];
    int32_t type;
    int32_t n_dims;
    int64_t ne[4];
    size_t nbytes;
    size_t offset;      // into q2a_model_file.data
} q2a_tensor_desc;

typedef struct {
    q2a_hparams hp;
    int32_t qntvr;          // quantization version (hparams.ftype / 1000)
    int32_t wtype;          // ggml type of the big matrices (from ftype)
    int32_t n_mel_filt, n_fft_filt;
    float * filters;        // [n_mel_filt][n_fft_filt]
    int32_t n_tensors;
    q2a_tensor_desc * tensors;
    uint8_t * data;         // all tensor payloads back to back
    size_t data_size;
} q2a_model_file;

// Parse a model file. Returns NULL on error and writes a message into err (if non-NULL).
q2a_model_file * q2a_model_file_read(const char * path, char * err, size_t err_len);
void q2a_model_file_free(q2a_model_file * mf);
const q2a_tensor_desc * q2a_model_file_find(const q2a_model_file * mf, const char * name);

#ifdef __cplusplus
}
#endif
