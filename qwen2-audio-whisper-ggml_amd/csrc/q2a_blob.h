// q2a_blob.h — the packed weight blob: its self-describing header, the layout plan, the host packer and the device
// expansion of the compact transport form (q2a_blob.hip). Private to the library: what the engine and the projector
// need of it. Nothing here is exported (hidden visibility); q2a_pack_linear / q2a_pack_layout are in q2a_internal.h.
#pragma once

#include "q2a_format.h"
#include "q2a_internal.h"

#include <cstring>
#include <vector>

#pragma GCC visibility push(hidden)
namespace q2a_blob {

// the calling thread's q2a_last_error text, printf-style (one thread-local, defined with the engine)
void set_err(const char * fmt, ...) __attribute__((format(printf, 1, 2)));

#define HIP_TRY(x)                                                                        \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess) {                                                           \
            set_err("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
            return Q2A_ERR_HIP;                                                           \
        }                                                                                 \
    } while (0)

// ------------------------------------------------------------------------------------------------
// packed device blob: 16 KiB self-describing header + 256-B aligned sections
// ------------------------------------------------------------------------------------------------
constexpr uint32_t BLOB_MAGIC = 0x42413251u;   // "Q2AB"
// version 3: the Q4_K gamma array holds -(dmin/dx) (stored negated); a version-2 blob (positive gamma) is refused
constexpr uint32_t BLOB_VERSION = 5;   // 4: conv1 taps against the three-part mel operand; 5: compact transport form
constexpr int MAX_LAYERS = 64;
constexpr size_t HEADER_BYTES = 32768;

enum { G_CONV1_W, G_CONV1_B, G_CONV2_W, G_CONV2_B, G_PE, G_LNP_W, G_LNP_B, G_FILT, G_TAB, G_GELU, G_GELU_C, G_COUNT };
// per-matrix arrays: W (fp16 [N][K]); block-major DX, DMIN, BETA = DX_{b-1}/DX_b, GAMMA = DMIN_b/DX_b (f32 [nblk][N]),
// WEXT (fp16 [nblk][N][16]). Q6_K: W = q - 32, DX = d [K/256][N], and in the WEXT slot its sub-block scales
// SC (f32 [K/16][N], sub-block-major: one K-step's four rows of a tile are contiguous runs)
enum { A_W, A_DX, A_DMIN, A_WEXT, A_BETA, A_GAMMA, A_COUNT };
constexpr int A_SC = A_WEXT;
enum { L_BQKV, L_BO, L_B1, L_B2, L_LN1W, L_LN1B, L_LN2W, L_LN2B, L_MAT0, L_COUNT = L_MAT0 + 4 * A_COUNT };

struct blob_header {
    uint32_t magic, version;
    q2a_hparams hp;
    int32_t wtype, blk, n_bins, act;   // act: Q2A_ACT_REFERENCE (0) or Q2A_ACT_BF16 (1)
    int32_t compact;                   // 1: the transport form (compact_of below); 0: the device layout
    uint64_t total;                    // bytes of the device layout (goff / loff address it)
    uint64_t goff[G_COUNT];
    uint64_t loff[MAX_LAYERS][L_COUNT];
};
static_assert(sizeof(blob_header) <= HEADER_BYTES, "header too large");

struct dims {
    int T, D, H, L, M, F, TM, TO;
};
inline dims dims_of(const q2a_hparams & hp) {
    dims d;
    d.T = hp.n_audio_ctx; d.D = hp.n_audio_state; d.H = hp.n_audio_head; d.L = hp.n_audio_layer; d.M = hp.n_mels;
    d.F = 4 * d.D; d.TM = 2 * d.T; d.TO = d.T / 2;
    return d;
}
inline void mat_dims(const dims & d, int which, int & N, int & K) {
    switch (which) {
        case 0: N = 3 * d.D; K = d.D; break;
        case 1: N = d.D; K = d.D; break;
        case 2: N = d.F; K = d.D; break;
        default: N = d.D; K = d.F; break;
    }
}
// the activation block of a weight type (its vec_dot_type's: Q8_K for the k-quants, Q8_0 for Q8_0 / Q4_0), 0 = fp16
inline int blk_of(int wtype) {
    return (wtype == Q2A_TYPE_Q4_K || wtype == Q2A_TYPE_Q5_K || wtype == Q2A_TYPE_Q6_K) ? 256
           : (wtype == Q2A_TYPE_Q8_0 || wtype == Q2A_TYPE_Q4_0) ? 32 : 0;
}
// the GEMM's block mode: the activation block, but for Q6_K (per-16 integer scales inside the 256-block)
inline int gblk_of(int wtype) { return wtype == Q2A_TYPE_Q6_K ? Q2A_BLK_Q6K : blk_of(wtype); }
// Q4_K's device layout (sc*q weights, min operand, block-ratio arrays): Q4_K and Q5_K
inline bool kq_minmax(int wtype) { return wtype == Q2A_TYPE_Q4_K || wtype == Q2A_TYPE_Q5_K; }

// the device layout of a model: every offset of `h` (false: too many layers)
bool plan(blob_header & h, const q2a_hparams & hp, int wtype, int act);

// The compact TRANSPORT form of a blob (what rank 0 broadcasts): the header (compact = 1, goff / loff
// still describing the device layout), the small sections verbatim as two kinds of runs — the global one
// [HEADER_BYTES, loff[0][L_BQKV]) and, per layer, the biases + LayerNorm run [loff[l][L_BQKV], loff[l][L_MAT0]) — then
// every linear weight as the model file's own ggml rows (QKV: the q | k | v rows), e.g. raw block_q4_K at 144 B per
// 256 weights instead of the 2-byte sc*q expansion plus its block-scale arrays. expand_blob rebuilds the device
// layout from it on the GPU, byte for byte what pack() writes on the host.
struct compact_layout {
    uint64_t g_off, g_len;
    uint64_t l_off[MAX_LAYERS], l_len[MAX_LAYERS];
    uint64_t raw_off[MAX_LAYERS][4], raw_len[MAX_LAYERS][4];
    uint64_t total;
};
compact_layout compact_of(const blob_header & h);

// A header that arrives from outside the packer: nullptr = valid, else the reason
const char * header_problem(const blob_header & h);

// the model file at `path` as a blob in `out`: the device layout, or with `compact` the transport form
int pack(const char * path, std::vector<uint8_t> & out, int act = 0, bool compact = false);

// device layout of `h` (compact = 1) from the compact blob `cb` (both on the current device); `out` holds h.total bytes
int expand_blob(const uint8_t * cb, const blob_header & h, uint8_t * out, hipStream_t s);

}  // namespace q2a_blob
#pragma GCC visibility pop
