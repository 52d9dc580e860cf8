// q2a_blob.hip — the packed weight blob (q2a_blob.h): the layout plan and its checks, the host packer of a model file
// and of one linear weight (q2a_pack_linear, also the ggml backend's), and the device expansion of the compact
// transport form. Nothing here takes an engine.
#include "q2a_blob.h"

#include <algorithm>
#include <cerrno>
#include <string>
#include <thread>

using namespace q2a_blob;

namespace q2a_blob {

bool plan(blob_header & h, const q2a_hparams & hp, int wtype, int act) {
    memset(&h, 0, sizeof(h));
    // bf16-activation mode: every linear weight dequantized to bf16 [N][K] (no block scales, no splits)
    h.magic = BLOB_MAGIC; h.version = BLOB_VERSION; h.hp = hp; h.wtype = wtype; h.blk = act ? 0 : blk_of(wtype); h.n_bins = 201;
    h.act = act;
    const dims d = dims_of(hp);
    if (d.L > MAX_LAYERS) return false;
    // all-F32 files: every fp16 operand is a [hi | .. ] split (SPLIT = 3 parts of K for the linears, conv1 taps of
    // 3 mel parts, conv2 taps of 2 parts), see expand_rows / pack
    const bool f32 = wtype == Q2A_TYPE_F32;
    const uint64_t kx = f32 && !act ? 3 : 1;
    uint64_t off = HEADER_BYTES;
    auto take = [&](uint64_t bytes) { const uint64_t o = off; off += (bytes + 255) & ~uint64_t(255); return o; };
    h.goff[G_CONV1_W] = take((uint64_t) d.D * 3 * 3 * d.M * 2);
    h.goff[G_CONV1_B] = take((uint64_t) d.D * 4);
    h.goff[G_CONV2_W] = take((uint64_t) d.D * 3 * (f32 ? 2 : 1) * d.D * 2);
    h.goff[G_CONV2_B] = take((uint64_t) d.D * 4);
    h.goff[G_PE] = take((uint64_t) d.T * d.D * 4);
    h.goff[G_LNP_W] = take((uint64_t) d.D * 4);
    h.goff[G_LNP_B] = take((uint64_t) d.D * 4);
    h.goff[G_FILT] = take((uint64_t) d.M * 201 * 4);
    h.goff[G_TAB] = take(1200 * 4);
    h.goff[G_GELU] = take(65536 * 2);
    h.goff[G_GELU_C] = take(Q2A_GELU_C_BYTES);
    for (int l = 0; l < d.L; ++l) {
        uint64_t * lo = h.loff[l];
        lo[L_BQKV] = take((uint64_t) 3 * d.D * 4);
        lo[L_BO] = take((uint64_t) d.D * 4);
        lo[L_B1] = take((uint64_t) d.F * 4);
        lo[L_B2] = take((uint64_t) d.D * 4);
        lo[L_LN1W] = take((uint64_t) d.D * 4);
        lo[L_LN1B] = take((uint64_t) d.D * 4);
        lo[L_LN2W] = take((uint64_t) d.D * 4);
        lo[L_LN2B] = take((uint64_t) d.D * 4);
        for (int w = 0; w < 4; ++w) {
            int N, K;
            mat_dims(d, w, N, K);
            uint64_t * a = lo + L_MAT0 + w * A_COUNT;
            a[A_W] = take((uint64_t) N * K * 2 * kx);
            if (h.blk) a[A_DX] = take((uint64_t) N * (K / h.blk) * 4);
            if (h.blk && kq_minmax(wtype)) {
                a[A_DMIN] = take((uint64_t) N * (K / 256) * 4);
                a[A_WEXT] = take((uint64_t) N * (K / 256) * 16 * 2);
                a[A_BETA] = take((uint64_t) N * (K / 256) * 4);
                a[A_GAMMA] = take((uint64_t) N * (K / 256) * 4);
            } else if (h.blk && wtype == Q2A_TYPE_Q6_K) {
                a[A_SC] = take((uint64_t) N * (K / 16) * 4);
            }
        }
    }
    h.total = off;
    return true;
}

compact_layout compact_of(const blob_header & h) {
    compact_layout c;
    memset(&c, 0, sizeof(c));
    const dims d = dims_of(h.hp);
    uint64_t off = HEADER_BYTES;
    auto take = [&](uint64_t bytes) { const uint64_t o = off; off += (bytes + 255) & ~uint64_t(255); return o; };
    c.g_len = h.loff[0][L_BQKV] - HEADER_BYTES;
    c.g_off = take(c.g_len);
    for (int l = 0; l < d.L; ++l) {
        c.l_len[l] = h.loff[l][L_MAT0 + A_W] - h.loff[l][L_BQKV];
        c.l_off[l] = take(c.l_len[l]);
    }
    for (int l = 0; l < d.L; ++l)
        for (int w = 0; w < 4; ++w) {
            int N, K;
            mat_dims(d, w, N, K);
            c.raw_len[l][w] = (uint64_t) N * q2a_row_size(h.wtype, K);
            c.raw_off[l][w] = take(c.raw_len[l][w]);
        }
    c.total = off;
    return c;
}

// A header that arrives from outside the packer (a device blob, an RCCL-broadcast buffer, a caller's host copy) is
// checked before anything is derived from it: compact_of and expand_blob index fixed [MAX_LAYERS] arrays by its layer
// count and address device memory by its offsets. Magic, version, the shape rules pack() enforces, and every offset
// equal to what plan() lays out for those hparams. nullptr = valid, else the reason.
const char * header_problem(const blob_header & h) {
    if (h.magic != BLOB_MAGIC || h.version != BLOB_VERSION) return "not a q2a weight blob";
    const dims d = dims_of(h.hp);
    if (d.L <= 0 || d.L > MAX_LAYERS) return "not a q2a weight blob (layer count out of range)";
    if (d.D <= 0 || d.D % 128 || d.D != d.H * 64 || d.T <= 0 || d.T % 2 || d.M <= 0 || d.M % 4 || d.T > (1 << 20) ||
        d.M > 4096)
        return "not a q2a weight blob (unsupported shapes)";
    if ((h.compact != 0 && h.compact != 1) || (h.act != Q2A_ACT_REFERENCE && h.act != Q2A_ACT_BF16) ||
        q2a_row_size(h.wtype, d.D) == 0 || (blk_of(h.wtype) == 256 && d.D % 256))
        return "not a q2a weight blob (bad type fields)";
    blob_header p;
    if (!plan(p, h.hp, h.wtype, h.act)) return "not a q2a weight blob (layout)";
    if (p.total != h.total || p.blk != h.blk || p.n_bins != h.n_bins || memcmp(p.goff, h.goff, sizeof(p.goff)) ||
        memcmp(p.loff, h.loff, sizeof(p.loff[0]) * d.L))
        return "not a q2a weight blob (inconsistent layout)";
    return nullptr;
}

}  // namespace q2a_blob

namespace {

inline void scale_min_k4(int j, const uint8_t * q, uint8_t * dd, uint8_t * mm) {   // ggml-quants.c:1898
    if (j < 4) { *dd = q[j] & 63; *mm = q[j + 4] & 63; }
    else {
        *dd = (uint8_t) ((q[j + 4] & 0xF) | ((q[j - 4] >> 6) << 4));
        *mm = (uint8_t) ((q[j + 4] >> 4) | ((q[j - 0] >> 6) << 4));
    }
}

// the 5-bit code of weight l of sub-block j (ggml-quants.c:2782-2783: nibble j & 1 of qs[32 (j / 2) + l], bit j of qh[l])
inline int q5k_code(const q2a_block_q5_K * x, int j, int l) {
    const uint8_t q = x->qs[32 * (j / 2) + l];
    return ((j & 1) ? (q >> 4) : (q & 0xF)) + (((x->qh[l] >> j) & 1) << 4);
}
// the 6-bit code (0..63) of weight k of a block (ggml-quants.c:2988-2998: per 128 weights, four runs of 32 over two
// 32-byte rows of nibbles and one of 2-bit pairs)
inline int q6k_code(const q2a_block_q6_K * x, int k) {
    const int h = k / 128, r = (k % 128) / 32, l = k % 32;
    const uint8_t n = x->ql[64 * h + 32 * (r & 1) + l];
    return ((r & 2) ? (n >> 4) : (n & 0xF)) | (((x->qh[32 * h + l] >> (2 * r)) & 3) << 4);
}

// Expand rows [r0, r1) of a ggml weight matrix into the blob arrays (rows offset by dst_row0).
// F16: copied. Q4_K: W' = sc_j * q (exact small integers), DX = d, DMIN = dmin, WEXT = (64 m_j, m_j). Q5_K: the same
// with its 5-bit codes (sc_j * q <= 1953, still an exact fp16 integer). Q6_K: W' = q - 32, DX = d, SC = sc_j.
// Q8_0: W' = q, DX = d. Q4_0: W' = q - 8, DX = d.
// one ggml row -> f32 values, as ggml's dequantize_row_* computes them (ggml-quants.c: q8_0 :1734, q4_0 :1694,
// q4_K :2555-2577 with d1 = d*sc, m1 = dmin*m, y = d1*q - m1)
void dequant_row(const uint8_t * row, int wtype, int K, float * y) {
    if (wtype == Q2A_TYPE_F32) { memcpy(y, row, (size_t) K * 4); return; }
    if (wtype == Q2A_TYPE_F16) { for (int k = 0; k < K; ++k) y[k] = q2a_fp16_to_fp32(((const uint16_t *) row)[k]); return; }
    if (wtype == Q2A_TYPE_Q8_0) {
        for (int b = 0; b < K / 32; ++b) {
            const q2a_block_q8_0 * x = (const q2a_block_q8_0 *) row + b;
            const float d = q2a_fp16_to_fp32(x->d);
            for (int l = 0; l < 32; ++l) y[b * 32 + l] = x->qs[l] * d;
        }
    } else if (wtype == Q2A_TYPE_Q4_0) {
        for (int b = 0; b < K / 32; ++b) {
            const q2a_block_q4_0 * x = (const q2a_block_q4_0 *) row + b;
            const float d = q2a_fp16_to_fp32(x->d);
            for (int l = 0; l < 16; ++l) {
                y[b * 32 + l] = ((x->qs[l] & 0xF) - 8) * d;
                y[b * 32 + 16 + l] = ((x->qs[l] >> 4) - 8) * d;
            }
        }
    } else if (wtype == Q2A_TYPE_Q4_K) {
        for (int b = 0; b < K / 256; ++b) {
            const q2a_block_q4_K * x = (const q2a_block_q4_K *) row + b;
            const float d = q2a_fp16_to_fp32(x->d), dmin = q2a_fp16_to_fp32(x->dmin);
            for (int j = 0; j < 8; ++j) {
                uint8_t sc, m;
                scale_min_k4(j, x->scales, &sc, &m);
                const float d1 = d * sc, m1 = dmin * m;
                const uint8_t * q = x->qs + 32 * (j / 2);
                for (int l = 0; l < 32; ++l) y[b * 256 + 32 * j + l] = d1 * ((j & 1) ? (q[l] >> 4) : (q[l] & 0xF)) - m1;
            }
        }
    } else if (wtype == Q2A_TYPE_Q5_K) {   // dequantize_row_q5_K, ggml-quants.c:2763-2788
        for (int b = 0; b < K / 256; ++b) {
            const q2a_block_q5_K * x = (const q2a_block_q5_K *) row + b;
            const float d = q2a_fp16_to_fp32(x->d), dmin = q2a_fp16_to_fp32(x->dmin);
            for (int j = 0; j < 8; ++j) {
                uint8_t sc, m;
                scale_min_k4(j, x->scales, &sc, &m);
                const float d1 = d * sc, m1 = dmin * m;
                for (int l = 0; l < 32; ++l) y[b * 256 + 32 * j + l] = d1 * q5k_code(x, j, l) - m1;
            }
        }
    } else if (wtype == Q2A_TYPE_Q6_K) {   // dequantize_row_q6_K, ggml-quants.c:2977-3006: (d * sc) * q
        for (int b = 0; b < K / 256; ++b) {
            const q2a_block_q6_K * x = (const q2a_block_q6_K *) row + b;
            const float d = q2a_fp16_to_fp32(x->d);
            for (int k = 0; k < 256; ++k) y[b * 256 + k] = d * x->scales[k / 16] * (int8_t) (q6k_code(x, k) - 32);
        }
    }
}

uint16_t f32_to_bf16(float f) {   // round to nearest even (finite inputs)
    uint32_t u;
    memcpy(&u, &f, 4);
    return (uint16_t) ((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

void expand_rows(const uint8_t * src, int wtype, int K, int Ntot, int r0, int r1, uint8_t * blob, const uint64_t * a, int dst_row0,
                 int act = 0) {
    uint16_t * W = (uint16_t *) (blob + a[A_W]);
    const size_t rs = q2a_row_size(wtype, K);
    std::vector<float> tmp(act ? K : 0);
    for (int r = r0; r < r1; ++r) {
        const uint8_t * row = src + (size_t) r * rs;
        const int n = dst_row0 + r;
        uint16_t * wr = W + (size_t) n * K;
        if (act) {   // bf16-activation mode: dequantized weight, RNE to bf16
            dequant_row(row, wtype, K, tmp.data());
            for (int k = 0; k < K; ++k) wr[k] = f32_to_bf16(tmp[k]);
        } else if (wtype == Q2A_TYPE_F16) {
            memcpy(wr, row, (size_t) K * 2);
        } else if (wtype == Q2A_TYPE_F32) {
            // [Wh | Wh | Wl] against activations [Ah | Al | Ah]: Ah.Wh + Al.Wh + Ah.Wl, F32-class products
            const float * x = (const float *) row;
            uint16_t * w3 = W + (size_t) n * 3 * K;
            for (int k = 0; k < K; ++k) {
                const uint16_t hi = q2a_fp32_to_fp16(x[k]);
                w3[k] = hi;
                w3[K + k] = hi;
                w3[2 * K + k] = q2a_fp32_to_fp16(x[k] - q2a_fp16_to_fp32(hi));
            }
        } else if (wtype == Q2A_TYPE_Q4_K || wtype == Q2A_TYPE_Q5_K) {
            // block-major scale arrays: [nb][Ntot] / [nb][Ntot][16] so a tile's block scales are contiguous
            // (block_q5_K begins like block_q4_K: d, dmin, scales[12]; only the codes are read by type)
            const bool q5 = wtype == Q2A_TYPE_Q5_K;
            const int nb = K / 256;
            float * dx = (float *) (blob + a[A_DX]);
            float * dm = (float *) (blob + a[A_DMIN]);
            float * be = (float *) (blob + a[A_BETA]);
            float * ga = (float *) (blob + a[A_GAMMA]);
            uint16_t * we = (uint16_t *) (blob + a[A_WEXT]);
            float dprev = 1.0f;
            for (int b = 0; b < nb; ++b) {
                const q2a_block_q5_K * x5 = (const q2a_block_q5_K *) row + b;
                const q2a_block_q4_K * x = q5 ? (const q2a_block_q4_K *) x5 : (const q2a_block_q4_K *) row + b;
                // d = 0: the block's d*sc*q terms vanish; store dx = 1 with zero weights instead (same products,
                // and the block-ratio rescaling of the 8-phase kernel never divides by zero)
                const float d = q2a_fp16_to_fp32(x->d);
                const float deff = d != 0.0f ? d : 1.0f;
                dx[(size_t) b * Ntot + n] = deff;
                dm[(size_t) b * Ntot + n] = q2a_fp16_to_fp32(x->dmin);
                be[(size_t) b * Ntot + n] = dprev / deff;
                ga[(size_t) b * Ntot + n] = -(q2a_fp16_to_fp32(x->dmin) / deff);   // negated: the kernels' fma addend
                dprev = deff;
                for (int j = 0; j < 8; ++j) {
                    uint8_t sc, m;
                    scale_min_k4(j, x->scales, &sc, &m);
                    we[((size_t) b * Ntot + n) * 16 + 2 * j + 0] = q2a_fp32_to_fp16(64.0f * m);
                    we[((size_t) b * Ntot + n) * 16 + 2 * j + 1] = q2a_fp32_to_fp16((float) m);
                    const uint8_t * q = x->qs + 32 * (j / 2);
                    for (int l = 0; l < 32; ++l) {
                        const int v = q5 ? q5k_code(x5, j, l) : (j & 1) ? (q[l] >> 4) : (q[l] & 0xF);
                        wr[b * 256 + 32 * j + l] = q2a_fp32_to_fp16(d != 0.0f ? (float) (sc * v) : 0.0f);
                    }
                }
            }
        } else if (wtype == Q2A_TYPE_Q6_K) {
            // (a block the quantizer zeroed, d = 0 with every byte 0, needs no special case: nothing divides by d)
            const int nb = K / 256;
            float * dx = (float *) (blob + a[A_DX]);
            float * sc = (float *) (blob + a[A_SC]);
            for (int b = 0; b < nb; ++b) {
                const q2a_block_q6_K * x = (const q2a_block_q6_K *) row + b;
                dx[(size_t) b * Ntot + n] = q2a_fp16_to_fp32(x->d);
                for (int j = 0; j < 16; ++j) sc[(size_t) (b * 16 + j) * Ntot + n] = (float) x->scales[j];
                for (int k = 0; k < 256; ++k) wr[b * 256 + k] = q2a_fp32_to_fp16((float) (q6k_code(x, k) - 32));
            }
        } else if (wtype == Q2A_TYPE_Q8_0) {
            const int nb = K / 32;
            float * dx = (float *) (blob + a[A_DX]);
            for (int b = 0; b < nb; ++b) {
                const q2a_block_q8_0 * x = (const q2a_block_q8_0 *) row + b;
                dx[(size_t) b * Ntot + n] = q2a_fp16_to_fp32(x->d);
                for (int l = 0; l < 32; ++l) wr[b * 32 + l] = q2a_fp32_to_fp16((float) x->qs[l]);
            }
        } else if (wtype == Q2A_TYPE_Q4_0) {
            const int nb = K / 32;
            float * dx = (float *) (blob + a[A_DX]);
            for (int b = 0; b < nb; ++b) {
                const q2a_block_q4_0 * x = (const q2a_block_q4_0 *) row + b;
                dx[(size_t) b * Ntot + n] = q2a_fp16_to_fp32(x->d);
                for (int l = 0; l < 16; ++l) {
                    wr[b * 32 + l] = q2a_fp32_to_fp16((float) ((x->qs[l] & 0xF) - 8));
                    wr[b * 32 + 16 + l] = q2a_fp32_to_fp16((float) ((x->qs[l] >> 4) - 8));
                }
            }
        }
    }
}

}  // namespace

namespace q2a_blob {

int pack(const char * path, std::vector<uint8_t> & out, int act, bool compact) {
    char err[256];
    q2a_model_file * mf = q2a_model_file_read(path, err, sizeof(err));
    if (!mf) { set_err("%s", err); return errno == ENOENT ? Q2A_ERR_IO : Q2A_ERR_FORMAT; }
    struct guard { q2a_model_file * m; ~guard() { q2a_model_file_free(m); } } gd{mf};
    const q2a_hparams & hp = mf->hp;
    const int wtype = mf->wtype;
    const dims d = dims_of(hp);
    if (d.D % 128 || d.D != d.H * 64 || d.T % 2 || d.M % 4 || (blk_of(wtype) == 256 && d.D % 256)) {
        set_err("unsupported shapes: D=%d H=%d T=%d M=%d", d.D, d.H, d.T, d.M);
        return Q2A_ERR_UNSUPPORTED;
    }
    if (mf->n_mel_filt != d.M || mf->n_fft_filt != 201) { set_err("bad mel filter shape"); return Q2A_ERR_FORMAT; }
    blob_header h;
    if (!plan(h, hp, wtype, act)) { set_err("too many layers"); return Q2A_ERR_UNSUPPORTED; }
    // the compact transport form is written directly (its size, not the device layout's: 0.38 vs 1.40 GB for Q4_K)
    compact_layout c;
    if (compact) { h.compact = 1; c = compact_of(h); }
    out.assign(compact ? c.total : h.total, 0);
    uint8_t * blob = out.data();
    memcpy(blob, &h, sizeof(h));
    // a small section's device-layout offset -> its bytes in `out` (the compact form keeps the global run and each
    // layer's bias / LayerNorm run verbatim, packed one after the other)
    auto at = [&](uint64_t off) -> uint8_t * {
        if (!compact) return blob + off;
        if (off < h.loff[0][L_BQKV]) return blob + c.g_off + (off - HEADER_BYTES);
        int l = d.L - 1;
        while (l > 0 && off < h.loff[l][L_BQKV]) --l;
        return blob + c.l_off[l] + (off - h.loff[l][L_BQKV]);
    };

    auto T = [&](const std::string & name, int type, std::initializer_list<int64_t> ne) -> const uint8_t * {
        const q2a_tensor_desc * t = q2a_model_file_find(mf, name.c_str());
        if (!t) { set_err("tensor '%s' missing from model file", name.c_str()); return nullptr; }
        if (type >= 0 && t->type != type) { set_err("tensor '%s' has type %d, expected %d", name.c_str(), t->type, type); return nullptr; }
        int i = 0;
        for (int64_t v : ne) {
            if (t->ne[i] != v) { set_err("tensor '%s' has wrong shape", name.c_str()); return nullptr; }
            ++i;
        }
        return mf->data + t->offset;
    };
    auto cpy = [&](uint64_t off, const uint8_t * src, size_t n) { memcpy(at(off), src, n); };

    // conv kernels are F16 in every file but the all-F32 one (vtype, qwen2-whisper.cpp:1542-1543)
    const bool f32 = wtype == Q2A_TYPE_F32;
    const int ctype = f32 ? Q2A_TYPE_F32 : Q2A_TYPE_F16;
    const uint8_t * c1 = T("conv1.weight", ctype, {3, d.M, d.D});
    const uint8_t * c1b = T("conv1.bias", Q2A_TYPE_F32, {1, d.D});
    const uint8_t * c2 = T("conv2.weight", ctype, {3, d.D, d.D});
    const uint8_t * c2b = T("conv2.bias", Q2A_TYPE_F32, {1, d.D});
    const uint8_t * pe = T("embed_positions.weight", Q2A_TYPE_F32, {d.D, d.T});
    const uint8_t * lnw = T("layer_norm.weight", Q2A_TYPE_F32, {d.D});
    const uint8_t * lnb = T("layer_norm.bias", Q2A_TYPE_F32, {d.D});
    if (!c1 || !c1b || !c2 || !c2b || !pe || !lnw || !lnb) return Q2A_ERR_FORMAT;
    {
        // hi / lo fp16 halves of a conv kernel element (F16 kernels: the value itself, lo = 0)
        auto hl = [&](const uint8_t * src, size_t i, uint16_t & hi, uint16_t & lo) {
            if (!f32) { hi = ((const uint16_t *) src)[i]; lo = 0; return; }
            const float x = ((const float *) src)[i];
            hi = q2a_fp32_to_fp16(x);
            lo = q2a_fp32_to_fp16(x - q2a_fp16_to_fp32(hi));
        };
        // conv1: [oc][ic][k] -> k-major taps against the mel operand rows: F16 [w | w | w] x [mel_h | mel_m | mel_l]
        // (exact); F32 [wh | wh | wl] x [mel_h | mel_l | mel_h]
        const int P1 = 3;
        uint16_t * w = (uint16_t *) at(h.goff[G_CONV1_W]);
        for (int oc = 0; oc < d.D; ++oc)
            for (int ic = 0; ic < d.M; ++ic)
                for (int k = 0; k < 3; ++k) {
                    uint16_t hi, lo;
                    hl(c1, ((size_t) oc * d.M + ic) * 3 + k, hi, lo);
                    uint16_t * t = w + (size_t) oc * 3 * P1 * d.M + (size_t) k * P1 * d.M + ic;
                    t[0] = hi;
                    t[d.M] = hi;
                    t[2 * d.M] = f32 ? lo : hi;
                }
        // conv2: k-major taps over three consecutive conv1 output rows: F16 [w]; F32 [wh | wl] x rows [y | y]
        const int P2 = f32 ? 2 : 1;
        uint16_t * w2 = (uint16_t *) at(h.goff[G_CONV2_W]);
        for (int oc = 0; oc < d.D; ++oc)
            for (int ic = 0; ic < d.D; ++ic)
                for (int k = 0; k < 3; ++k) {
                    uint16_t hi, lo;
                    hl(c2, ((size_t) oc * d.D + ic) * 3 + k, hi, lo);
                    uint16_t * t = w2 + (size_t) oc * 3 * P2 * d.D + (size_t) k * P2 * d.D + ic;
                    t[0] = hi;
                    if (f32) t[d.D] = lo;
                }
    }
    cpy(h.goff[G_CONV1_B], c1b, (size_t) d.D * 4);
    cpy(h.goff[G_CONV2_B], c2b, (size_t) d.D * 4);
    cpy(h.goff[G_PE], pe, (size_t) d.T * d.D * 4);
    cpy(h.goff[G_LNP_W], lnw, (size_t) d.D * 4);
    cpy(h.goff[G_LNP_B], lnb, (size_t) d.D * 4);
    cpy(h.goff[G_FILT], (const uint8_t *) mf->filters, (size_t) d.M * 201 * 4);
    q2a_make_mel_tables((float *) at(h.goff[G_TAB]));
    q2a_make_gelu_table((uint16_t *) at(h.goff[G_GELU]));
    {   // compact |x| <= 10 image of the table for the LDS-resident epilogue lookups: [+0 .. +10] | [-0 .. -10]
        const uint16_t * t = (const uint16_t *) at(h.goff[G_GELU]);
        uint16_t * cg = (uint16_t *) at(h.goff[G_GELU_C]);
        memset(cg, 0, Q2A_GELU_C_BYTES);
        for (int i = 0; i < Q2A_GELU_C_HALF; ++i) { cg[i] = t[i]; cg[Q2A_GELU_C_HALF + i] = t[0x8000 + i]; }
    }

    struct job { const uint8_t * src; int K, Ntot, r0, r1; const uint64_t * a; int dst0; };
    std::vector<job> jobs;
    for (int l = 0; l < d.L; ++l) {
        const std::string p = "layers." + std::to_string(l) + ".";
        const uint64_t * lo = h.loff[l];
        const uint8_t * wq = T(p + "self_attn.q_proj.weight", wtype, {d.D, d.D});
        const uint8_t * bq = T(p + "self_attn.q_proj.bias", Q2A_TYPE_F32, {d.D});
        const uint8_t * wk = T(p + "self_attn.k_proj.weight", wtype, {d.D, d.D});
        const uint8_t * wv = T(p + "self_attn.v_proj.weight", wtype, {d.D, d.D});
        const uint8_t * bv = T(p + "self_attn.v_proj.bias", Q2A_TYPE_F32, {d.D});
        const uint8_t * wo = T(p + "self_attn.out_proj.weight", wtype, {d.D, d.D});
        const uint8_t * bo = T(p + "self_attn.out_proj.bias", Q2A_TYPE_F32, {d.D});
        const uint8_t * l1w = T(p + "self_attn_layer_norm.weight", Q2A_TYPE_F32, {d.D});
        const uint8_t * l1b = T(p + "self_attn_layer_norm.bias", Q2A_TYPE_F32, {d.D});
        const uint8_t * w1 = T(p + "fc1.weight", wtype, {d.D, d.F});
        const uint8_t * b1 = T(p + "fc1.bias", Q2A_TYPE_F32, {d.F});
        const uint8_t * w2 = T(p + "fc2.weight", wtype, {d.F, d.D});
        const uint8_t * b2 = T(p + "fc2.bias", Q2A_TYPE_F32, {d.D});
        const uint8_t * l2w = T(p + "final_layer_norm.weight", Q2A_TYPE_F32, {d.D});
        const uint8_t * l2b = T(p + "final_layer_norm.bias", Q2A_TYPE_F32, {d.D});
        if (!wq || !bq || !wk || !wv || !bv || !wo || !bo || !l1w || !l1b || !w1 || !b1 || !w2 || !b2 || !l2w || !l2b)
            return Q2A_ERR_FORMAT;
        float * bqkv = (float *) at(lo[L_BQKV]);
        memcpy(bqkv, bq, (size_t) d.D * 4);                 // q bias; k has no bias (qwen2-whisper.cpp:2037)
        memcpy(bqkv + 2 * d.D, bv, (size_t) d.D * 4);
        cpy(lo[L_BO], bo, (size_t) d.D * 4);
        cpy(lo[L_B1], b1, (size_t) d.F * 4);
        cpy(lo[L_B2], b2, (size_t) d.D * 4);
        cpy(lo[L_LN1W], l1w, (size_t) d.D * 4);
        cpy(lo[L_LN1B], l1b, (size_t) d.D * 4);
        cpy(lo[L_LN2W], l2w, (size_t) d.D * 4);
        cpy(lo[L_LN2B], l2b, (size_t) d.D * 4);
        const uint64_t * a0 = lo + L_MAT0;
        jobs.push_back({wq, d.D, 3 * d.D, 0, d.D, a0, 0});
        jobs.push_back({wk, d.D, 3 * d.D, 0, d.D, a0, d.D});
        jobs.push_back({wv, d.D, 3 * d.D, 0, d.D, a0, 2 * d.D});
        jobs.push_back({wo, d.D, d.D, 0, d.D, lo + L_MAT0 + A_COUNT, 0});
        jobs.push_back({w1, d.D, d.F, 0, d.F, lo + L_MAT0 + 2 * A_COUNT, 0});
        jobs.push_back({w2, d.F, d.D, 0, d.D, lo + L_MAT0 + 3 * A_COUNT, 0});
    }
    if (compact) {   // the transport form: small sections written above, linear weights as the file's ggml rows
        for (int l = 0; l < d.L; ++l)
            for (int w = 0; w < 4; ++w) {   // jobs[6l..6l+5] = q, k, v, o, fc1, fc2
                const int j0 = w == 0 ? 0 : w + 2, nj = w == 0 ? 3 : 1;
                uint64_t o = c.raw_off[l][w];
                for (int q = 0; q < nj; ++q) {
                    const job & jb = jobs[6 * l + j0 + q];
                    const size_t n = (size_t) (jb.r1 - jb.r0) * q2a_row_size(wtype, jb.K);
                    memcpy(blob + o, jb.src, n);
                    o += n;
                }
            }
        return Q2A_OK;
    }
    const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t)
        th.emplace_back([&, t]() {
            for (const job & j : jobs) {
                const int n = j.r1 - j.r0;
                expand_rows(j.src, wtype, j.K, j.Ntot, j.r0 + n * t / nt, j.r0 + n * (t + 1) / nt, blob, j.a, j.dst0, act);
            }
        });
    for (auto & x : th) x.join();
    return Q2A_OK;
}

}  // namespace q2a_blob

// One weight matrix on its own (the ggml-backend plugin's MUL_MAT weights): same arrays as a blob matrix,
// laid out in one allocation whose offsets go to off[A_W..A_GAMMA] (0 = absent).
uint64_t q2a_pack_layout(int wtype, int N, int K, uint64_t off[6]) {
    const int blk = blk_of(wtype);
    if ((wtype != Q2A_TYPE_F16 && !blk) || (blk && K % blk) || N <= 0 || K <= 0) return 0;
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) { const uint64_t r = o; o += (bytes + 255) & ~uint64_t(255); return r; };
    for (int i = 0; i < A_COUNT; ++i) off[i] = 0;
    off[A_W] = take((uint64_t) N * K * 2);
    if (blk) off[A_DX] = take((uint64_t) N * (K / blk) * 4);
    if (kq_minmax(wtype)) {
        off[A_DMIN] = take((uint64_t) N * (K / 256) * 4);
        off[A_WEXT] = take((uint64_t) N * (K / 256) * 16 * 2);
        off[A_BETA] = take((uint64_t) N * (K / 256) * 4);
        off[A_GAMMA] = take((uint64_t) N * (K / 256) * 4);
    } else if (wtype == Q2A_TYPE_Q6_K) {
        off[A_SC] = take((uint64_t) N * (K / 16) * 4);
    }
    return o;
}

int q2a_pack_linear(const uint8_t * raw, int wtype, int N, int K, std::vector<uint8_t> & out, uint64_t off[6]) {
    const uint64_t o = q2a_pack_layout(wtype, N, K, off);
    if (!o) return Q2A_ERR_UNSUPPORTED;
    out.assign(o, 0);
    const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t)
        th.emplace_back([&, t]() { expand_rows(raw, wtype, K, N, (int) ((int64_t) N * t / nt), (int) ((int64_t) N * (t + 1) / nt), out.data(), off, 0); });
    for (auto & x : th) x.join();
    return Q2A_OK;
}

namespace {

// ---- compact blob -> device layout (expand_rows on the GPU: every value bit-identical to the host pack) ----
__device__ __forceinline__ float h2f(uint16_t u) { return (float) __builtin_bit_cast(_Float16, u); }
__device__ __forceinline__ uint16_t f2h(float f) { return __builtin_bit_cast(uint16_t, (_Float16) f); }   // RNE
__device__ __forceinline__ uint16_t f2bf(float f) {   // RNE on the bits, as f32_to_bf16 (finite inputs)
    const uint32_t u = __builtin_bit_cast(uint32_t, f);
    return (uint16_t) ((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ void scale_min_k4_d(int j, const uint8_t * q, int & dd, int & mm) {   // ggml-quants.c:1898
    if (j < 4) { dd = q[j] & 63; mm = q[j + 4] & 63; }
    else { dd = (q[j + 4] & 0xF) | ((q[j - 4] >> 6) << 4); mm = (q[j + 4] >> 4) | ((q[j - 0] >> 6) << 4); }
}
__device__ __forceinline__ int q5k_code_d(const q2a_block_q5_K * x, int j, int l) {   // as q5k_code
    const int q = x->qs[32 * (j / 2) + l];
    return ((j & 1) ? (q >> 4) : (q & 0xF)) + (((x->qh[l] >> j) & 1) << 4);
}
__device__ __forceinline__ int q6k_code_d(const q2a_block_q6_K * x, int k) {   // as q6k_code
    const int h = k / 128, r = (k % 128) / 32, l = k % 32;
    const int n = x->ql[64 * h + 32 * (r & 1) + l];
    return ((r & 2) ? (n >> 4) : (n & 0xF)) | (((x->qh[32 * h + l] >> (2 * r)) & 3) << 4);
}

struct expand_args {
    const uint8_t * raw;    // ggml rows [nrows][row_size]
    uint8_t * blob;         // device layout
    uint64_t a[A_COUNT];    // the matrix's array offsets in the device layout
    int wtype, act, K, Ntot, kx;
};

// one workgroup = 256 consecutive weights of one row (blockIdx.x = row, blockIdx.y = 256-chunk of K); the float
// operations are expand_rows' / dequant_row's, uncontracted, so every byte equals the host pack
__global__ __launch_bounds__(256) void k_expand_rows(const expand_args p) {
#pragma clang fp contract(off)
    const int n = blockIdx.x, t = threadIdx.x, k = blockIdx.y * 256 + t;
    const size_t rs = p.wtype == Q2A_TYPE_Q4_K ? (size_t) p.K / 256 * 144 : p.wtype == Q2A_TYPE_Q5_K ? (size_t) p.K / 256 * 176
                    : p.wtype == Q2A_TYPE_Q6_K ? (size_t) p.K / 256 * 210 : p.wtype == Q2A_TYPE_Q8_0 ? (size_t) p.K / 32 * 34
                    : p.wtype == Q2A_TYPE_Q4_0 ? (size_t) p.K / 32 * 18 : p.wtype == Q2A_TYPE_F16 ? (size_t) p.K * 2 : (size_t) p.K * 4;
    const uint8_t * row = p.raw + (size_t) n * rs;
    uint16_t * W = (uint16_t *) (p.blob + p.a[A_W]);
    if (k >= p.K) return;
    float val = 0.0f;   // dequantized value (bf16 mode)
    if (p.wtype == Q2A_TYPE_Q4_K || p.wtype == Q2A_TYPE_Q5_K) {
        const bool q5 = p.wtype == Q2A_TYPE_Q5_K;   // (block_q5_K begins like block_q4_K: d, dmin, scales[12])
        const int b = k / 256, j = (k % 256) / 32, l = k % 32;
        const q2a_block_q5_K * x5 = (const q2a_block_q5_K *) row + b;
        const q2a_block_q4_K * x = q5 ? (const q2a_block_q4_K *) x5 : (const q2a_block_q4_K *) row + b;
        int sc, m;
        scale_min_k4_d(j, x->scales, sc, m);
        const int v = q5 ? q5k_code_d(x5, j, l) : (j & 1) ? (x->qs[32 * (j / 2) + l] >> 4) : (x->qs[32 * (j / 2) + l] & 0xF);
        const float d = h2f(x->d), dmin = h2f(x->dmin);
        if (p.act) {
            const float d1 = d * (float) sc, m1 = dmin * (float) m;
            val = d1 * (float) v - m1;
        } else {
            W[(size_t) n * p.K + k] = d != 0.0f ? f2h((float) (sc * v)) : (uint16_t) 0;
            const size_t bi = (size_t) b * p.Ntot + n;
            const float deff = d != 0.0f ? d : 1.0f;
            if (t == 0) {
                float dprev = 1.0f;
                if (b > 0) {
                    const float dp = q5 ? h2f((x5 - 1)->d) : h2f((x - 1)->d);
                    dprev = dp != 0.0f ? dp : 1.0f;
                }
                ((float *) (p.blob + p.a[A_DX]))[bi] = deff;
                ((float *) (p.blob + p.a[A_DMIN]))[bi] = dmin;
                ((float *) (p.blob + p.a[A_BETA]))[bi] = dprev / deff;
                ((float *) (p.blob + p.a[A_GAMMA]))[bi] = -(dmin / deff);
            }
            if (t < 16) {
                int sj, mj;
                scale_min_k4_d(t / 2, x->scales, sj, mj);
                ((uint16_t *) (p.blob + p.a[A_WEXT]))[bi * 16 + t] = f2h((t & 1) ? (float) mj : 64.0f * (float) mj);
            }
            return;
        }
    } else if (p.wtype == Q2A_TYPE_Q6_K) {
        const int b = k / 256, kk = k % 256;
        const q2a_block_q6_K * x = (const q2a_block_q6_K *) row + b;
        const int q = q6k_code_d(x, kk) - 32;
        const float d = h2f(x->d);
        if (p.act) val = d * (float) x->scales[kk / 16] * (float) q;
        else {
            W[(size_t) n * p.K + k] = f2h((float) q);
            if (t == 0) ((float *) (p.blob + p.a[A_DX]))[(size_t) b * p.Ntot + n] = d;
            if (t < 16) ((float *) (p.blob + p.a[A_SC]))[(size_t) (b * 16 + t) * p.Ntot + n] = (float) x->scales[t];
            return;
        }
    } else if (p.wtype == Q2A_TYPE_Q8_0) {
        const q2a_block_q8_0 * x = (const q2a_block_q8_0 *) row + k / 32;
        const float d = h2f(x->d);
        if (p.act) val = x->qs[k % 32] * d;
        else {
            W[(size_t) n * p.K + k] = f2h((float) x->qs[k % 32]);
            if (k % 32 == 0) ((float *) (p.blob + p.a[A_DX]))[(size_t) (k / 32) * p.Ntot + n] = d;
            return;
        }
    } else if (p.wtype == Q2A_TYPE_Q4_0) {
        const q2a_block_q4_0 * x = (const q2a_block_q4_0 *) row + k / 32;
        const int l = k % 32, q = (l < 16 ? (x->qs[l] & 0xF) : (x->qs[l - 16] >> 4)) - 8;
        const float d = h2f(x->d);
        if (p.act) val = q * d;
        else {
            W[(size_t) n * p.K + k] = f2h((float) q);
            if (l == 0) ((float *) (p.blob + p.a[A_DX]))[(size_t) (k / 32) * p.Ntot + n] = d;
            return;
        }
    } else if (p.wtype == Q2A_TYPE_F16) {
        const uint16_t u = ((const uint16_t *) row)[k];
        if (p.act) val = h2f(u);
        else { W[(size_t) n * p.K + k] = u; return; }
    } else {   // F32
        const float x = ((const float *) row)[k];
        if (p.act) val = x;
        else {   // [Wh | Wh | Wl]
            uint16_t * w3 = W + (size_t) n * 3 * p.K;
            const uint16_t hi = f2h(x);
            w3[k] = hi;
            w3[p.K + k] = hi;
            w3[2 * p.K + k] = f2h(x - h2f(hi));
            return;
        }
    }
    W[(size_t) n * p.K + k] = f2bf(val);
}

}  // namespace

namespace q2a_blob {

// device layout of `h` (compact = 1) from the compact blob `cb` (both on the current device); `out` holds h.total bytes
int expand_blob(const uint8_t * cb, const blob_header & h, uint8_t * out, hipStream_t s) {
    const compact_layout c = compact_of(h);
    const dims d = dims_of(h.hp);
    std::vector<uint8_t> head(HEADER_BYTES, 0);
    // on every return (errors included) the stream drains before `head`, which an async copy may still read, is freed
    struct drain { hipStream_t s; ~drain() { (void) hipStreamSynchronize(s); } } dr{s};
    blob_header hx = h;
    hx.compact = 0;
    memcpy(head.data(), &hx, sizeof(hx));
    HIP_TRY(hipMemsetAsync(out, 0, h.total, s));
    HIP_TRY(hipMemcpyAsync(out, head.data(), HEADER_BYTES, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(out + HEADER_BYTES, cb + c.g_off, c.g_len, hipMemcpyDeviceToDevice, s));
    const int kx = h.wtype == Q2A_TYPE_F32 && !h.act ? 3 : 1;
    for (int l = 0; l < d.L; ++l) {
        HIP_TRY(hipMemcpyAsync(out + h.loff[l][L_BQKV], cb + c.l_off[l], c.l_len[l], hipMemcpyDeviceToDevice, s));
        for (int w = 0; w < 4; ++w) {
            int N, K;
            mat_dims(d, w, N, K);
            expand_args a;
            a.raw = cb + c.raw_off[l][w];
            a.blob = out;
            for (int i = 0; i < A_COUNT; ++i) a.a[i] = h.loff[l][L_MAT0 + w * A_COUNT + i];
            a.wtype = h.wtype; a.act = h.act; a.K = K; a.Ntot = N; a.kx = kx;
            hipLaunchKernelGGL(k_expand_rows, dim3((unsigned) N, (unsigned) ((K + 255) / 256)), dim3(256), 0, s, a);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipStreamSynchronize(s));   // (the header's host staging must outlive its copy)
    return Q2A_OK;
}

}  // namespace q2a_blob
