// inputs_embeds on the device (include/q2a_encoder.h, the q2a_inputs_embeds_* section): the row map of the
// projector GEMM's row-map epilogue derived from input_ids, and the gather of the text rows from the embedding table.
//   k_ids_count / k_ids_place   stable compaction of the positions of audio_token_id: a count per chunk of tokens, then
//                               every workgroup sums the counts in front of its chunk and writes its positions. Two
//                               launches; no workgroup waits for another one's progress.
//   k_embed_gather              row t of the destination := row input_ids[t] of the table, a byte copy in 16-byte
//                               pieces; audio positions are left to the GEMM's epilogue.
//   k_qrow_gather               the same from a table of ggml blocks (Q4_0, Q8_0, Q2_K, Q3_K, Q4_K, Q5_K, Q6_K): the raw row through
//                               LDS, decoded there to ggml's dequantize_row_* values, stored as f32 / fp16 / bf16.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "q2a_format.h"
#include "q2a_internal.h"

namespace {

constexpr int CHUNK = Q2A_IDS_CHUNK;       // tokens per workgroup: 4 waves x WAVE_TOK
constexpr int WAVE_TOK = CHUNK / 4;        // consecutive tokens owned by one wave
constexpr int ITERS = WAVE_TOK / 64;       // 64 consecutive tokens per wave-instruction
static_assert(CHUNK == 4 * 64 * ITERS && CHUNK <= 4096 && (CHUNK & (CHUNK - 1)) == 0, "chunk: a power of two <= 4096");

// the ballots of a wave's WAVE_TOK tokens: bit `lane` of bal[it] = token base + it * 64 + lane is audio_id. The loads
// go out together (the index is clamped, the bound applied to the comparison); ids are compared as 64-bit values, so
// an int64 id whose low word alone equals the audio id does not match. Returns the wave's number of hits.
template <typename IdT>
__device__ __forceinline__ int wave_ballots(const IdT * ids, int n, int64_t audio_id, int base, int lane, uint64_t (&bal)[ITERS]) {
    IdT v[ITERS];
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int t = base + it * 64 + lane;
        v[it] = ids[t < n ? t : n - 1];
    }
    int hits = 0;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int t = base + it * 64 + lane;
        bal[it] = __ballot(t < n && (int64_t) v[it] == audio_id);
        hits += __popcll(bal[it]);
    }
    return hits;
}

// chunk_count[b] = audio tokens among tokens b * CHUNK .. (b + 1) * CHUNK - 1
template <typename IdT>
__global__ __launch_bounds__(256) void k_ids_count(const IdT * ids, int n, int64_t audio_id, int32_t * chunk_count) {
    __shared__ int wave_hits[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t bal[ITERS];
    const int hits = wave_ballots(ids, n, audio_id, blockIdx.x * CHUNK + w * WAVE_TOK, lane, bal);
    if (lane == 0) wave_hits[w] = hits;
    __syncthreads();
    if (threadIdx.x == 0) chunk_count[blockIdx.x] = wave_hits[0] + wave_hits[1] + wave_hits[2] + wave_hits[3];
}

// row_map[k] = the flat position of the k-th audio token for k < min(count, n_feat), -1 for count <= k < n_feat;
// report = {count, n_feat, 0, count != n_feat} (workgroup 0). Nothing at or behind row_map[n_feat] is written.
template <typename IdT>
__global__ __launch_bounds__(256) void k_ids_place(const IdT * ids, int n, int64_t audio_id, const int32_t * chunk_count,
                                                   int n_chunks, int n_feat, int32_t * row_map, int32_t * report) {
    __shared__ int red[2][4];
    __shared__ int wave_hits[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // the audio tokens in front of this chunk, and all of them
    int before = 0, total = 0;
    for (int i = threadIdx.x; i < n_chunks; i += 256) {
        const int c = chunk_count[i];
        total += c;
        before += i < (int) blockIdx.x ? c : 0;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        before += __shfl_xor(before, m);
        total += __shfl_xor(total, m);
    }
    uint64_t bal[ITERS];
    const int base = blockIdx.x * CHUNK + w * WAVE_TOK;
    const int hits = wave_ballots(ids, n, audio_id, base, lane, bal);
    if (lane == 0) { red[0][w] = before; red[1][w] = total; wave_hits[w] = hits; }
    __syncthreads();
    before = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    total = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    int pos = before;
    for (int i = 0; i < w; ++i) pos += wave_hits[i];
    const uint64_t below = (1ull << lane) - 1;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int k = pos + __popcll(bal[it] & below);
        if (((bal[it] >> lane) & 1) && k < n_feat) row_map[k] = base + it * 64 + lane;
        pos += __popcll(bal[it]);
    }
    // the feature rows without an audio token: the epilogue skips a row whose map entry is negative
    for (int64_t k = (int64_t) total + blockIdx.x * 256 + threadIdx.x; k < n_feat; k += (int64_t) gridDim.x * 256) row_map[k] = -1;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        report[0] = total; report[1] = n_feat; report[2] = 0; report[3] = total != n_feat ? 1 : 0;
    }
}

// One wave per token t (wave-uniform id): out row t := table row id, row16 16-byte pieces, four loads in flight per lane
// (clamped index: no load sits under a branch of its own). The audio id: nothing. An id outside [0, vocab): nothing
// stored, report[2] += 1, report[3] |= 2. Strides in 16-byte units.
template <typename IdT>
__global__ __launch_bounds__(256) void k_embed_gather(const IdT * ids, int n, int64_t audio_id, const uint4 * table, int64_t vocab,
                                                      int64_t table_ld16, uint4 * out, int64_t out_ld16, int row16, int32_t * report) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    if (t >= n) return;
    const int64_t id = (int64_t) ids[t];
    if (id == audio_id) return;
    if (id < 0 || id >= vocab) {
        if (lane == 0) { atomicAdd(report + 2, 1); atomicOr(report + 3, 2); }
        return;
    }
    const uint4 * src = table + id * table_ld16;
    uint4 * dst = out + (int64_t) t * out_ld16;
    const int last = row16 - 1;
    for (int i = lane; i < row16; i += 256) {
        // (named values, no array: an indexed one was promoted to 16 KiB of LDS)
        const uint4 v0 = src[i];
        const uint4 v1 = src[i + 64 < last ? i + 64 : last];
        const uint4 v2 = src[i + 128 < last ? i + 128 : last];
        const uint4 v3 = src[i + 192 < last ? i + 192 : last];
        dst[i] = v0;
        if (i + 64 < row16) dst[i + 64] = v1;
        if (i + 128 < row16) dst[i + 128] = v2;
        if (i + 192 < row16) dst[i + 192] = v3;
    }
}

// ---- the decoding gather ---------------------------------------------------------------------------------------------
// One wave per token, as k_embed_gather; a row is decoded in passes of QSEG columns (a pass starts on a 16-byte piece
// of the row for every format: 8 Q6_K blocks are 105 pieces). A pass:
//   1. the raw blocks of the pass, global -> registers -> the wave's LDS strip in 16-byte pieces, every load issued
//      before the first use (clamped index, no load under a branch);
//   2. the scale table of the pass, one entry per scale group, built once from the block headers in LDS: Q4_K / Q5_K
//      (d * sc, dmin * m) per 32 columns out of the 6-bit packing, Q6_K d * sc per 16 columns, Q8_0 / Q4_0 d per block,
//      Q2_K (d * (sc & 15), dmin * (sc >> 4)) and Q3_K d * (sc - 32) per 16 columns.
//      All of these products are exact in f32;
//   3. the decode: lane l of step k owns the 16 / ES consecutive columns (64 k + l) * 16 / ES .. of the pass — one
//      16-byte store per lane, 1024 contiguous bytes per wave store. Consecutive columns of one scale group are
//      consecutive code bytes under one nibble / bit-pair selector in every format, so a lane reads 4 code bytes per 4
//      columns (plus 4 high-bit bytes for Q5_K / Q6_K) and one table entry, and the two halves of a code byte are taken
//      by different lanes (32 columns apart in Q4_K / Q5_K, 64 in Q6_K, 16 in Q4_0) that read the same LDS word.
//      Q2_K / Q3_K: a block's 84 / 110 bytes are never split by value: a lane's four columns are four consecutive qs
//      bytes under one 2-bit selector (the four selectors of a byte are 32 columns apart, taken by other lanes), for
//      Q3_K plus the four hmask bytes of the same columns under one bit selector. Q2_K blocks lie on dword boundaries
//      (84 = 21 dwords), every read a whole aligned dword; Q3_K blocks of odd index start 2 bytes past one (110 = 27.5
//      dwords), so a lane reads the two aligned dwords around its four bytes and funnels them (v_alignbyte), and only
//      the table build, once per 16 columns, reads the 12 scale bytes and d as halfwords.
// The LDS strip is the wave's own: no workgroup barrier, the waves of a workgroup do not wait for each other.
constexpr int QSEG = 4096;

template <int TYPE> struct qfmt;   // BB bytes per block of BC columns; a table entry of TW floats per TC columns
template <> struct qfmt<Q2A_TYPE_Q2_K> { static constexpr int BB = 84, BC = 256, TC = 16, TW = 2; };
template <> struct qfmt<Q2A_TYPE_Q3_K> { static constexpr int BB = 110, BC = 256, TC = 16, TW = 1; };
template <> struct qfmt<Q2A_TYPE_Q4_K> { static constexpr int BB = 144, BC = 256, TC = 32, TW = 2; };
template <> struct qfmt<Q2A_TYPE_Q5_K> { static constexpr int BB = 176, BC = 256, TC = 32, TW = 2; };
template <> struct qfmt<Q2A_TYPE_Q6_K> { static constexpr int BB = 210, BC = 256, TC = 16, TW = 1; };
template <> struct qfmt<Q2A_TYPE_Q8_0> { static constexpr int BB = 34, BC = 32, TC = 32, TW = 1; };
template <> struct qfmt<Q2A_TYPE_Q4_0> { static constexpr int BB = 18, BC = 32, TC = 32, TW = 1; };

// LDS traffic of one wave, ordered for all its lanes: what was written in front is seen by every lane behind
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float h2f(uint32_t h) { return (float) __builtin_bit_cast(_Float16, (uint16_t) h); }   // exact, subnormals too
// four consecutive bytes at a 4-byte / a 2-byte aligned LDS address (Q6_K, Q8_0 and Q4_0 blocks are only 2-byte aligned)
__device__ __forceinline__ uint32_t lds4(const uint8_t * p) { return *(const uint32_t *) p; }
__device__ __forceinline__ uint32_t lds2x2(const uint8_t * p) {
    const uint16_t * q = (const uint16_t *) p;
    return (uint32_t) q[0] | ((uint32_t) q[1] << 16);
}

// four consecutive bytes at a 2-byte aligned LDS address as two aligned dword reads and a funnel shift (the dword behind
// must be readable: true of every qs / hmask position of a Q3_K block, whose last 14 bytes are scales and d)
__device__ __forceinline__ uint32_t lds4_funnel(const uint8_t * p) {
    const uint32_t a = (uint32_t) (uintptr_t) p & 3u;
    const uint32_t * q = (const uint32_t *) (p - a);
    return __builtin_amdgcn_alignbyte(q[1], q[0], a);
}

// the scale table of `cols` columns of blocks at L
template <int TYPE>
__device__ __forceinline__ void q_build_tab(const uint8_t * L, float * tab, int cols, int lane) {
    using F = qfmt<TYPE>;
    for (int e = lane; e < cols / F::TC; e += 64) {
        if constexpr (TYPE == Q2A_TYPE_Q4_K || TYPE == Q2A_TYPE_Q5_K) {
            // get_scale_min_k4 (ggml-quants.c:1898) of sub-block j on the header words {d | dmin << 16, scales[0..11]}
            const int b = e >> 3, j = e & 7, sh = 8 * (j & 3);
            const uint32_t * hw = (const uint32_t *) (L + b * F::BB);
            const uint32_t dd = hw[0], s0 = (hw[1] >> sh) & 0xFF, s1 = (hw[2] >> sh) & 0xFF, s2 = (hw[3] >> sh) & 0xFF;
            const uint32_t sc = j < 4 ? (s0 & 63) : ((s2 & 0xF) | ((s0 >> 6) << 4));
            const uint32_t m = j < 4 ? (s1 & 63) : ((s2 >> 4) | ((s1 >> 6) << 4));
            ((float2 *) tab)[e] = float2{h2f(dd & 0xFFFF) * (float) sc, h2f(dd >> 16) * (float) m};
        } else if constexpr (TYPE == Q2A_TYPE_Q2_K) {
            // header words: scales[16] = words 0..3, {d | dmin << 16} = word 20; both products exact (11 x 4 bits)
            const int j = e & 15;
            const uint32_t * hw = (const uint32_t *) (L + (e >> 4) * F::BB);
            const uint32_t sc = (hw[j >> 2] >> (8 * (j & 3))) & 0xFF, dd = hw[20];
            ((float2 *) tab)[e] = float2{h2f(dd & 0xFFFF) * (float) (sc & 0xF), h2f(dd >> 16) * (float) (sc >> 4)};
        } else if constexpr (TYPE == Q2A_TYPE_Q3_K) {
            // 6-bit scale j: low four bits in a nibble of scales[j % 8], high two in scales[8 + j % 4] (dequantize_row_q3_K's
            // aux words); the block is 2-byte aligned, its scale bytes read as halfwords
            const int j = e & 15;
            const uint8_t * blk = L + (e >> 4) * F::BB;
            const uint16_t * sh = (const uint16_t *) (blk + 96);
            auto byte = [&](int i) { return (uint32_t) (sh[i >> 1] >> (8 * (i & 1))) & 0xFFu; };
            const uint32_t lo4 = j < 8 ? (byte(j) & 0xF) : (byte(j - 8) >> 4);
            const uint32_t hi2 = (byte(8 + (j & 3)) >> (2 * (j >> 2))) & 3;
            tab[e] = h2f(*(const uint16_t *) (blk + 108)) * (float) ((int) (lo4 | (hi2 << 4)) - 32);
        } else if constexpr (TYPE == Q2A_TYPE_Q6_K) {
            const uint8_t * blk = L + (e >> 4) * F::BB;
            tab[e] = h2f(*(const uint16_t *) (blk + 208)) * (float) ((const int8_t *) blk)[192 + (e & 15)];
        } else {
            tab[e] = h2f(*(const uint16_t *) (L + e * F::BB));
        }
    }
}

// columns c .. c + 3 of the pass (c a multiple of 4), ggml's values
template <int TYPE>
__device__ __forceinline__ void q_decode4(const uint8_t * L, const float * tab, int c, float * y) {
    using F = qfmt<TYPE>;
    if constexpr (TYPE == Q2A_TYPE_Q4_K || TYPE == Q2A_TYPE_Q5_K) {
        // sub-block j: nibble j & 1 of qs[32 (j / 2) + l]; Q5_K adds bit j of qh[l] as bit 4. y = d1 * q - m1: d1 * q is
        // exact, so the fused form rounds once where ggml's subtraction does
        const int b = c >> 8, j = (c >> 5) & 7, l = c & 31;
        const uint8_t * blk = L + b * F::BB;
        const float2 dm = ((const float2 *) tab)[c >> 5];
        uint32_t wq = (lds4(blk + (TYPE == Q2A_TYPE_Q5_K ? 48 : 16) + 32 * (j >> 1) + l) >> (4 * (j & 1))) & 0x0F0F0F0Fu;
        if constexpr (TYPE == Q2A_TYPE_Q5_K) wq |= ((lds4(blk + 16 + l) >> j) & 0x01010101u) << 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) y[i] = __builtin_fmaf(dm.x, (float) ((wq >> (8 * i)) & 0xFF), -dm.y);
    } else if constexpr (TYPE == Q2A_TYPE_Q2_K) {
        // column k of a block: bit pair (k % 128) / 32 of qs[32 (k / 128) + k % 32]; y = dl * q - ml, ggml's multiply then
        // subtract, uncontracted
#pragma clang fp contract(off)
        const int b = c >> 8, k = c & 255;
        const uint8_t * blk = L + b * F::BB;
        const float2 dm = ((const float2 *) tab)[c >> 4];
        const uint32_t wq = (lds4(blk + 16 + 32 * (k >> 7) + (k & 31)) >> (2 * ((k >> 5) & 3))) & 0x03030303u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float t = dm.x * (float) ((wq >> (8 * i)) & 0xFF);
            y[i] = t - dm.y;
        }
    } else if constexpr (TYPE == Q2A_TYPE_Q3_K) {
        // the same pair from qs (block byte 32 on), the third bit = bit k / 32 of hmask[k % 32]; (d * (sc - 32)) * (q - 4)
        const int b = c >> 8, k = c & 255;
        const uint8_t * blk = L + b * F::BB;
        const float dl = tab[c >> 4];
        const uint32_t lo = (lds4_funnel(blk + 32 + 32 * (k >> 7) + (k & 31)) >> (2 * ((k >> 5) & 3))) & 0x03030303u;
        const uint32_t hi = (lds4_funnel(blk + (k & 31)) >> (k >> 5)) & 0x01010101u;
        const uint32_t wq = lo | (hi << 2);
#pragma unroll
        for (int i = 0; i < 4; ++i) y[i] = dl * (float) ((int) ((wq >> (8 * i)) & 0xFF) - 4);
    } else if constexpr (TYPE == Q2A_TYPE_Q6_K) {
        // run r of half h: nibble r / 2 of ql[64 h + 32 (r & 1) + l], bits 2 r .. 2 r + 1 of qh[32 h + l]; (d * sc) * (q - 32)
        const int b = c >> 8, h = (c >> 7) & 1, r = (c >> 5) & 3, l = c & 31;
        const uint8_t * blk = L + b * F::BB;
        const float ds = tab[c >> 4];
        const uint32_t lo = (lds2x2(blk + 64 * h + 32 * (r & 1) + l) >> (4 * (r >> 1))) & 0x0F0F0F0Fu;
        const uint32_t hi = (lds2x2(blk + 128 + 32 * h + l) >> (2 * r)) & 0x03030303u;
        const uint32_t wq = lo | (hi << 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) y[i] = ds * (float) ((int) ((wq >> (8 * i)) & 0xFF) - 32);
    } else if constexpr (TYPE == Q2A_TYPE_Q8_0) {
        const int b = c >> 5, l = c & 31;
        const float d = tab[b];
        const uint32_t wq = lds2x2(L + b * F::BB + 2 + l);
#pragma unroll
        for (int i = 0; i < 4; ++i) y[i] = (float) (int8_t) (wq >> (8 * i)) * d;
    } else {
        // Q4_0: columns 0..15 of a block are the low nibbles of qs[0..15], columns 16..31 the high ones
        const int b = c >> 5, l = c & 31;
        const float d = tab[b];
        const uint32_t wq = (lds2x2(L + b * F::BB + 2 + (l & 15)) >> (4 * (l >> 4))) & 0x0F0F0F0Fu;
#pragma unroll
        for (int i = 0; i < 4; ++i) y[i] = (float) ((int) ((wq >> (8 * i)) & 0xFF) - 8) * d;
    }
}

// f32 -> the 16 bits of a fp16 / bf16 destination, round to nearest even (the _to calls' rule; finite inputs for bf16)
template <int DT>
__device__ __forceinline__ uint32_t q_cvt16(float f) {
    if constexpr (DT == Q2A_DT_F16) {
        // the f32 value first, in a register of its own: folded into the conversion (v_fma_mixlo_f16 d, q, 0) the product
        // of a zero and a negative factor came out as +0 where ggml stores -0
        asm volatile("" : "+v"(f));
        return __builtin_bit_cast(uint16_t, (_Float16) f);
    }
    const uint32_t u = __builtin_bit_cast(uint32_t, f);
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

// ids: int64 (wide) or int32, loaded by the wave-uniform width. row16 / out_ld16: strides in 16-byte units.
template <int TYPE, int DT>
__global__ __launch_bounds__(256) void k_qrow_gather(const void * ids, int wide, int n, int64_t audio_id, const uint4 * rows,
                                                        int64_t vocab, int64_t row16, int n_cols, uint4 * out, int64_t out_ld16,
                                                        int32_t * report) {
    using F = qfmt<TYPE>;
    constexpr int EPL = DT == Q2A_DT_F32 ? 4 : 8;   // columns per lane and step: one 16-byte store
    constexpr int RAW16 = (QSEG / F::BC * F::BB + 15) / 16, NLD = (RAW16 + 63) / 64;
    __shared__ uint4 raw_s[4][RAW16];
    __shared__ float tab_s[4][QSEG / F::TC * F::TW];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const int t = blockIdx.x * 4 + w;
    if (t >= n) return;
    const int64_t id = wide ? ((const int64_t *) ids)[t] : (int64_t) ((const int32_t *) ids)[t];
    if (id == audio_id) return;
    if (id < 0 || id >= vocab) {
        if (lane == 0) { atomicAdd(report + 2, 1); atomicOr(report + 3, 2); }
        return;
    }
    uint4 * raw = raw_s[w];
    float * tab = tab_s[w];
    const uint8_t * L = (const uint8_t *) raw;
    const uint4 * src = rows + id * row16;
    uint4 * dst = out + (int64_t) t * out_ld16;
    for (int c0 = 0; c0 < n_cols; c0 += QSEG) {
        const int cols = n_cols - c0 < QSEG ? n_cols - c0 : QSEG;
        const int seg16 = (cols / F::BC * F::BB + 15) / 16;
        const uint4 * sp = src + (int64_t) (c0 / QSEG) * (QSEG / F::BC * F::BB / 16);
        // (the LDS writes are clamped like the loads, a lane past the end rewriting the last piece with its own bytes:
        // under a bound of their own, the compiler moved each load in behind it, one wait per piece)
        uint4 v[NLD];
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int k = lane + 64 * i;
            v[i] = sp[k < seg16 ? k : seg16 - 1];
        }
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int k = lane + 64 * i;
            raw[k < seg16 ? k : seg16 - 1] = v[i];
        }
        wave_lds_sync();
        q_build_tab<TYPE>(L, tab, cols, lane);
        wave_lds_sync();
        uint4 * dp = dst + c0 / EPL;
        for (int c = lane * EPL; c < cols; c += 64 * EPL) {
            float y[EPL];
            q_decode4<TYPE>(L, tab, c, y);
            uint4 o;
            if constexpr (EPL == 4) {
                o = uint4{__builtin_bit_cast(uint32_t, y[0]), __builtin_bit_cast(uint32_t, y[1]), __builtin_bit_cast(uint32_t, y[2]),
                          __builtin_bit_cast(uint32_t, y[3])};
            } else {
                q_decode4<TYPE>(L, tab, c + 4, y + 4);
                o = uint4{q_cvt16<DT>(y[0]) | (q_cvt16<DT>(y[1]) << 16), q_cvt16<DT>(y[2]) | (q_cvt16<DT>(y[3]) << 16),
                          q_cvt16<DT>(y[4]) | (q_cvt16<DT>(y[5]) << 16), q_cvt16<DT>(y[6]) | (q_cvt16<DT>(y[7]) << 16)};
            }
            dp[c / EPL] = o;
        }
        wave_lds_sync();   // the next pass overwrites the strip
    }
}

template <int TYPE, int DT>
void launch_gather_q(const q2a_embed_gather_q_args & a, hipStream_t s) {
    const int n = (int) a.n_tokens;
    hipLaunchKernelGGL((k_qrow_gather<TYPE, DT>), dim3((unsigned) ((n + 3) / 4)), dim3(256), 0, s, a.ids, a.width == 8 ? 1 : 0, n, a.audio_id,
                       (const uint4 *) a.rows, a.vocab, a.row_bytes / 16, (int) a.n_cols, (uint4 *) a.out, a.out_ld_bytes / 16, a.report);
}
template <int TYPE>
void launch_gather_q_dt(const q2a_embed_gather_q_args & a, hipStream_t s) {
    if (a.out_dt == Q2A_DT_F32) launch_gather_q<TYPE, Q2A_DT_F32>(a, s);
    else if (a.out_dt == Q2A_DT_F16) launch_gather_q<TYPE, Q2A_DT_F16>(a, s);
    else launch_gather_q<TYPE, Q2A_DT_BF16>(a, s);
}

}  // namespace

hipError_t q2a_launch_audio_token_rows(const q2a_ids_args & a, hipStream_t s) {
    if (!a.ids || (a.width != 4 && a.width != 8) || a.n_tokens < 1 || a.n_tokens > Q2A_IDS_MAX_TOKENS || a.n_feat < 0 ||
        !a.chunk_count || !a.report || (a.n_feat > 0 && !a.row_map))
        return hipErrorInvalidValue;
    const int n = (int) a.n_tokens, n_chunks = (n + CHUNK - 1) / CHUNK;
    if (a.width == 8) {
        hipLaunchKernelGGL(k_ids_count<int64_t>, dim3((unsigned) n_chunks), dim3(256), 0, s, (const int64_t *) a.ids, n, a.audio_id, a.chunk_count);
        hipLaunchKernelGGL(k_ids_place<int64_t>, dim3((unsigned) n_chunks), dim3(256), 0, s, (const int64_t *) a.ids, n, a.audio_id,
                           a.chunk_count, n_chunks, a.n_feat, a.row_map, a.report);
    } else {
        hipLaunchKernelGGL(k_ids_count<int32_t>, dim3((unsigned) n_chunks), dim3(256), 0, s, (const int32_t *) a.ids, n, a.audio_id, a.chunk_count);
        hipLaunchKernelGGL(k_ids_place<int32_t>, dim3((unsigned) n_chunks), dim3(256), 0, s, (const int32_t *) a.ids, n, a.audio_id,
                           a.chunk_count, n_chunks, a.n_feat, a.row_map, a.report);
    }
    return hipGetLastError();
}

hipError_t q2a_launch_embed_gather(const q2a_embed_gather_args & a, hipStream_t s) {
    if (!a.ids || (a.width != 4 && a.width != 8) || a.n_tokens < 1 || a.n_tokens > Q2A_IDS_MAX_TOKENS || !a.table || a.vocab < 1 ||
        !a.out || !a.report || a.row_bytes < 16 || a.row_bytes % 16 || a.table_ld_bytes % 16 || a.out_ld_bytes % 16 ||
        a.table_ld_bytes < a.row_bytes || a.out_ld_bytes < a.row_bytes || ((uintptr_t) a.table & 15) || ((uintptr_t) a.out & 15))
        return hipErrorInvalidValue;
    const int n = (int) a.n_tokens, row16 = (int) (a.row_bytes / 16);
    const dim3 grid((unsigned) ((n + 3) / 4));
    if (a.width == 8)
        hipLaunchKernelGGL(k_embed_gather<int64_t>, grid, dim3(256), 0, s, (const int64_t *) a.ids, n, a.audio_id, (const uint4 *) a.table,
                           a.vocab, a.table_ld_bytes / 16, (uint4 *) a.out, a.out_ld_bytes / 16, row16, a.report);
    else
        hipLaunchKernelGGL(k_embed_gather<int32_t>, grid, dim3(256), 0, s, (const int32_t *) a.ids, n, a.audio_id, (const uint4 *) a.table,
                           a.vocab, a.table_ld_bytes / 16, (uint4 *) a.out, a.out_ld_bytes / 16, row16, a.report);
    return hipGetLastError();
}

hipError_t q2a_launch_embed_gather_q(const q2a_embed_gather_q_args & a, hipStream_t s) {
    const int t = a.ggml_type;
    if (t != Q2A_TYPE_Q4_0 && t != Q2A_TYPE_Q8_0 && t != Q2A_TYPE_Q2_K && t != Q2A_TYPE_Q3_K && t != Q2A_TYPE_Q4_K && t != Q2A_TYPE_Q5_K &&
        t != Q2A_TYPE_Q6_K)
        return hipErrorInvalidValue;
    if (a.out_dt != Q2A_DT_F32 && a.out_dt != Q2A_DT_F16 && a.out_dt != Q2A_DT_BF16) return hipErrorInvalidValue;
    const int es = a.out_dt == Q2A_DT_F32 ? 4 : 2;
    if (!a.ids || (a.width != 4 && a.width != 8) || a.n_tokens < 1 || a.n_tokens > Q2A_IDS_MAX_TOKENS || !a.rows || a.vocab < 1 || !a.out ||
        !a.report || a.n_cols < 256 || a.n_cols % 256 || a.n_cols > (1 << 24) || a.row_bytes % 16 ||
        a.row_bytes < (int64_t) q2a_row_size(t, a.n_cols) || a.out_ld_bytes % 16 || a.out_ld_bytes < a.n_cols * es ||
        ((uintptr_t) a.rows & 15) || ((uintptr_t) a.out & 15))
        return hipErrorInvalidValue;
    switch (t) {
        case Q2A_TYPE_Q4_0: launch_gather_q_dt<Q2A_TYPE_Q4_0>(a, s); break;
        case Q2A_TYPE_Q8_0: launch_gather_q_dt<Q2A_TYPE_Q8_0>(a, s); break;
        case Q2A_TYPE_Q2_K: launch_gather_q_dt<Q2A_TYPE_Q2_K>(a, s); break;
        case Q2A_TYPE_Q3_K: launch_gather_q_dt<Q2A_TYPE_Q3_K>(a, s); break;
        case Q2A_TYPE_Q4_K: launch_gather_q_dt<Q2A_TYPE_Q4_K>(a, s); break;
        case Q2A_TYPE_Q5_K: launch_gather_q_dt<Q2A_TYPE_Q5_K>(a, s); break;
        default: launch_gather_q_dt<Q2A_TYPE_Q6_K>(a, s); break;
    }
    return hipGetLastError();
}
