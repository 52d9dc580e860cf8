// inputs_embeds on the device (include/q2a_encoder.h, the q2a_inputs_embeds_* section): the row map of the
// projector GEMM's row-map epilogue derived from input_ids, and the gather of the text rows from the embedding table.
//   k_ids_count / k_ids_place   stable compaction of the positions of audio_token_id: a count per chunk of tokens, then
//                               every workgroup sums the counts in front of its chunk and writes its positions. Two
//                               launches; no workgroup waits for another one's progress.
//   k_embed_gather              row t of the destination := row input_ids[t] of the table, a byte copy in 16-byte
//                               pieces; audio positions are left to the GEMM's epilogue.
#include <hip/hip_runtime.h>

#include <cstdint>

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
