// q2a_ingest.hip — native-rate PCM to the engine's 16 kHz mono f32 on the device: a polyphase Kaiser-windowed-sinc
// resampler (include/q2a_encoder.h q2a_ingest_*; the contract's host half is q2a_resample.h).
//
// Output n = q L + r of a clip reads the T input frames from floor(n M / L) - H on, against row r of the coefficient
// bank. A tile of consecutive outputs would need every row of the bank (227 KB at 44.1 kHz), so the work is split by
// residue instead: a workgroup owns P residues r0 .. r0+P-1 of Q consecutive periods q0 .. q0+Q-1 of one clip.
//   1. its P coefficient rows go to LDS once, tap-major ([Tp][P]), each row shifted right by the offset of its window
//      against the window of the first residue of its register group (zeros in front and behind);
//   2. the input span (Q - 1) M + T + the residues' spread is read once with coalesced loads, converted and downmixed
//      on the way, zero outside the clip, and laid out in polyphase order: frame k_rel at (k_rel % M) * Rw + k_rel / M;
//   3. a wave takes a register group — 4 residues of 64 periods (L >= 4), or one residue of 4 x 64 periods (L = 1, 2:
//      there are no 4 residues) — and its lanes take consecutive periods. At tap i every lane of the wave reads input
//      k_rel = c + i + q M: the same polyphase row, consecutive words, for every M (stride M in a plain layout would
//      conflict for M = 2, 6, 12); the coefficients of the tap are one broadcast read. 4 FMAs per 2 LDS reads (L >= 4),
//      4 per 5 (L < 4). Everything that walks the taps is wave-uniform scalar arithmetic; no branch on the clip's edges;
//   4. the accumulators go through an LDS tile [Q][P+1] and leave as runs of P consecutive samples per period (the whole
//      tile is one run where P = L).
// The order of the sum of an output is ascending k whatever the batch: a workgroup depends on its clip's own numbers
// only. f32 FMAs on the VALU: the f32 MFMA has no higher f32 rate on gfx950, and its operand here would be a Hankel view
// of one signal (every element loaded once per row it appears in).
#include "q2a_internal.h"

namespace {

constexpr int NT = 256;   // threads per workgroup (4 waves)

__device__ __forceinline__ float frame_at(const void * __restrict__ src, int format, int channels, int64_t k) {
    if (format == Q2A_PCM_S16) {
        const int16_t * s = (const int16_t *) src;
        if (channels == 1) return (float) s[k] * (1.0f / 32768.0f);                 // exact, = float(s) / 32768
        return (float) ((int) s[2 * k] + (int) s[2 * k + 1]) * (1.0f / 65536.0f);   // exact, = float(l + r) / 65536
    }
    const float * f = (const float *) src;
    if (channels == 1) return f[k];
    return 0.5f * (f[2 * k] + f[2 * k + 1]);
}

// WIDE = false: R = 4 residues x U = 1 period per lane; true: R = 1 x U = 4
template <bool WIDE>
__global__ __launch_bounds__(NT) void k_ingest(const q2a_ingest_geom g, const float * __restrict__ bank,
                                               const q2a_ingest_clip * __restrict__ clips) {
    constexpr int R = WIDE ? 1 : 4, U = WIDE ? 4 : 1;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const q2a_ingest_clip c = clips[blockIdx.y];
    const int L = g.L, M = g.M, P = g.P, Tp = g.Tp, Rw = g.Rw, Q = g.Q;
    const int64_t n_per = ((int64_t) c.n_out + L - 1) / L;   // periods with an output
    const int group = blockIdx.x % g.n_groups;               // neighbours share a span through L2
    const int64_t q0 = (int64_t) (blockIdx.x / g.n_groups) * Q;
    if (q0 >= n_per) return;
    float * cl = lds;                        // [Tp][P]
    float * xl = cl + Tp * P;                // [M][Rw]
    float * yl = xl + (int64_t) M * Rw;      // [Q][P + 1]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r0 = group * P;
    const int off0 = r0 * M / L;
    const int64_t k0 = q0 * M + off0 - g.H;  // the span's first frame (may lie before the clip)

    {   // 1. coefficient rows (NT % P == 0: a thread stays on one row)
        const int rl = tid & (P - 1), r = r0 + rl;
        const int d = r * M / L - (r0 + (rl & ~(R - 1))) * M / L;
        const bool live = r < L;
        const float * row = bank + (int64_t) (live ? r : 0) * g.T - d;
        for (int idx = tid; idx < Tp * P; idx += NT) {
            const int j = (idx >> g.logP) - d;
            cl[idx] = live && j >= 0 && j < g.T ? row[idx >> g.logP] : 0.f;
        }
    }
    {   // 2. input span, polyphase
        int rem = tid % M, dv = tid / M;
        const int sr = NT % M, sd = NT / M;
        for (int kr = tid; kr < g.span; kr += NT) {
            const int64_t k = k0 + kr;
            xl[rem * Rw + dv] = k >= 0 && k < c.n_in ? frame_at(c.src, c.format, c.channels, k) : 0.f;
            rem += sr;
            dv += sd;
            if (rem >= M) { rem -= M; ++dv; }
        }
    }
    __syncthreads();

    // 3. the taps
    const int n_rg = P / R, n_items = n_rg * ((Q + 64 * U - 1) / (64 * U));
    for (int item = wave; item < n_items; item += NT / 64) {
        const int rg = item % n_rg, qb = item / n_rg * (64 * U);
        const int cg = (r0 + rg * R) * M / L - off0;   // this group's window against the span
        int ql[U];
#pragma unroll
        for (int u = 0; u < U; ++u) ql[u] = min(qb + lane + 64 * u, Q - 1);   // (lanes past the run: read, not stored)
        float acc[R][U];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int u = 0; u < U; ++u) acc[r][u] = 0.f;
        int rem = cg % M, a = rem * Rw + cg / M;
        const float * cp = cl + rg * R;
#pragma unroll 4
        for (int i = 0; i < Tp; ++i) {
            float cf[R], xs[U];
#pragma unroll
            for (int r = 0; r < R; ++r) cf[r] = cp[i * P + r];
#pragma unroll
            for (int u = 0; u < U; ++u) xs[u] = xl[a + ql[u]];
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int u = 0; u < U; ++u) acc[r][u] = __builtin_fmaf(cf[r], xs[u], acc[r][u]);
            a += Rw;
            if (++rem == M) { rem = 0; a -= M * Rw - 1; }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int qq = qb + lane + 64 * u;
            if (qq < Q) {
#pragma unroll
                for (int r = 0; r < R; ++r) yl[qq * (P + 1) + rg * R + r] = acc[r][u];
            }
        }
    }
    __syncthreads();

    // 4. the tile, P consecutive samples per period
    for (int idx = tid; idx < Q * P; idx += NT) {
        const int qq = idx >> g.logP, rl = idx & (P - 1);
        const int64_t n = (q0 + qq) * L + r0 + rl;
        if (r0 + rl < L && n < c.n_out) c.dst[n] = yl[qq * (P + 1) + rl];
    }
}

__global__ __launch_bounds__(NT) void k_ingest_convert(const q2a_ingest_clip * __restrict__ clips) {
    const q2a_ingest_clip c = clips[blockIdx.y];
    const int64_t n0 = (int64_t) blockIdx.x * (NT * 4) + threadIdx.x;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t n = n0 + u * NT;
        if (n < c.n_out) c.dst[n] = frame_at(c.src, c.format, c.channels, n);
    }
}

constexpr int LDS_MAX = 160 * 1024;

}  // namespace

bool q2a_ingest_geom_of(int L, int M, int H, int T, q2a_ingest_geom & g) {
    g = q2a_ingest_geom{};
    if (L < 1 || M < 1 || T < 1 || L == 3) return false;
    g.L = L; g.M = M; g.H = H; g.T = T;
    g.wide = L < 4;
    const int R = g.wide ? 1 : 4, U = g.wide ? 4 : 1;
    int P = g.wide ? L : 16;
    while (!g.wide && P > 4 && P / 2 >= L) P /= 2;
    for (; P >= (g.wide ? 1 : 4); P /= 2) {
        // floor(a + b) - floor(a) <= ceil(b): the largest shift inside a register group, and of a group in the span
        const int dmax = (int) (((int64_t) (R - 1) * M + L - 1) / L);
        const int spread = (int) (((int64_t) (P - 1) * M + L - 1) / L);
        const int Tp = T + dmax;
        for (int Q = g.wide ? 64 * U * (4 / L) : 64; Q >= 1; --Q) {
            const int64_t span = spread + (int64_t) (Q - 1) * M + Tp;
            const int64_t Rw = ((span + M - 1) / M) | 1;
            const int64_t words = (int64_t) Tp * P + M * Rw + (int64_t) Q * (P + 1);
            if (words * 4 > LDS_MAX) continue;
            g.P = P; g.Q = Q; g.Tp = Tp; g.span = (int) span; g.Rw = (int) Rw;
            g.logP = 0;
            while ((1 << g.logP) < P) ++g.logP;
            g.n_groups = (L + P - 1) / P;
            g.lds_bytes = (int) (words * 4);
            return true;
        }
        if (g.wide) break;
    }
    return false;
}

hipError_t q2a_launch_ingest(const q2a_ingest_geom & g, const float * bank, const q2a_ingest_clip * clips_dev, int n_clips,
                             int64_t max_n_out, hipStream_t s) {
    if (n_clips <= 0 || max_n_out <= 0) return hipSuccess;
    if (!bank || !clips_dev || n_clips > 65535 || g.lds_bytes <= 0 || g.lds_bytes > LDS_MAX) return hipErrorInvalidValue;
    const int64_t runs = ((max_n_out + g.L - 1) / g.L + g.Q - 1) / g.Q;
    if (runs * g.n_groups > INT32_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned) (runs * g.n_groups), (unsigned) n_clips);
    const auto kern = g.wide ? k_ingest<true> : k_ingest<false>;
    if (g.lds_bytes > 64 * 1024) {
        const hipError_t rc = hipFuncSetAttribute((const void *) kern, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);
        if (rc != hipSuccess) return rc;
    }
    hipLaunchKernelGGL(kern, grid, dim3(NT), (size_t) g.lds_bytes, s, g, bank, clips_dev);
    return hipGetLastError();
}

hipError_t q2a_launch_ingest_convert(const q2a_ingest_clip * clips_dev, int n_clips, int64_t max_n_out, hipStream_t s) {
    if (n_clips <= 0 || max_n_out <= 0) return hipSuccess;
    if (!clips_dev || n_clips > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned) ((max_n_out + NT * 4 - 1) / (NT * 4)), (unsigned) n_clips);
    hipLaunchKernelGGL(k_ingest_convert, grid, dim3(NT), 0, s, clips_dev);
    return hipGetLastError();
}
