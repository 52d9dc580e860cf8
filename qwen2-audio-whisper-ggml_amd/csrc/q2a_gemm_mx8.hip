// q2a_gemm_mx8.hip — the MXFP8 contract's weight GEMM for gfx950: C[M][N] = A[M][K] . W[N][K]^T with
// OCP e4m3 elements and one e8m0 scale per 32 along K on both sides, on v_mfma_scale_f32_16x16x128_f8f6f4 (f32
// accumulators chained over ascending 128-deep K-steps), with the bf16 contract's epilogues; and the quantizer that
// writes such an operand from bf16 rows.
//
// Operand layout of the instruction (diag/mfma_f8_layout.hip, mfma_f8_scale_map.hip, mfma_f8_opsel.hip):
// lane (i = lane & 15, g = lane >> 4) holds 32 bytes of row i; byte j is K = 64 (j >> 4) + 16 g + (j & 15) of the K-step.
// The scale operand of lane (i, s) covers K-block s (K = 32 s .. 32 s + 31) of row i, read from the byte op_sel names.
// One dword of a row's scale array holds the four codes of a K-step: every lane of row i loads it and shifts by 8 g.
//
// Tiling: BM x BN x 128 per workgroup of WM x WN waves, each wave 64 columns and BM / WM rows of 16x16 tiles; W is the
// instruction's A operand, the activations its B, so a lane holds 4 consecutive columns of one row (C^T tiles).
// 256x256 on 8 waves for whole rounds of a many-row launch, 128x128 on 4 waves for few rows and for the rows of the
// partial last round (q2a_launch_gemm_mx8). Two LDS stages; a stage is the A image then the W image, rows of 128 bytes
// (one K-step), filled by global_load_lds_dwordx4 with the swizzle on the global source.
//
// LDS image and banks. The 16-B chunk c (0..7) of tile row r sits at chunk c ^ ((r >> 1) & 7) of the row's 128 bytes. A
// fragment is two ds_read_b128: chunk g (bytes 0..15 of the lane) and chunk 4 + g (bytes 16..31). A ds_read_b128 is
// served 16 lanes at a time, 256 B = the 64 banks once: the 16 lanes of a group hold rows r0 .. r0 + 15 (r0 % 16 == 0)
// and one chunk c. Row r begins at bank 32 (r & 1): the rows of one parity share a 128-B bank half and differ in
// (r >> 1) & 7, which the swizzle turns into eight different chunks — sixteen rows on sixteen different 16-B bank
// groups, conflict-free (the rule holds for any 8 consecutive lanes as well). The write side needs no rule: glds
// writes lane-linear, 1 KiB = 8 whole rows per instruction, and the lane that fills chunk pc of row r fetches global
// chunk pc ^ ((r >> 1) & 7), so eight lanes still read one whole 128-B global line.
#include "q2a_internal.h"
#include "q2a_quant.h"

#include <algorithm>

namespace {

typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void * lds_ptr_t;

constexpr int KS = 128;   // K-step = bytes per LDS row

// ggml_vec_gelu_f32 with GGML_GELU_FP16 (the lookup of the fused GEMM's GELU epilogues)
__device__ __forceinline__ float gelu_lut(float x, const uint16_t * tab) {
    const _Float16 h = (_Float16) x;
    uint16_t u;
    __builtin_memcpy(&u, &h, 2);
    const uint16_t g = __ldg(tab + u);
    _Float16 gh;
    __builtin_memcpy(&gh, &g, 2);
    return x <= -10.0f ? 0.0f : x >= 10.0f ? x : (float) gh;
}

__device__ __forceinline__ uint16_t bf16_bits(float v) { return __builtin_bit_cast(uint16_t, (__bf16) v); }

// the 32 bytes of lane (i, g) for tile row `row` of an image
__device__ __forceinline__ v8i frag8(const char * img, int row, int g) {
    const int sw = (row >> 1) & 7;
    const v4i lo = *(const v4i *) (img + row * KS + ((g ^ sw) << 4));
    const v4i hi = *(const v4i *) (img + row * KS + (((4 + g) ^ sw) << 4));
    return v8i{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

template <int BM, int BN, int WM, int WN, int EPI>
__global__ __launch_bounds__(WM * WN * 64, 1) void k_gemm_mx8(const q2a_gemm_args p, const uint8_t * __restrict__ a_scale,
                                                              const uint8_t * __restrict__ w_scale) {
    constexpr int NW = WM * WN, WR = BM / WM, WC = BN / WN;
    constexpr int MI = WR / 16, NJ = WC / 16;
    static_assert(WC == 64, "a wave owns 64 columns (one head of the QKV epilogue)");
    constexpr int LA = BM / 8 / NW, LB = BN / 8 / NW;   // glds instructions per wave per stage
    constexpr int OPB = (BM + BN) * KS;                 // one stage: A image | W image
    constexpr int VS = WR + 4;                          // V^T staging: bf16 per d-row
    constexpr int EPI_LDS = EPI == Q2A_EPI_QKV ? NW * 64 * VS * 2 : 0;
    constexpr int LDS_BYTES = 2 * OPB > EPI_LDS ? 2 * OPB : EPI_LDS;
    static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
    __shared__ __attribute__((aligned(16))) char lds_raw[LDS_BYTES];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int l16 = lane & 15, q = lane >> 4;
    // consecutive workgroups walk the N tiles of one row block: they share its A panel through L2
    const int nbn = p.N / BN;
    const int tm = blockIdx.x / nbn, tn = blockIdx.x - tm * nbn;
    const int m0 = p.m_base + tm * BM, n0 = tn * BN;
    const int nsc = p.K / 32;   // scale bytes per row

    // per-lane sources of this wave's glds instructions: 8 rows per instruction, 8 lanes per row, the swizzle on the
    // source chunk (rows past M clamp to M - 1: loaded, never stored)
    const uint8_t * A8 = (const uint8_t *) p.A;
    const uint8_t * W8 = (const uint8_t *) p.W;
    int64_t arow[LA], wrow[LB];
#pragma unroll
    for (int i = 0; i < LA; ++i) {
        const int r = (wave * LA + i) * 8 + (lane >> 3);
        arow[i] = (int64_t) min(m0 + r, p.M - 1) * p.K + (((lane & 7) ^ ((r >> 1) & 7)) << 4);
    }
#pragma unroll
    for (int i = 0; i < LB; ++i) {
        const int r = (wave * LB + i) * 8 + (lane >> 3);
        wrow[i] = (int64_t) (n0 + r) * p.K + (((lane & 7) ^ ((r >> 1) & 7)) << 4);
    }
    auto stage = [&](char * buf, int k0) {
#pragma unroll
        for (int i = 0; i < LA; ++i)
            __builtin_amdgcn_global_load_lds((const void *) (A8 + arow[i] + k0), (lds_ptr_t) (buf + (wave * LA + i) * 8 * KS), 16, 0, 0);
#pragma unroll
        for (int i = 0; i < LB; ++i)
            __builtin_amdgcn_global_load_lds((const void *) (W8 + wrow[i] + k0), (lds_ptr_t) (buf + (BM + (wave * LB + i) * 8) * KS), 16, 0, 0);
    };
    // the K-step's four scale codes of this lane's rows, one dword each (lanes of one row read the same dword)
    const uint32_t * asc[MI];
    const uint32_t * wsc[NJ];
#pragma unroll
    for (int i = 0; i < MI; ++i) asc[i] = (const uint32_t *) (a_scale + (int64_t) min(m0 + wm * WR + i * 16 + l16, p.M - 1) * nsc);
#pragma unroll
    for (int j = 0; j < NJ; ++j) wsc[j] = (const uint32_t *) (w_scale + (int64_t) (n0 + wn * WC + j * 16 + l16) * nsc);
    uint32_t sa[MI], sw[NJ];
    auto scales = [&](int kt) {
#pragma unroll
        for (int i = 0; i < MI; ++i) sa[i] = asc[i][kt];
#pragma unroll
        for (int j = 0; j < NJ; ++j) sw[j] = wsc[j][kt];
    };

    f4 acc[MI][NJ];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

    const int nk = p.K / KS;
    stage(lds_raw, 0);
    scales(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const char * ia = lds_raw + (kt & 1) * OPB;
        const char * iw = ia + BM * KS;
        // this step's scale codes: K-block g of the lane's row in the low byte (op_sel 0)
        int ca[MI], cw[NJ];
#pragma unroll
        for (int i = 0; i < MI; ++i) ca[i] = (int) (sa[i] >> (8 * q));
#pragma unroll
        for (int j = 0; j < NJ; ++j) cw[j] = (int) (sw[j] >> (8 * q));
        // the next step's images into the other stage (its last readers passed the barrier that ended step kt - 1)
        if (kt + 1 < nk) {
            stage(lds_raw + ((kt + 1) & 1) * OPB, (kt + 1) * KS);
            scales(kt + 1);
        }
        v8i wf[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) wf[j] = frag8(iw, wn * WC + j * 16 + l16, q);
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const v8i af = frag8(ia, wm * WR + i * 16 + l16, q);
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[j], af, acc[i][j], 0, 0, 0, cw[j], 0, ca[i]);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    // ---- epilogue: lane holds columns n = cbase + 16 j + 4 q + r of row m = rbase + 16 i + l16
    const int rbase = m0 + wm * WR, cbase = n0 + wn * WC;
    f4 bias4[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
        bias4[j] = EPI == Q2A_EPI_STORE_F ? f4{0.f, 0.f, 0.f, 0.f} : *(const f4 *) (p.bias + cbase + j * 16 + 4 * q);
    if constexpr (EPI == Q2A_EPI_STORE_F) {
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const int m = rbase + i * 16 + l16;
            if (m >= p.M) continue;
#pragma unroll
            for (int j = 0; j < NJ; ++j) *(f4 *) (p.outF + (int64_t) m * p.ldo + cbase + j * 16 + 4 * q) = acc[i][j];
        }
    } else if constexpr (EPI == Q2A_EPI_RESID) {
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const int m = rbase + i * 16 + l16;
            if (m >= p.M) continue;
            float * xr = p.outF + (int64_t) m * p.ldo + cbase + 4 * q;
            f4 add[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) add[j] = *(const f4 *) (xr + 16 * j);
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
#pragma clang fp contract(off)
                f4 v;
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = (acc[i][j][r] + bias4[j][r]) + add[j][r];   // (acc + bias) + x
                *(f4 *) (xr + 16 * j) = v;
            }
        }
    } else if constexpr (EPI == Q2A_EPI_GELU_H) {
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const int m = rbase + i * 16 + l16;
            if (m >= p.M) continue;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                uint16_t h[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) h[r] = bf16_bits(gelu_lut(acc[i][j][r] + bias4[j][r], p.gelu_tab));
                *(uint2 *) (p.outH + (int64_t) m * p.ldo + cbase + j * 16 + 4 * q) =
                    make_uint2(h[0] | ((uint32_t) h[1] << 16), h[2] | ((uint32_t) h[3] << 16));
            }
        }
    } else {
        static_assert(EPI == Q2A_EPI_QKV, "epilogues: QKV, RESID, GELU_H, STORE_F");
        const int part = cbase / p.D;   // q | k | v: uniform per wave (D % 64 == 0)
        const float vscale = part == 0 ? p.qscale : 1.0f;
        auto val = [&](int i, int j, int r) -> float {
#pragma clang fp contract(off)
            float v = acc[i][j][r] + bias4[j][r];
            v = v * vscale;   // ggml_scale after the bias add, exact 2^-3
            return v;
        };
        if (part < 2) {
            q2a_half * dst = part == 0 ? p.qh : p.kh;
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                const int m = rbase + i * 16 + l16;
                if (m >= p.M) continue;
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    uint16_t h[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) h[r] = bf16_bits(val(i, j, r));
                    *(uint2 *) (dst + (int64_t) m * p.D + cbase - part * p.D + j * 16 + 4 * q) =
                        make_uint2(h[0] | ((uint32_t) h[1] << 16), h[2] | ((uint32_t) h[3] << 16));
                }
            }
        }
        // V^T [clip][head][d][TP] (the image Q2A_BLK_BF16 writes): the wave's WR rows (t) of its 64 columns (d, one head)
        // staged [d][t] in the wave's own LDS region, then stored as runs of 4 t (8 B) along a d-row. The barrier is the
        // workgroup's: every wave is past its last read of the operand images
        __syncthreads();
        if (part == 2) {
            uint16_t * wl = (uint16_t *) lds_raw + wave * 64 * VS;
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) wl[(j * 16 + 4 * q + r) * VS + i * 16 + l16] = bf16_bits(val(i, j, r));
            // wave-private region, written by one lane mapping and read by another: the wave's LDS writes before its reads
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int h = (cbase - 2 * p.D) >> 6;
            for (int idx = lane; idx < 64 * (WR / 4); idx += 64) {
                const int d = idx / (WR / 4), ml = 4 * (idx - d * (WR / 4)), m = rbase + ml;
                if (m >= p.M) continue;
                const int clip = m / p.T, t = m - clip * p.T;
                q2a_half * vd = p.vt + (((int64_t) clip * p.H + h) * 64 + d) * p.TP;
                const uint16_t * src = wl + d * VS + ml;
                if (m + 3 < p.M && t + 3 < p.T && (t & 3) == 0) {
                    *(uint2 *) (vd + t) = *(const uint2 *) src;
                } else {   // a run that crosses a clip's end, the last rows, or T % 4 != 0: element by element
                    for (int e = 0; e < 4 && m + e < p.M; ++e) {
                        const int c2 = (m + e) / p.T, t2 = m + e - c2 * p.T;
                        ((uint16_t *) p.vt)[(((int64_t) c2 * p.H + h) * 64 + d) * p.TP + t2] = src[e];
                    }
                }
            }
        }
    }
}

// bf16 rows -> MXFP8: a thread takes 8 consecutive elements (16 B), four threads one 32-block
__global__ __launch_bounds__(256) void k_quant_mx8(const q2a_half * __restrict__ X, int64_t nchunks, uint8_t * __restrict__ out,
                                                   uint8_t * __restrict__ sc) {
    const int64_t c = (int64_t) blockIdx.x * 256 + threadIdx.x;
    // (nchunks % 4 == 0 and the grid's threads come in fours: a block's four lanes are all here or all gone)
    if (c >= nchunks) return;
    const uint4 raw = ((const uint4 *) X)[c];
    const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
    float v[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {   // bf16 -> f32: the bits, shifted
        v[2 * i] = __uint_as_float(w[i] << 16);
        v[2 * i + 1] = __uint_as_float(w[i] & 0xFFFF0000u);
    }
    float amax = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(v[i]));
    amax = fmaxf(amax, __shfl_xor(amax, 1));
    amax = fmaxf(amax, __shfl_xor(amax, 2));
    const uint32_t code = mx8_code(amax);
    const float inv = mx8_inv(code);
    ((uint2 *) out)[c] = make_uint2(mx8_pack4(v[0], v[1], v[2], v[3], inv), mx8_pack4(v[4], v[5], v[6], v[7], inv));
    if ((c & 3) == 0) sc[c >> 2] = (uint8_t) code;
}

template <int BM, int BN, int WM, int WN, int EPI>
hipError_t launch_tiles(const q2a_gemm_args & a, const uint8_t * a_scale, const uint8_t * w_scale, int m_base, int m_end, hipStream_t s) {
    q2a_gemm_args b = a;
    b.m_base = m_base;
    b.M = m_end;   // rows [m_base, m_end): the guard, the clamp and the grid read M as the end
    const int nbm = (m_end - m_base + BM - 1) / BM;
    if (nbm <= 0) return hipSuccess;
    hipLaunchKernelGGL((k_gemm_mx8<BM, BN, WM, WN, EPI>), dim3((unsigned) (nbm * (a.N / BN))), dim3(WM * WN * 64), 0, s, b, a_scale, w_scale);
    return hipGetLastError();
}

// rows [0, m_main) on 256x256 tiles: the whole rounds of one tile per compute unit; the rest on 128x128 tiles
int wide_rows(int M, int N) {
    if (N % 256) return 0;
    const int cus = q2a_cu_count();
    const int tpr = N / 256, fb = M / 256;
    if (cus <= 0 || fb * tpr < cus) return 0;
    return (fb - ((fb * tpr) % cus) / tpr) * 256;
}

template <int EPI>
hipError_t launch_epi(const q2a_gemm_args & a, const uint8_t * a_scale, const uint8_t * w_scale, hipStream_t s) {
    const int m_main = wide_rows(a.M, a.N);
    if (m_main > 0) {
        const hipError_t e = launch_tiles<256, 256, 2, 4, EPI>(a, a_scale, w_scale, 0, m_main, s);
        if (e != hipSuccess) return e;
    }
    return launch_tiles<128, 128, 2, 2, EPI>(a, a_scale, w_scale, m_main, a.M, s);
}

}  // namespace

hipError_t q2a_launch_gemm_mx8(const q2a_gemm_args & a, const uint8_t * a_scale, const uint8_t * w_scale, int epi, hipStream_t s) {
    if (a.M <= 0 || a.N <= 0 || a.N % 128 || a.K <= 0 || a.K % 128 || !a.A || !a.W || !a_scale || !w_scale) return hipErrorInvalidValue;
    if (((uintptr_t) a.A | (uintptr_t) a.W) & 15 || ((uintptr_t) a_scale | (uintptr_t) w_scale) & 3) return hipErrorInvalidValue;
    if (epi != Q2A_EPI_STORE_F && !a.bias) return hipErrorInvalidValue;
    switch (epi) {
        case Q2A_EPI_QKV:
            if (!a.qh || !a.kh || !a.vt || a.N != 3 * a.D || a.D % 64 || a.T <= 0 || a.TP < a.T) return hipErrorInvalidValue;
            return launch_epi<Q2A_EPI_QKV>(a, a_scale, w_scale, s);
        case Q2A_EPI_RESID:
            if (!a.outF || a.ldo < a.N) return hipErrorInvalidValue;
            return launch_epi<Q2A_EPI_RESID>(a, a_scale, w_scale, s);
        case Q2A_EPI_GELU_H:
            if (!a.outH || !a.gelu_tab || a.ldo < a.N) return hipErrorInvalidValue;
            return launch_epi<Q2A_EPI_GELU_H>(a, a_scale, w_scale, s);
        case Q2A_EPI_STORE_F:
            if (!a.outF || a.ldo < a.N) return hipErrorInvalidValue;
            return launch_epi<Q2A_EPI_STORE_F>(a, a_scale, w_scale, s);
        default:
            return hipErrorInvalidValue;
    }
}

hipError_t q2a_launch_quant_mx8(const q2a_half * X, int M, int K, uint8_t * out, uint8_t * sc, hipStream_t s) {
    if (M <= 0 || K <= 0 || K % 32 || !X || !out || !sc) return hipErrorInvalidValue;
    const int64_t nchunks = (int64_t) M * K / 8;
    hipLaunchKernelGGL(k_quant_mx8, dim3((unsigned) ((nchunks + 255) / 256)), dim3(256), 0, s, X, nchunks, out, sc);
    return hipGetLastError();
}
