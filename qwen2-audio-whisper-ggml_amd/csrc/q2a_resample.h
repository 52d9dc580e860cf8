// q2a_resample.h — host arithmetic of the native-rate PCM ingestion (q2a_ingest_*): the rational rate
// change to 16 kHz, the output length, and the coefficient bank of the Kaiser-windowed sinc. Host code only; shared by
// q2a_format.cpp (q2a_resampled_length, in both libraries) and the engine (the bank the kernel reads).
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

constexpr int Q2A_RS_OUT_RATE = 16000;
constexpr int Q2A_RS_Z = 64;                             // zero crossings of the sinc each side
constexpr double Q2A_RS_BETA = 14.769656459379492;       // Kaiser window
constexpr double Q2A_RS_RHO = 0.9475937167399596;        // cutoff as a fraction of the narrower Nyquist
constexpr int Q2A_RS_MAX_L = 640;

// 16000 / rate = L / M reduced; H = ceil(Z / s) taps each side of the centre, T = 2 H + 1 taps per phase,
// s = min(1, L / M). rate == 16000: L = M = 1, no filter (H = T = 0).
struct q2a_rs_plan {
    int L, M, H, T;
};

inline bool q2a_rs_plan_of(int rate, q2a_rs_plan & p) {
    if (rate < 8000 || rate > 192000) return false;
    int a = Q2A_RS_OUT_RATE, b = rate;
    while (b) { const int t = a % b; a = b; b = t; }
    p.L = Q2A_RS_OUT_RATE / a;
    p.M = rate / a;
    if (p.L > Q2A_RS_MAX_L) return false;
    if (rate == Q2A_RS_OUT_RATE) { p.H = p.T = 0; return true; }
    // Z / s = Z * max(L, M) / L
    const int den = p.M > p.L ? p.M : p.L;
    p.H = (Q2A_RS_Z * den + p.L - 1) / p.L;
    p.T = 2 * p.H + 1;
    return true;
}

// n_out = ceil(n_frames * 16000 / rate); -1 where the product leaves int64
inline int64_t q2a_rs_out_len(int64_t n_frames, int rate) {
    if (n_frames > (INT64_MAX - rate) / Q2A_RS_OUT_RATE) return -1;
    return (n_frames * Q2A_RS_OUT_RATE + rate - 1) / rate;
}

inline double q2a_rs_i0(double x) {   // power series: every term positive, converged well before 64 terms for x <= 15
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 64; ++k) { term *= q / ((double) k * k); sum += term; }
    return sum;
}

// g at t = num / L input samples (num an integer: k L - n M), 0 outside |s t| < Z. s t = num / max(L, M) exactly.
inline double q2a_rs_g(const q2a_rs_plan & p, int64_t num) {
    const int den = p.M > p.L ? p.M : p.L;
    const int64_t an = num < 0 ? -num : num;
    if (an >= (int64_t) Q2A_RS_Z * den) return 0.0;
    const double s = p.M > p.L ? (double) p.L / p.M : 1.0;
    const double u = (double) num / den;   // s t
    const double x = M_PI * Q2A_RS_RHO * u;
    const double sinc = num == 0 ? 1.0 : sin(x) / x;
    const double w = u / Q2A_RS_Z;
    return Q2A_RS_RHO * s * sinc * q2a_rs_i0(Q2A_RS_BETA * sqrt(1.0 - w * w)) / q2a_rs_i0(Q2A_RS_BETA);
}

// bank[r][j], r = n % L, j = 0 .. T-1: the coefficient of input frame floor(n M / L) - H + j for output n, computed in
// double and rounded once to f32
inline void q2a_rs_bank(const q2a_rs_plan & p, std::vector<float> & bank) {
    bank.assign((size_t) p.L * p.T, 0.f);
    for (int r = 0; r < p.L; ++r) {
        const int ph = (int) (((int64_t) r * p.M) % p.L);
        for (int j = 0; j < p.T; ++j)
            bank[(size_t) r * p.T + j] = (float) q2a_rs_g(p, (int64_t) (j - p.H) * p.L - ph);
    }
}
