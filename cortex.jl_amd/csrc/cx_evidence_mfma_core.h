// cx_evidence_mfma_core.h — the wave-level pieces that cx_evidence_mfma.hip (cx_log_evidence_mfma) and cx_learn_mfma.hip
// (cx_factor_beliefs_mfma, cx_factor_statistics_mfma) share: a sum of message records into upper tiles, the blocked Cholesky with its
// vector solve, X'y, a datum in both vector layouts.  All on the helpers of cx_mv64w_core.h; nothing here launches anything.
#pragma once
#include "cx_mv64w_core.h"

namespace cx {
namespace evm {

using namespace w64;

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) x += __shfl_xor(x, m, 64);
    return x;
}

// M (upper tiles) += the Λ of the message records srcs[0 .. n); wcv[j] += their η[16 j + c]
template <int NT>
__device__ __forceinline__ void add_sources(d4 (&M)[NT * (NT + 1) / 2], double (&wcv)[NT], const double *__restrict__ f2v, const int32_t *__restrict__ srcs, int n,
                                            int mo, int c) {
    constexpr int KD = 16 * NT, KM = KD + KD * KD;
    for (int s = 0; s < n; s++) {
        const gcdp p = (gcdp)(f2v + (int64_t)srcs[s] * KM);
#pragma unroll
        for (int a = 0; a < NT; a++)
#pragma unroll
            for (int b = a; b < NT; b++)
#pragma unroll
                for (int r = 0; r < 4; r++) M[utn<NT>(a, b)][r] += p[KD + mo + tile_const_n<NT>(a, b, r)];
#pragma unroll
        for (int j = 0; j < NT; j++) wcv[j] += p[16 * j + c];
    }
}

// M = U'U in place (the off-diagonal tiles become U, V_k = U_kk⁻¹ goes to Vs), then z = U^-T w on the vector pipe (rule64_body's two
// passes).  logdet = Σ_{k < u} 2 log U_kk = -2 Σ log V_kk off the tile diagonals; quad = Σ_{k < u} z_k²; pd: every pivot below u is
// positive and finite.  zrv: z in the row layout (lane (g, c) holds z[16 j + g + 4 r]).
template <int NT>
__device__ __forceinline__ void factor_solve(d4 (&M)[NT * (NT + 1) / 2], const double (&wcv)[NT], double (&zrv)[NT][4], double *S, double (*Vs)[16 * kLdT],
                                             const int g, const int c, const int u, double &logdet, double &quad, bool &pd) {
    double ld = 0.0;
    bool bad = false;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // (an earlier factorisation's reads of S and Vs have returned)
#pragma unroll
    for (int k = 0; k < NT; k++) {
        const d4 Vk = diag_factor(M[utn<NT>(k, k)], S, g, c);
#pragma unroll
        for (int r = 0; r < 4; r++) Vs[k][(g + 4 * r) * kLdT + c] = Vk[r];
        // V[i][i] sits in lane (g, c) = (i & 3, i), register i >> 2
        const int rr = c >> 2;
        const double dv = rr == 0 ? Vk[0] : rr == 1 ? Vk[1] : rr == 2 ? Vk[2] : Vk[3];
        const bool on = g == (c & 3) && 16 * k + c < u, fine = dv > 0.0 && dv < __builtin_inf();
        bad = bad || (on && !fine);
        ld += log(on && fine ? dv : 1.0);
#pragma unroll
        for (int j = k + 1; j < NT; j++) M[utn<NT>(k, j)] = tts(Vk, M[utn<NT>(k, j)], d4{0.0, 0.0, 0.0, 0.0});
#pragma unroll
        for (int i = k + 1; i < NT; i++) {
            const d4 nu = neg(M[utn<NT>(k, i)]);
#pragma unroll
            for (int j = i; j < NT; j++) M[utn<NT>(i, j)] = tts(nu, M[utn<NT>(k, j)], M[utn<NT>(i, j)]);
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    double q = 0.0;
#pragma unroll
    for (int j = 0; j < NT; j++) {
        double w = wcv[j];
#pragma unroll
        for (int k = 0; k < j; k++) {
            double p = 0.0;
#pragma unroll
            for (int r = 0; r < 4; r++) p += M[utn<NT>(k, j)][r] * zrv[k][r];
            w -= sum_groups(p);
        }
        double p = 0.0;
#pragma unroll
        for (int r = 0; r < 4; r++) p += Vs[j][(g + 4 * r) * kLdT + c] * cv_to_rv(w, g, r);
        const double zcv = sum_groups(p);
#pragma unroll
        for (int r = 0; r < 4; r++) zrv[j][r] = cv_to_rv(zcv, g, r);
        q += (g == 0 && 16 * j + c < u) ? zcv * zcv : 0.0;
    }
    logdet = -2.0 * wave_sum(ld);
    quad = wave_sum(q);
    pd = __ballot(bad) == 0;
}

// out[a] (lane (g, c): entry 16 a + c) = (X' y)[16 a + c] for a row-major KD x KD matrix X and y in the row layout
template <int NT>
__device__ __forceinline__ void xty(const double *__restrict__ Xp, const double (&yrv)[NT][4], double (&out)[NT], const int mo) {
    constexpr int KD = 16 * NT;
    const gcdp X = (gcdp)Xp;
#pragma unroll
    for (int a = 0; a < NT; a++) {
        double p = 0.0;
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) p += X[mo + tile_const_n<NT>(j, a, r)] * yrv[j][r];
        out[a] = sum_groups(p);
    }
}
// a datum (the η part of a stored variable→factor record) in both layouts
template <int NT>
__device__ __forceinline__ void load_y(const double *__restrict__ y, double (&yrv)[NT][4], double (&ycv)[NT], const int g, const int c) {
#pragma unroll
    for (int j = 0; j < NT; j++) {
        ycv[j] = y[16 * j + c];
#pragma unroll
        for (int r = 0; r < 4; r++) yrv[j][r] = y[16 * j + g + 4 * r];
    }
}
// Σ_{k < u} a_k b_k of two vectors in the column layout (every lane group holds a copy: lane group 0 counts); the real block only, like
// every other quadratic form here
template <int NT>
__device__ __forceinline__ double dot_cv(const double (&a)[NT], const double (&b)[NT], const int g, const int c, const int u) {
    double p = 0.0;
#pragma unroll
    for (int j = 0; j < NT; j++) p += (g == 0 && 16 * j + c < u) ? a[j] * b[j] : 0.0;
    return wave_sum(p);
}

}  // namespace evm
}  // namespace cx
