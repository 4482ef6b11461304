// cx_evidence_mfma_core.h — the wave kit of the readers of the stored messages at the matrix-core dims: cx_evidence_mfma.hip
// (cx_log_evidence_mfma), cx_learn_mfma.hip (cx_factor_beliefs_mfma, cx_factor_statistics_mfma), cx_predict_mfma.hip (cx_predictive_mfma)
// and cx_causal_mfma.hip (cx_causal_marginals_mfma); cx_sample_mfma.hip (cx_sample_posterior_mfma) factors and solves with it.  Sums of message records into upper tiles, the scan for NaN records, the blocked
// Cholesky with its vector solve, the block-column solve U^-T X, the pass S = T ± Y'Y with h = Y'z, the identity on the padding diagonal,
// the flat-pivot rule, the symmetric store through LDS, X'y, a datum in both vector layouts.  All on the helpers of cx_mv64w_core.h;
// every helper is inlined into its caller and launches nothing.  The compiler fences (the empty asm that keeps one block column or one
// tile in flight, the LDS waits) are inside the helpers, at the points of the source where the callers had them.  What that was shown
// to keep: every instantiation's register class, LDS, waves per SIMD and absence of scratch, and the outputs bit for bit.  The assembly
// is NOT what it was — hipcc schedules an inlined body differently (waits, scalar and integer instructions; k_cmm_rows has 20 to 39
// more s_waitcnt) — so a change here is checked by the resource report and the bits again (profiles/mfma_readers_kit.md, sections a to
// c), not taken on trust.  The host side, the kernel that folds row statuses included: cx_mfma_reader.h.
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

// the upper tiles of a row-major KD x KD table; ld(k): its element at the lane's place plus the constant k
template <int NT, class Ld>
__device__ __forceinline__ void load_upper(d4 (&M)[NT * (NT + 1) / 2], Ld ld) {
#pragma unroll
    for (int a = 0; a < NT; a++)
#pragma unroll
        for (int b = a; b < NT; b++)
#pragma unroll
            for (int r = 0; r < 4; r++) M[utn<NT>(a, b)][r] = ld(tile_const_n<NT>(a, b, r));
}

// M (upper tiles) += the Λ of n message records, wcv[j] += their η[16 j + c]; record_at(s): where record s lies
template <int NT, class At>
__device__ __forceinline__ void add_records(d4 (&M)[NT * (NT + 1) / 2], double (&wcv)[NT], int n, At record_at, int mo, int c) {
    constexpr int KD = 16 * NT;
    for (int s = 0; s < n; s++) {
        const gcdp p = (gcdp)record_at(s);
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
// the same of the stored message records srcs[0 .. n)
template <int NT>
__device__ __forceinline__ void add_sources(d4 (&M)[NT * (NT + 1) / 2], double (&wcv)[NT], const double *__restrict__ f2v, const int32_t *__restrict__ srcs, int n,
                                            int mo, int c) {
    constexpr int KD = 16 * NT, KM = KD + KD * KD;
    add_records<NT>(M, wcv, n, [&](int s) { return f2v + (int64_t)srcs[s] * KM; }, mo, c);
}

// `seen`, or Λ[0][0] or η[0] of a stored message record srcs[0 .. n) is NaN (whole messages are NaN together).  The inputs looked at
// themselves: a sum that a failed factorisation has already filled with NaN says nothing about them
template <int NT>
__device__ __forceinline__ bool any_nan_record(bool seen, const double *f2v, const int32_t *srcs, int n) {
    constexpr int KD = 16 * NT, KM = KD + KD * KD;
    for (int s = 0; s < n; s++) {
        const double *p = f2v + (int64_t)srcs[s] * KM;
        seen = seen || __builtin_isnan(p[0]) || __builtin_isnan(p[KD]);
    }
    return seen;
}

// the identity on the padding diagonal (entries u .. KD - 1) of an embedded dim: a sum of messages may be zero there, and the real block
// stays as it is.  Entry [i][i] of a diagonal tile sits in lane (g, c) = (i & 3, i), register i >> 2
template <int NT>
__device__ __forceinline__ void pad_identity(d4 (&M)[NT * (NT + 1) / 2], const int g, const int c, const int u) {
    const int rr = c >> 2;
#pragma unroll
    for (int j = 0; j < NT; j++) {
        const bool pad = g == (c & 3) && 16 * j + c >= u;
#pragma unroll
        for (int r = 0; r < 4; r++) M[utn<NT>(j, j)][r] += (pad && r == rr) ? 1.0 : 0.0;
    }
}

// The flat-pivot rule, after factor_solve, off the tile diagonals of V = U^-1 in Vs: a pivot below u at or below k_flat times the same
// diagonal entry of the sum of the stored message records srcs[0 .. n) — ALL messages into the variable — is flat: a message whose
// information is flat reaches a sum as the rounding of C - Yt'Yt, a number of either sign that must not pass for information
// (cx_predict.hip: kFlatPivot).  Lane c looks at entry 16 k + c; the caller ballots
template <int NT>
__device__ __forceinline__ bool flat_pivot(double (*Vs)[16 * kLdT], const double *__restrict__ f2v, const int32_t *__restrict__ srcs, int n, const int c,
                                           const int u, const double k_flat) {
    constexpr int KD = 16 * NT, KM = KD + KD * KD;
    bool flat = false;
#pragma unroll
    for (int k = 0; k < NT; k++) {
        double ref = 0.0;
        for (int s = 0; s < n; s++) ref += f2v[(int64_t)srcs[s] * KM + KD + (16 * k + c) * (KD + 1)];
        const double v = Vs[k][c * kLdT + c], piv = 1.0 / (v * v);      // V_kk = 1 / U_kk
        flat = flat || (16 * k + c < u && !(piv > k_flat * fmax(ref, 0.0)));
    }
    return flat;
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

// z waits in LDS between its solve and its use (Y'z), not in 8 NT registers across the matrix solve (rule64_body: Z_IN_LDS)
template <int NT>
__device__ __forceinline__ void park_z(double *ZS, const double (&zrv)[NT][4], const int g) {
#pragma unroll
    for (int j = 0; j < NT; j++)
#pragma unroll
        for (int r = 0; r < 4; r++) ZS[16 * j + g + 4 * r] = zrv[j][r];      // (the 16 lanes of a group write one value to one place)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// One block column: Yb = U^-T Yb from block row j0 on (the rows above are zero and stay so).  U: the off-diagonal tiles of M after
// factor_solve, V_k = U_kk⁻¹ in Vs
template <int NT>
__device__ __forceinline__ void solve_col(d4 (&Yb)[NT], const d4 (&M)[NT * (NT + 1) / 2], double (*Vs)[16 * kLdT], const int j0, const int g, const int c) {
#pragma unroll
    for (int j = j0; j < NT; j++) {
        d4 Vj;
#pragma unroll
        for (int r = 0; r < 4; r++) Vj[r] = Vs[j][(g + 4 * r) * kLdT + c];
        Yb[j] = tts(Vj, Yb[j], d4{0.0, 0.0, 0.0, 0.0});
#pragma unroll
        for (int jj = j + 1; jj < NT; jj++) Yb[jj] = tts(neg(M[utn<NT>(j, jj)]), Yb[j], Yb[jj]);
    }
}
// Y = U^-T X in registers, Y[b]: block column b, its tiles by block row.  ld(k): X's element at the lane's place plus the constant k,
// one block column of it in flight at a time.  IDENT: X = I, nothing is loaded, and of the lower block triangle Y only the tiles
// (j, b), j >= b, are written
template <int NT, bool IDENT, class Ld>
__device__ __forceinline__ void solve_block_cols(d4 (&Y)[NT][NT], const d4 (&M)[NT * (NT + 1) / 2], double (*Vs)[16 * kLdT], Ld ld, const int g, const int c) {
#pragma unroll
    for (int b = 0; b < NT; b++) {
        if (!IDENT) asm volatile("" ::: "memory");      // (one block column of X in flight at a time)
#pragma unroll
        for (int j = IDENT ? b : 0; j < NT; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) Y[b][j][r] = IDENT ? ((j == b && g + 4 * r == c) ? 1.0 : 0.0) : ld(tile_const_n<NT>(j, b, r));
        solve_col<NT>(Y[b], M, Vs, IDENT ? b : 0, g, c);
    }
}
// Y = U^-T, the lower block triangle
template <int NT>
__device__ __forceinline__ void solve_identity_cols(d4 (&Y)[NT][NT], const d4 (&M)[NT * (NT + 1) / 2], double (*Vs)[16 * kLdT], const int g, const int c) {
    solve_block_cols<NT, true>(Y, M, Vs, [](int) { return 0.0; }, g, c);
}

// Sm (upper tiles) = T + SIGN Y'Y and, block row by block row, h(a, (Y'z)[16 a + c]) with z from park_z; ld(k): T's element at the lane's
// place plus the constant k
template <int NT, int SIGN, class Ld, class H>
__device__ __forceinline__ void gram_pass(d4 (&Sm)[NT * (NT + 1) / 2], const d4 (&Y)[NT][NT], const double *ZS, Ld ld, H h, const int g) {
#pragma unroll
    for (int a = 0; a < NT; a++) {
#pragma unroll
        for (int b = a; b < NT; b++) {
            asm volatile("" ::: "memory");      // (one tile of T in flight at a time: hoisted together they cost 80 registers at NT = 4)
            d4 G = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int j = 0; j < NT; j++) G = tts(Y[a][j], Y[b][j], G);
#pragma unroll
            for (int r = 0; r < 4; r++) Sm[utn<NT>(a, b)][r] = SIGN > 0 ? ld(tile_const_n<NT>(a, b, r)) + G[r] : ld(tile_const_n<NT>(a, b, r)) - G[r];
        }
        double p = 0.0;
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) p += Y[a][j][r] * ZS[16 * j + g + 4 * r];
        h(a, sum_groups(p));
    }
}

// Tile (a, b), b >= a, of a symmetric matrix and its mirror image: the upper tile as it is, the lower one turned through the LDS tile S,
// a diagonal tile the mean of its two triangles, so that what is stored is symmetric to the last bit.  put(a, b, r, v): the store of
// entry (16 a + g + 4 r, 16 b + c)
template <class Put>
__device__ __forceinline__ void store_symmetric(const d4 D, const int a, const int b, double *S, Put put, const int g, const int c) {
    if (b > a) {
#pragma unroll
        for (int r = 0; r < 4; r++) put(a, b, r, D[r]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the previous tile's reads have returned
#pragma unroll
    for (int r = 0; r < 4; r++) S[(g + 4 * r) * kLdT + c] = D[r];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const double tr = S[c * kLdT + g + 4 * r];
        put(b, a, r, b > a ? tr : 0.5 * (D[r] + tr));
    }
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
