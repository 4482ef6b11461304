// cx_functional_mfma.hip — cx_linear_moments_mfma: cx_linear_moments at the matrix-core dims (cx_create dim 5 .. 64): the
// exact mean and covariance of K linear functionals φ_k(x) = Σ_i w_{k,i}' x_i of cx_sample_posterior_mfma's q(x) (§4r), from the stored
// factor→variable messages and the data.  The derivation is DESIGN.md §4s.
//
// The sampler's draw is x = x⁰ + B ε: x_q = G_q x_par(q) + off_q + U_q⁻¹ ε_q down the rooted forest (cx_sample_mfma_core.h).  So
// E φ = W x⁰ and Cov(φ) = (B'W')'(B'W'), and B' is the same plan run leaf-to-root on PANELS of 16 functionals in place of 16 samples:
//
//   k_fnm_mean       one block per functional: Σ w·x⁰ over its entries (x⁰: the sampler's scan with one panel and zero noise), the datum
//                    of an observed variable; compensated, fixed tree; the status of the components it touches
//   k_fnm_scatter    u[position][functional of the chunk][KD] = w: the layout of z (the host has merged repeated variables)
//   per light depth, deepest first:
//     k_fnm_inject   one wave per (position with light paths, panel): u_q += Σ G_c' t_c over their heads c, in path order
//     k_spm_compose  the sampler's own kernel with no panel: the tiles' composed G (used transposed)
//     k_fnm_compose  level l: one wave per (tile item, panel) composes s ↦ o + P' s tail-to-head from zero
//     k_fnm_walk     <TOP> one wave per (path, panel) from zero at the tail; level l .. 1 from each item's carry; level 1 leaves
//                    t_q = u_q + (what the rest of the path pulls) in u
//   k_fnm_noise      one wave per (position, panel): g = U_q^-T t_q, zero in a failed component, kept for all K as [position][K][KD]
//   k_fnm_cov        one wave per (block of kCovPos positions, panel pair of the lower triangle): Σ_q Σ_a tts(g_P1[a], g_P2[a])
//   k_fnm_cov_final  the blocks in index order, compensated; NaN rows and columns of the failed functionals; the mirror image
//
// THE TRANSPOSED TILES.  The links are stored for tts(T, S) = T'S, so that apply_g computes G Z.  Here G' Z and U^-T t are needed: the
// same stored tiles with rows and columns exchanged.  They are LOADED with the transposed lane mapping, and the contraction index of a
// tile product is renumbered so that every lane reads 32 contiguous bytes: a panel here has lane (g, c) register r = component 4 g + r
// (not g + 4 r) of functional c, the operand of row block a and column block b has lane (g, c) register s = element
// (16 a + 4 (c & 3) + (c >> 2), 16 b + 4 g + s) of the stored matrix, and the product comes out in the same panel layout (§4s shows
// why).  No LDS, no second copy of the links.
//
// Every (item, panel column) sum has a fixed order that does not depend on K: a functional's numbers do not depend on which others
// share the call or on how the call is cut into chunks, and two calls on one state are bit-identical.  No atomics.  UNCENTRED, like
// the sampler: §4r's note on data far from the origin applies unchanged.
#include "cx_sample_mfma_core.h"

namespace cx {
namespace fnm {

using namespace w64;
using sp::kT;
using spm::get_panel, spm::kPanel, spm::LR, spm::put_panel;

constexpr int kCovPos = 256;                        // positions per block of k_fnm_cov: fixed, so that no sum depends on K
constexpr int64_t kMaxG = (int64_t)1 << 30;         // doubles of g kept per call (8 GiB)
constexpr int64_t kMaxPart = (int64_t)1 << 28;      // (k, l) block partials of the covariance per call (2 GiB)

// ---- a panel of 16 functionals: lane (g, c) register r of tile b = component 16 b + 4 g + r of functional c -----------------------
template <int NT>
__device__ __forceinline__ void get_u(const double *__restrict__ U, const int64_t q, const int64_t Kc, const int64_t col0, d4 (&Z)[NT], const int g, const int c) {
    constexpr int KD = 16 * NT;
    const gcdp o = (gcdp)(U + (q * Kc + col0 + c) * KD + 4 * g);
#pragma unroll
    for (int b = 0; b < NT; b++)
#pragma unroll
        for (int r = 0; r < 4; r++) Z[b][r] = o[16 * b + r];
}
template <int NT>
__device__ __forceinline__ void put_u(double *__restrict__ U, const int64_t q, const int64_t Kc, const int64_t col0, const d4 (&Z)[NT], const int g, const int c) {
    constexpr int KD = 16 * NT;
    gdp o = (gdp)(U + (q * Kc + col0 + c) * KD + 4 * g);
#pragma unroll
    for (int b = 0; b < NT; b++)
#pragma unroll
        for (int r = 0; r < 4; r++) o[16 * b + r] = Z[b][r];
}
// the lane's part of every transposed operand: row 4 (c & 3) + (c >> 2) of the stored tile, columns 4 g ..
template <int NT>
__device__ __forceinline__ int adj_lane(const int g, const int c) { return (4 * (c & 3) + (c >> 2)) * (16 * NT) + 4 * g; }

// Z <- N + M Z for a stored row-major KD x KD matrix M (G' of a link, U^-T, a tile's composed G'); LOWER: M is lower block triangular
template <int NT, bool LOWER>
__device__ __forceinline__ void adj_apply(const gcdp M, d4 (&Z)[NT], d4 (&N)[NT], const int mt) {
    constexpr int KD = 16 * NT;
#pragma unroll
    for (int a = 0; a < NT; a++) {
#pragma unroll
        for (int b = 0; b < (LOWER ? a + 1 : NT); b++) {
            d4 T;
#pragma unroll
            for (int s = 0; s < 4; s++) T[s] = M[mt + 16 * a * KD + 16 * b + s];
            N[a] = tts(T, Z[b], N[a]);
        }
    }
#pragma unroll
    for (int a = 0; a < NT; a++) Z[a] = N[a];
}
template <int NT>
__device__ __forceinline__ void zero(d4 (&Z)[NT]) {
#pragma unroll
    for (int a = 0; a < NT; a++) Z[a] = d4{0.0, 0.0, 0.0, 0.0};
}

// ---- the means and the status of every functional -----------------------------------------------------------------------------------
// Z: the sampler's z of one panel (S = 16) under zero noise; column 0 is x⁰
__global__ __launch_bounds__(kT) void k_fnm_mean(int u, int kd, const int64_t *__restrict__ foff, const int32_t *__restrict__ fvar, const double *__restrict__ fw,
                                                 const uint8_t *__restrict__ vinfo, const int32_t *__restrict__ dslot, const int32_t *__restrict__ var_pos,
                                                 const int32_t *__restrict__ comp, const uint8_t *__restrict__ cflag, const uint8_t *__restrict__ cimp,
                                                 const double *__restrict__ v2f, const double *__restrict__ Z, ev::Part *__restrict__ part) {
    double s = 0.0, c = 0.0;
    unsigned bad = 0;
    for (int64_t e = foff[blockIdx.x] + threadIdx.x; e < foff[blockIdx.x + 1]; e += kT) {
        const int32_t v = fvar[e];
        const double *x = nullptr;
        if (vinfo[v] & kClamped) {
            if (dslot[v] >= 0) x = v2f + (int64_t)dslot[v] * ((int64_t)kd * (kd + 1));
            else bad = 1;      // (an observed variable on no connection has no datum)
        } else {
            const int32_t q = var_pos[v], cc = comp[q];
            if (cflag[cc] | cimp[cc]) bad = 1;
            else x = Z + (int64_t)q * kPanel * kd;
        }
        double t = 0.0;
        if (x)
            for (int k = 0; k < u; k++) t += fw[e * u + k] * x[k];
        if (!bad) ev::neu(s, c, t);
    }
    ev::block_part<kT>(bad ? 0.0 : s, bad ? 0.0 : c, bad, 0, 0, 0, part);
}

// ---- u <- the weights: one thread per (entry e0 .. e0 + n of the chunk's functionals k0 .., component below the user's dim) ----------
__global__ __launch_bounds__(kT) void k_fnm_scatter(int64_t n, int64_t e0, int k0, int64_t Kc, int u, int kd, const int32_t *__restrict__ fvar,
                                                    const int32_t *__restrict__ ffun, const double *__restrict__ fw, const uint8_t *__restrict__ vinfo,
                                                    const int32_t *__restrict__ var_pos, double *__restrict__ U) {
    const int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (t >= n * u) return;
    const int64_t e = e0 + t / u;
    const int k = (int)(t % u);
    const int32_t v = fvar[e];
    if (vinfo[v] & kClamped) return;      // (an observed variable: the mean only)
    U[((int64_t)var_pos[v] * Kc + (ffun[e] - k0)) * kd + k] = fw[e * u + k];
}

// ---- u_q += Σ G_c' t_c over the light paths on q, in path order: one wave per (position q0 + j, panel) ------------------------------
template <int NT>
__global__ __launch_bounds__(64) void k_fnm_inject(int64_t q0, int64_t n, int np, const int32_t *__restrict__ att_off, const int32_t *__restrict__ att_head,
                                                   const double *__restrict__ link, double *__restrict__ U) {
    const int64_t j = blockIdx.x / np;
    const int x = (int)(blockIdx.x - j * np);
    if (j >= n) return;
    const int64_t q = q0 + j, Kc = (int64_t)np * kPanel;
    const int32_t b = att_off[q], e = att_off[q + 1];
    if (b == e) return;
    const int lane = threadIdx.x, g = lane >> 4, c = lane & 15, mt = adj_lane<NT>(g, c);
    d4 N[NT];
    get_u<NT>(U, q, Kc, x * kPanel, N, g, c);
    for (int32_t a = b; a < e; a++) {
        const int64_t hd = att_head[a];
        d4 Z[NT];
        get_u<NT>(U, hd, Kc, x * kPanel, Z, g, c);
        adj_apply<NT, false>((gcdp)(link + hd * LR<NT>::N + LR<NT>::GT), Z, N, mt);
    }
    put_u<NT>(U, q, Kc, x * kPanel, N, g, c);
}

// ---- the blocked scan, tail to head -------------------------------------------------------------------------------------------------
// s_i = G_i'(u_i + s_{i+1}) is what position i hands to the one before it.  A tile [a, b) maps s_b to s_a = o + P' s_b with
// P = G_{b-1} .. G_a, the sampler's tile matrix: Gc holds P' row-major, as k_spm_compose leaves it.  oc and carry: [item][panel] panels
template <int NT, bool POS>
__global__ __launch_bounds__(64) void k_fnm_compose(int64_t n, int np, const int2 *__restrict__ rng, const double *__restrict__ link, const double *__restrict__ U,
                                                    const double *__restrict__ Gb, const double *__restrict__ ob, double *__restrict__ oc) {
    constexpr int KD = 16 * NT;
    const int64_t j = blockIdx.x / np;
    const int x = (int)(blockIdx.x - j * np);
    if (j >= n) return;
    const int lane = threadIdx.x, g = lane >> 4, c = lane & 15, mt = adj_lane<NT>(g, c);
    const int64_t Kc = (int64_t)np * kPanel;
    const int2 r = rng[j];
    d4 S[NT];
    zero<NT>(S);
    for (int32_t i = r.y - 1; i >= r.x; i--) {
        d4 N[NT];
        if constexpr (POS) {
            get_u<NT>(U, i, Kc, x * kPanel, N, g, c);
#pragma unroll
            for (int a = 0; a < NT; a++) S[a] += N[a];
            zero<NT>(N);
            adj_apply<NT, false>((gcdp)(link + (int64_t)i * LR<NT>::N + LR<NT>::GT), S, N, mt);
        } else {
            get_panel<NT>(ob, (int64_t)i * np + x, N, lane);
            adj_apply<NT, false>((gcdp)(Gb + (int64_t)i * KD * KD), S, N, mt);
        }
    }
    put_panel<NT>(oc, j * np + x, S, lane);
}

// TOP: item j is a path, top[j].xy the range of its top-level items, the carry in at its tail is zero; otherwise the carry of item j of
// this level.  POS: the children are positions (u_q becomes t_q), else items of the level below (their carries written to cb)
template <int NT, bool POS, bool TOP>
__global__ __launch_bounds__(64) void k_fnm_walk(int64_t n, int np, const int4 *__restrict__ top, const int2 *__restrict__ rng, const double *__restrict__ carry,
                                                 const double *__restrict__ link, const double *__restrict__ Gb, const double *__restrict__ ob,
                                                 double *__restrict__ cb, double *__restrict__ U) {
    constexpr int KD = 16 * NT;
    const int64_t j = blockIdx.x / np;
    const int x = (int)(blockIdx.x - j * np);
    if (j >= n) return;
    const int lane = threadIdx.x, g = lane >> 4, c = lane & 15, mt = adj_lane<NT>(g, c);
    const int64_t Kc = (int64_t)np * kPanel;
    d4 S[NT];
    int32_t b, e;
    if constexpr (TOP) {
        const int4 p = top[j];
        b = p.x; e = p.y;
        zero<NT>(S);
    } else {
        const int2 r = rng[j];
        b = r.x; e = r.y;
        get_panel<NT>(carry, j * np + x, S, lane);
    }
    for (int32_t i = e - 1; i >= b; i--) {
        d4 N[NT];
        if constexpr (POS) {
            get_u<NT>(U, i, Kc, x * kPanel, N, g, c);
#pragma unroll
            for (int a = 0; a < NT; a++) S[a] += N[a];
            put_u<NT>(U, i, Kc, x * kPanel, S, g, c);
            zero<NT>(N);
            adj_apply<NT, false>((gcdp)(link + (int64_t)i * LR<NT>::N + LR<NT>::GT), S, N, mt);
        } else {
            put_panel<NT>(cb, (int64_t)i * np + x, S, lane);
            get_panel<NT>(ob, (int64_t)i * np + x, N, lane);
            adj_apply<NT, false>((gcdp)(Gb + (int64_t)i * KD * KD), S, N, mt);
        }
    }
}

// ---- the noise coordinates g_q = U_q^-T t_q, zero in a failed component: one wave per (position, panel) ------------------------------
// G: [position][Kp][KD], Kp the call's functionals in whole panels; the chunk's first functional is k0
template <int NT>
__global__ __launch_bounds__(64) void k_fnm_noise(int64_t npos, int np, int64_t k0, int64_t Kp, const double *__restrict__ link, const int32_t *__restrict__ comp,
                                                  const uint8_t *__restrict__ cflag, const uint8_t *__restrict__ cimp, const double *__restrict__ U,
                                                  double *__restrict__ G) {
    const int64_t q = blockIdx.x / np;
    const int x = (int)(blockIdx.x - q * np);
    if (q >= npos) return;
    const int lane = threadIdx.x, g = lane >> 4, c = lane & 15, mt = adj_lane<NT>(g, c);
    d4 Z[NT], N[NT];
    zero<NT>(N);
    const int32_t cc = comp[q];
    if (!(cflag[cc] | cimp[cc])) {
        get_u<NT>(U, q, (int64_t)np * kPanel, x * kPanel, Z, g, c);
        adj_apply<NT, true>((gcdp)(link + q * LR<NT>::N + LR<NT>::UT), Z, N, mt);
    }
    put_u<NT>(G, q, Kp, k0 + x * kPanel, N, g, c);
}

// ---- cov[k][l] = Σ_q g_q^k · g_q^l -----------------------------------------------------------------------------------------------------
// wave = (a block of kCovPos positions, a panel pair (pi, pj <= pi) of the lower triangle), the pair fastest.  Two accumulators, the even
// and the odd positions of the block: the order is fixed.  part: [block][pair][lane][4], lane (g, c) register r = (16 pi + g + 4 r, 16 pj + c)
template <int NT>
__global__ __launch_bounds__(64) void k_fnm_cov(int64_t npos, int64_t Kp, int npair, const double *__restrict__ G, double *__restrict__ part) {
    const int64_t blk = blockIdx.x / npair;
    int pi = 0, pj = (int)(blockIdx.x - blk * npair);
    while (pj > pi) { pj -= pi + 1; pi++; }
    const int lane = threadIdx.x, g = lane >> 4, c = lane & 15;
    const int64_t q0 = blk * kCovPos, q1 = q0 + kCovPos < npos ? q0 + kCovPos : npos;
    d4 acc[2] = {d4{0.0, 0.0, 0.0, 0.0}, d4{0.0, 0.0, 0.0, 0.0}};
    for (int64_t q = q0; q < q1; q += 2) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            if (q + h >= q1) break;
            d4 T[NT], S[NT];
            get_u<NT>(G, q + h, Kp, (int64_t)pi * kPanel, T, g, c);
            get_u<NT>(G, q + h, Kp, (int64_t)pj * kPanel, S, g, c);
#pragma unroll
            for (int a = 0; a < NT; a++) acc[h] = tts(T[a], S[a], acc[h]);
        }
    }
    gdp o = (gdp)(part + (int64_t)blockIdx.x * 256);
#pragma unroll
    for (int r = 0; r < 4; r++) o[4 * lane + r] = acc[0][r] + acc[1][r];
}

__global__ __launch_bounds__(kT) void k_fnm_cov_final(int64_t nblk, int K, int npair, const double *__restrict__ part, const ev::Part *__restrict__ fpart,
                                                      double *__restrict__ cov) {
    const int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (t >= (int64_t)K * K) return;
    const int k = (int)(t / K), l = (int)(t - (int64_t)k * K);
    if (l > k) return;
    const int pi = k >> 4, pj = l >> 4, kk = k & 15;
    const int64_t at = ((int64_t)pi * (pi + 1) / 2 + pj) * 256 + 4 * ((kk & 3) * 16 + (l & 15)) + (kk >> 2);
    double s = 0.0, c = 0.0;
    for (int64_t b = 0; b < nblk; b++) ev::neu(s, c, part[b * npair * 256 + at]);
    const double v = fpart[k].n[0] || fpart[l].n[0] ? __builtin_nan("") : s + c;
    cov[(int64_t)k * K + l] = v;
    cov[(int64_t)l * K + k] = v;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
using spm::blocks;

// x⁰ into P.d_Z (one panel, zero noise) and the means; the links and the statuses first
template <int NT>
void launch_mean(cx_handle *h, spm::Plan &P, int K) {
    // n_valid = 0: every column of the panel gets exact zero noise.  (A caller's-noise pointer that is never read: no Philox either)
    const spm::Gen g{P.d_link.get(), h->nv, 0, 0, 0, mfr::user_dim(h)};
    spm::launch_cond<NT>(h, P);
    spm::launch_samples<NT>(h, P, kPanel, g);
    hipLaunchKernelGGL(k_fnm_mean, dim3((unsigned)K), dim3(kT), 0, h->stream, mfr::user_dim(h), h->cfg.dim, P.d_foff, P.d_fvar, P.d_fw, h->d_vinfo, P.d_dslot,
                       P.d_var_pos, P.d_comp, P.d_cflag, P.d_cimp, h->d_mv_v2f, P.d_Z, P.d_fpart);
}

// the adjoint scan of the chunk's Kc functionals (np panels) from functional k0 on, entries e0 .. e0 + ne; g into P.d_fg
template <int NT>
void launch_adjoint(cx_handle *h, spm::Plan &P, int64_t k0, int64_t Kc, int64_t Kp, int64_t e0, int64_t ne) {
    constexpr int KD = 16 * NT;
    const int np = (int)(Kc / kPanel), u = mfr::user_dim(h);
    const spm::Gen none{nullptr, 0, 0, 0, 0, u};
    (void)hipMemsetAsync(P.d_Z, 0, (size_t)(P.npos * Kc * KD) * sizeof(double), h->stream);
    if (ne)
        hipLaunchKernelGGL(k_fnm_scatter, dim3(blocks(ne * u, kT)), dim3(kT), 0, h->stream, ne, e0, (int)k0, Kc, u, KD, P.d_fvar, P.d_ffun, P.d_fw, h->d_vinfo,
                           P.d_var_pos, P.d_Z);
    for (size_t di = P.depths.size(); di-- > 0;) {
        const sp::Depth &dp = P.depths[di];
        if (dp.n_att)
            hipLaunchKernelGGL(k_fnm_inject<NT>, dim3((unsigned)((dp.pos_end - dp.pos_beg) * np)), dim3(64), 0, h->stream, dp.pos_beg, dp.pos_end - dp.pos_beg, np,
                               P.d_att_off, P.d_att_head, P.d_link, P.d_Z);
        for (int l = 1; l <= dp.levels; l++) {
            const int64_t n = dp.n_items[(size_t)l - 1];
            const int2 *rng = P.d_rng + dp.rng_off[(size_t)l - 1];
            // the tiles' composed G: the sampler's kernel with no panel (wave x of an item: block column x of the product)
            if (l == 1) {
                hipLaunchKernelGGL((spm::k_spm_compose<NT, true>), dim3((unsigned)(n * NT)), dim3(64), 0, h->stream, n, 0, rng, P.d_link, P.d_pos_var, none, nullptr,
                                   nullptr, P.d_Gc[1], P.d_oc[1]);
                hipLaunchKernelGGL((k_fnm_compose<NT, true>), dim3((unsigned)(n * np)), dim3(64), 0, h->stream, n, np, rng, P.d_link, P.d_Z, nullptr, nullptr,
                                   P.d_oc[1]);
            } else {
                hipLaunchKernelGGL((spm::k_spm_compose<NT, false>), dim3((unsigned)(n * NT)), dim3(64), 0, h->stream, n, 0, rng, P.d_link, P.d_pos_var, none,
                                   P.d_Gc[(size_t)l - 1], P.d_oc[(size_t)l - 1], P.d_Gc[(size_t)l], P.d_oc[(size_t)l]);
                hipLaunchKernelGGL((k_fnm_compose<NT, false>), dim3((unsigned)(n * np)), dim3(64), 0, h->stream, n, np, rng, P.d_link, P.d_Z,
                                   P.d_Gc[(size_t)l - 1], P.d_oc[(size_t)l - 1], P.d_oc[(size_t)l]);
            }
        }
        const int4 *top = P.d_top + dp.top_off;
        const int L = dp.levels;
        const unsigned gtop = (unsigned)(dp.n_paths * np);
        if (L == 0)
            hipLaunchKernelGGL((k_fnm_walk<NT, true, true>), dim3(gtop), dim3(64), 0, h->stream, dp.n_paths, np, top, nullptr, nullptr, P.d_link, nullptr, nullptr,
                               nullptr, P.d_Z);
        else
            hipLaunchKernelGGL((k_fnm_walk<NT, false, true>), dim3(gtop), dim3(64), 0, h->stream, dp.n_paths, np, top, nullptr, nullptr, P.d_link,
                               P.d_Gc[(size_t)L], P.d_oc[(size_t)L], P.d_carry[(size_t)L], P.d_Z);
        for (int l = L; l >= 1; l--) {
            const int64_t n = dp.n_items[(size_t)l - 1];
            const int2 *rng = P.d_rng + dp.rng_off[(size_t)l - 1];
            const unsigned grid = (unsigned)(n * np);
            if (l == 1)
                hipLaunchKernelGGL((k_fnm_walk<NT, true, false>), dim3(grid), dim3(64), 0, h->stream, n, np, nullptr, rng, P.d_carry[1], P.d_link, nullptr, nullptr,
                                   nullptr, P.d_Z);
            else
                hipLaunchKernelGGL((k_fnm_walk<NT, false, false>), dim3(grid), dim3(64), 0, h->stream, n, np, nullptr, rng, P.d_carry[(size_t)l], P.d_link,
                                   P.d_Gc[(size_t)l - 1], P.d_oc[(size_t)l - 1], P.d_carry[(size_t)l - 1], P.d_Z);
        }
    }
    if (P.npos)
        hipLaunchKernelGGL(k_fnm_noise<NT>, dim3((unsigned)(P.npos * np)), dim3(64), 0, h->stream, P.npos, np, k0, Kp, P.d_link, P.d_comp, P.d_cflag, P.d_cimp,
                           P.d_Z, P.d_fg);
}

template <int NT>
void launch_cov(cx_handle *h, spm::Plan &P, int K, int64_t Kp, int64_t nblk, int npair) {
    if (nblk) hipLaunchKernelGGL(k_fnm_cov<NT>, dim3((unsigned)(nblk * npair)), dim3(64), 0, h->stream, P.npos, Kp, npair, P.d_fg, P.d_fcpart);
    hipLaunchKernelGGL(k_fnm_cov_final, dim3(blocks((int64_t)K * K, kT)), dim3(kT), 0, h->stream, nblk, K, npair, P.d_fcpart, P.d_fpart, P.d_fcov);
}

}  // namespace fnm
}  // namespace cx

using namespace cxh;

extern "C" int32_t cx_linear_moments_mfma(cx_handle *h, int64_t n_functionals, const int64_t *offsets, const int64_t *variable_ids, const double *weights,
                                          double *mean, double *cov, int64_t *counts4) {
    const std::string who = "cx_linear_moments_mfma";
    try {
        namespace spm = cx::spm;
        namespace mfr = cx::mfr;
        namespace fnm = cx::fnm;
        int32_t rc;
        const int64_t K = n_functionals;
        const char *bad = nullptr;
        if (K < 0 || !offsets || !counts4 || (K > 0 && !mean)) bad = "n_functionals < 0, or null offsets, mean or counts4";
        else {
            bool mono = offsets[0] == 0;
            for (int64_t k = 0; k < K && mono; k++) mono = offsets[k + 1] >= offsets[k];
            if (!mono) bad = "offsets must start at 0 and never decrease";
            else if (offsets[K] > 0 && (!variable_ids || !weights)) bad = "null variable_ids or weights";
            else if (K > 32768) bad = "more than 32768 functionals";
        }
        if ((rc = mfr::prepare(h, who, bad, {"cx_linear_moments", "the variational and Beta-Bernoulli families have no Gaussian joint to take moments of", "links"})) != CX_OK)
            return rc;
        if ((rc = mv_ensure_chain_msgs(h)) != CX_OK) return rc;      // (every reader of d_mv_f2v calls this first)
        spm::Plan *Pp = nullptr;
        if ((rc = spm::plan_of(h, who, Pp)) != CX_OK) return rc;
        spm::Plan &P = *Pp;
        const int kd = h->cfg.dim, d = mfr::user_dim(h);
        const int64_t nnz = offsets[K];
        // the entries by variable index; a variable named more than once in a functional becomes one entry, its weights added in the
        // order given (the scatter then writes every (position, functional) once: no atomics)
        std::vector<int64_t> foff((size_t)K + 1, 0);
        std::vector<int32_t> fvar, ffun;
        std::vector<double> fw;
        fvar.reserve((size_t)nnz); ffun.reserve((size_t)nnz); fw.reserve((size_t)nnz * d);
        std::vector<std::pair<int32_t, int64_t>> ent;
        for (int64_t k = 0; k < K; k++) {
            ent.clear();
            for (int64_t e = offsets[k]; e < offsets[k + 1]; e++) {
                const int64_t v = find_var(h, variable_ids[e]);
                if (v < 0) return fail(h, CX_ERR_NOT_FOUND, who + ": no variable " + std::to_string(variable_ids[e]));
                ent.push_back({(int32_t)v, e});
            }
            std::stable_sort(ent.begin(), ent.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
            for (size_t i = 0; i < ent.size(); i++) {
                if (i && ent[i].first == ent[i - 1].first) {
                    for (int j = 0; j < d; j++) fw[fw.size() - (size_t)d + (size_t)j] += weights[ent[i].second * d + j];
                    continue;
                }
                fvar.push_back(ent[i].first);
                ffun.push_back((int32_t)k);
                for (int j = 0; j < d; j++) fw.push_back(weights[ent[i].second * d + j]);
            }
            foff[(size_t)k + 1] = (int64_t)fvar.size();
        }
        int64_t n_nan = 0;
        if (K > 0) {
            // functionals in chunks of whole panels that keep u and the level buffers under 2^27 doubles, cx_sample.hip's bound; one panel
            // at the least.  CX_FN_MFMA_CHUNK (tests, A/B) sets the chunk: a call of more functionals runs in several, which must not
            // change a bit of the result
            const int64_t Kp = (K + spm::kPanel - 1) / spm::kPanel * spm::kPanel, npan = Kp / spm::kPanel;
            int64_t per = P.npos;
            for (size_t l = 1; l < P.level_cap.size(); l++) per += 2 * P.level_cap[l];
            per = std::max<int64_t>(per * kd, 1);
            int64_t chunk = std::max<int64_t>(spm::kPanel, std::min<int64_t>(Kp, ((int64_t)1 << 27) / per / spm::kPanel * spm::kPanel));
            if (const int64_t o = spm::chunk_override("CX_FN_MFMA_CHUNK")) chunk = std::min(o, Kp);
            CX_REQUIRE(h, P.npos * (chunk / spm::kPanel) < (int64_t)0x7fffff00, CX_ERR_UNSUPPORTED, who + ": more than 2^31 (position, panel) pairs in a chunk");
            if (cov && Kp * P.npos * kd > fnm::kMaxG)
                return fail(h, CX_ERR_OUT_OF_MEMORY, who + ": the noise coordinates of " + std::to_string(K) + " functionals over " + std::to_string(P.npos) +
                                                         " variables pass 2^30 doubles: ask for fewer functionals per call");
            const int64_t nblk = (P.npos + fnm::kCovPos - 1) / fnm::kCovPos, npair = npan * (npan + 1) / 2;
            if (cov && nblk * npair * 256 > fnm::kMaxPart)
                return fail(h, CX_ERR_OUT_OF_MEMORY, who + ": the block partials of a " + std::to_string(K) + " x " + std::to_string(K) + " covariance over " +
                                                         std::to_string(P.npos) + " variables pass 2^28 pairs: ask for fewer functionals per call");
            if ((rc = spm::ensure_chunk(h, P, cov ? chunk : spm::kPanel)) != CX_OK) return rc;
            if ((rc = P.d_foff.upload(h, foff)) != CX_OK || (rc = P.d_fvar.upload(h, fvar)) != CX_OK || (rc = P.d_ffun.upload(h, ffun)) != CX_OK ||
                (rc = P.d_fw.upload(h, fw)) != CX_OK || (rc = P.d_fpart.ensure(h, K)) != CX_OK) return rc;
            if (cov && ((rc = P.d_fg.ensure(h, std::max<int64_t>(Kp * P.npos * kd, 1))) != CX_OK || (rc = P.d_fcov.ensure(h, K * K)) != CX_OK ||
                        (rc = P.d_fcpart.ensure(h, std::max<int64_t>(nblk * npair, 1) * 256)) != CX_OK)) return rc;
            CX_HIP(h, hipStreamSynchronize(h->stream));
            mfr::for_tiles(kd, [&](auto nt) { fnm::launch_mean<decltype(nt)::value>(h, P, (int)K); });
            CX_HIP(h, hipGetLastError());
            std::vector<double> hcov;
            if (cov) {
                for (int64_t k0 = 0; k0 < Kp; k0 += chunk) {
                    const int64_t Kc = std::min<int64_t>(chunk, Kp - k0), k1 = std::min<int64_t>(k0 + Kc, K);
                    const int64_t e0 = foff[(size_t)k0], ne = foff[(size_t)k1] - e0;
                    mfr::for_tiles(kd, [&](auto nt) { fnm::launch_adjoint<decltype(nt)::value>(h, P, k0, Kc, Kp, e0, ne); });
                    CX_HIP(h, hipGetLastError());
                }
                mfr::for_tiles(kd, [&](auto nt) { fnm::launch_cov<decltype(nt)::value>(h, P, (int)K, Kp, nblk, (int)npair); });
                CX_HIP(h, hipGetLastError());
                // (through a host vector: a call that fails on the device leaves the caller's array as it was)
                hcov.resize((size_t)(K * K));
                CX_HIP(h, hipMemcpyAsync(hcov.data(), P.d_fcov, (size_t)(K * K) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            }
            std::vector<cx::ev::Part> part((size_t)K);
            CX_HIP(h, hipMemcpyAsync(part.data(), P.d_fpart, (size_t)K * sizeof(cx::ev::Part), hipMemcpyDeviceToHost, h->stream));
            CX_HIP(h, hipStreamSynchronize(h->stream));      // (the host vectors die here)
            if (cov) std::copy(hcov.begin(), hcov.end(), cov);
            for (int64_t k = 0; k < K; k++) {
                const bool failed = part[(size_t)k].n[0] != 0;
                n_nan += failed;
                mean[k] = failed ? std::nan("") : part[(size_t)k].s + part[(size_t)k].c;
            }
        } else {
            // no functional: the status alone
            mfr::for_tiles(kd, [&](auto nt) { spm::launch_cond<decltype(nt)::value>(h, P); });
            CX_HIP(h, hipGetLastError());
            CX_HIP(h, hipStreamSynchronize(h->stream));
        }
        if (P.n_comp) CX_HIP(h, hipMemcpy(P.h_cflag.data(), P.d_cflag, (size_t)P.n_comp, hipMemcpyDeviceToHost));
        int64_t failed = 0;
        for (int64_t c = 0; c < P.n_comp; c++) failed += P.h_cimp[(size_t)c] != 0 || P.h_cflag[(size_t)c] != 0;
        counts4[0] = P.n_comp;
        counts4[1] = failed;
        counts4[2] = n_nan;
        counts4[3] = P.npos;
        return CX_OK;
    } catch (const std::bad_alloc &) { return fail(h, CX_ERR_OUT_OF_MEMORY, who + ": host allocation failed"); }
}
