// cx_functional.hip — cx_linear_moments: the exact mean and covariance of K linear functionals φ_k(x) = Σ_i w_{k,i}' x_i of the posterior
// of a Gaussian forest (dim 1 .. 4), from the stored factor→variable messages.  No counterpart in the reference; DESIGN.md §4i.
//
// cx_sample_posterior's draw is x = c + z, z = z⁰ + F ε (cx_sample_core.h, §4g): z_q = G_q z_par(q) + off_q + M_q ε_q + Σ_x X_x ε_sib(x) down
// the rooted forest.  So E φ = W (c + z⁰) and Cov(φ) = (F'W')'(F'W'), and F' is the same plan run leaf-to-root:
//
//   k_fn_mean       one block per functional: Σ w·(c + z⁰) over its entries (z⁰: the sampler's forward scan with ε = 0, one "sample"),
//                   the datum of an observed variable; compensated, fixed tree; the status of the components it touches
//   k_fn_scatter    one thread per entry on a free variable: u[position][functional][d] = w (the host has merged repeated variables)
//   per light depth, deepest first, the reverse of the sampler's order:
//     k_fn_inject   one thread per (position, functional): u_q += Σ G_c' u_c over the heads c of the light paths that hang on q
//     k_fn_compose  level l: one thread per (tile of 64 items, functional) composes s ↦ o + P' s tail-to-head from zero; one more thread
//                   per tile the matrix product P (the sampler's, used transposed)
//     k_fn_walk<TOP> one thread per (path, functional): from zero at the tail over the top tiles, leaving every tile's carry
//     k_fn_walk     level l .. 1: from each tile's carry over its items, last to first; level 1 leaves u_q = the whole subtree's pull
//   k_fn_noise      one thread per (position, functional): g = M_q' u_q + Σ X_x' u_q' over the earlier siblings q' of a k-ary factor
//   k_fn_cov        per block of kCovPos positions and 16 x 16 tile of the lower triangle: Σ_q g_q^k · g_q^l, compensated
//   k_fn_cov_final  the blocks in index order; NaN rows and columns of the failed functionals; the mirror image
//
// u lies [position][functional][d]: the lanes of a tile read and write contiguous runs.  Every (item, functional) is one thread's work
// and every sum has a fixed order that does not depend on K: a functional's numbers do not depend on which others share the call, and
// two calls on one state are bit-identical.  No atomics.
//
// Functionals run in chunks that keep u and the level buffers under 2^27 doubles (the sampler's bound).  g is KEPT for all K
// ([position][K][d] doubles) so that cov across chunks needs no second scan; a call whose g would pass kMaxG doubles is refused
// (CX_ERR_OUT_OF_MEMORY), and so is one whose K x K block partials would pass kMaxPart.  cov == NULL skips the adjoint altogether.
#include "cx_sample_core.h"

#include <algorithm>

namespace cx {
namespace fn {

using ev::Lay;
using sp::kT;
using sp::LR;

constexpr int kCovPos = 2048;                       // positions per block of k_fn_cov: fixed, so that no sum depends on K
constexpr int kCovTile = 16;                        // a block's tile of (k, l) pairs: 16 x 16 threads
constexpr int64_t kMaxG = (int64_t)1 << 30;         // doubles of g kept per call (8 GiB)
constexpr int64_t kMaxPart = (int64_t)1 << 28;      // (s, c) block partials of the covariance per call (4 GiB)

// r = G_q' t
template <int D>
__device__ __forceinline__ void gt_mul(const double *__restrict__ g, const double (&t)[D], double (&r)[D]) {
#pragma unroll
    for (int j = 0; j < D; j++) {
        double u = 0.0;
#pragma unroll
        for (int i = 0; i < D; i++) u += g[i * D + j] * t[i];
        r[j] = u;
    }
}

// ---- the means and the status of every functional -------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(kT) void k_fn_mean(const int64_t *__restrict__ foff, const int32_t *__restrict__ fvar, const double *__restrict__ fw,
                                                const uint8_t *__restrict__ vinfo, const int32_t *__restrict__ dslot, const int32_t *__restrict__ var_pos,
                                                const int32_t *__restrict__ comp, const uint8_t *__restrict__ cflag, const double *__restrict__ v2f,
                                                const double *__restrict__ W, const double *__restrict__ Z, ev::Part *__restrict__ part) {
    constexpr int NT = Lay<D>::NT, K = Lay<D>::K;
    double s = 0.0, c = 0.0;
    unsigned bad = 0;
    for (int64_t e = foff[blockIdx.x] + threadIdx.x; e < foff[blockIdx.x + 1]; e += kT) {
        const int32_t v = fvar[e];
        double x[D];
        if (vinfo[v] & kClamped) ev::datum<D>(v2f, dslot[v], x);
        else {
            // (k_sp_gather's value with one sample)
            const int32_t q = var_pos[v];
            if (cflag[comp[q]]) bad = 1;
            const double *w = W + (int64_t)v * K;
            const bool pd = D == 1 ? w[D] > 0.0 : w[D + NT] != 0.0;
#pragma unroll
            for (int k = 0; k < D; k++) x[k] = (pd ? w[k] : 0.0) + Z[(int64_t)q * D + k];
        }
        double u = 0.0;
#pragma unroll
        for (int k = 0; k < D; k++) u += fw[e * D + k] * x[k];
        if (!bad) ev::neu(s, c, u);
    }
    ev::block_part<kT>(bad ? 0.0 : s, bad ? 0.0 : c, bad, 0, 0, 0, part);
}

// ---- u <- the weights --------------------------------------------------------------------------------------------------------------
// entries e0 .. e0 + n of the chunk's functionals k0 .. k0 + Kc
template <int D>
__global__ __launch_bounds__(kT) void k_fn_scatter(int64_t n, int64_t e0, int k0, int Kc, const int32_t *__restrict__ fvar, const int32_t *__restrict__ ffun,
                                                   const double *__restrict__ fw, const uint8_t *__restrict__ vinfo, const int32_t *__restrict__ var_pos,
                                                   double *__restrict__ U) {
    const int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (t >= n) return;
    const int64_t e = e0 + t;
    const int32_t v = fvar[e];
    if (vinfo[v] & kClamped) return;      // (an observed variable: the mean only)
    double *u = U + ((int64_t)var_pos[v] * Kc + (ffun[e] - k0)) * D;
#pragma unroll
    for (int k = 0; k < D; k++) u[k] = fw[e * D + k];
}

// ---- u_q += Σ G_c' u_c over the light paths on q, in path order ------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(kT) void k_fn_inject(int64_t q0, int64_t n, int Kc, const int32_t *__restrict__ att_off, const int32_t *__restrict__ att_head,
                                                  const double *__restrict__ link, double *__restrict__ U) {
    const int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x;
    const int64_t j = t / Kc;
    const int k = (int)(t - j * Kc);
    if (j >= n) return;
    const int64_t q = q0 + j;
    const int32_t b = att_off[q], e = att_off[q + 1];
    if (b == e) return;
    double u[D];
#pragma unroll
    for (int i = 0; i < D; i++) u[i] = U[(q * Kc + k) * D + i];
    for (int32_t a = b; a < e; a++) {
        const int64_t c = att_head[a];
        double tc[D], r[D];
#pragma unroll
        for (int i = 0; i < D; i++) tc[i] = U[(c * Kc + k) * D + i];
        gt_mul<D>(link + c * LR<D>::N + LR<D>::G, tc, r);
#pragma unroll
        for (int i = 0; i < D; i++) u[i] += r[i];
    }
#pragma unroll
    for (int i = 0; i < D; i++) U[(q * Kc + k) * D + i] = u[i];
}

// ---- the blocked scan, tail to head ------------------------------------------------------------------------------------------------
// s_i = G_i'(u_i + s_{i+1}) is what position i hands to the one before it.  A tile [a, b) maps s_b to s_a = o + P' s_b with
// P = G_{b-1} .. G_a, the sampler's tile matrix.  Buffers as the sampler's: Gc [item][D*D], oc and carry [item][Kc][D].
template <int D, bool POS>
__global__ __launch_bounds__(kT) void k_fn_compose(int64_t n, int Kc, const int2 *__restrict__ rng, const double *__restrict__ link,
                                                   const double *__restrict__ U, const double *__restrict__ Gb, const double *__restrict__ ob,
                                                   double *__restrict__ Gc, double *__restrict__ oc) {
    const int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x;
    const int64_t j = t / (Kc + 1);
    const int k = (int)(t - j * (Kc + 1));
    if (j >= n) return;
    const int2 r = rng[j];
    if (k == Kc) {
        // the product of the items' G, last one leftmost (k_sp_compose's): shared by all functionals
        double P[D][D];
#pragma unroll
        for (int a = 0; a < D; a++)
#pragma unroll
            for (int b = 0; b < D; b++) P[a][b] = a == b ? 1.0 : 0.0;
        for (int32_t i = r.x; i < r.y; i++) {
            const double *g = POS ? link + (int64_t)i * LR<D>::N + LR<D>::G : Gb + (int64_t)i * D * D;
            double N[D][D];
#pragma unroll
            for (int a = 0; a < D; a++)
#pragma unroll
                for (int b = 0; b < D; b++) {
                    double u = 0.0;
#pragma unroll
                    for (int m = 0; m < D; m++) u += g[a * D + m] * P[m][b];
                    N[a][b] = u;
                }
#pragma unroll
            for (int a = 0; a < D; a++)
#pragma unroll
                for (int b = 0; b < D; b++) P[a][b] = N[a][b];
        }
#pragma unroll
        for (int a = 0; a < D; a++)
#pragma unroll
            for (int b = 0; b < D; b++) Gc[j * D * D + a * D + b] = P[a][b];
        return;
    }
    double s[D];
#pragma unroll
    for (int i = 0; i < D; i++) s[i] = 0.0;
    for (int32_t i = r.y - 1; i >= r.x; i--) {
        double ns[D];
        if constexpr (POS) {
            double tt[D];
#pragma unroll
            for (int a = 0; a < D; a++) tt[a] = U[((int64_t)i * Kc + k) * D + a] + s[a];
            gt_mul<D>(link + (int64_t)i * LR<D>::N + LR<D>::G, tt, ns);
        } else {
            gt_mul<D>(Gb + (int64_t)i * D * D, s, ns);
#pragma unroll
            for (int a = 0; a < D; a++) ns[a] += ob[((int64_t)i * Kc + k) * D + a];
        }
#pragma unroll
        for (int a = 0; a < D; a++) s[a] = ns[a];
    }
#pragma unroll
    for (int a = 0; a < D; a++) oc[(j * Kc + k) * D + a] = s[a];
}

// TOP: item j is a path, top[j].xy the range of its top-level items, the carry in at its tail is zero; otherwise the carry of item j of
// this level.  POS: the children are positions (u_q becomes the pull of q's whole subtree), else items of the level below (their carries
// written to cb).
template <int D, bool POS, bool TOP>
__global__ __launch_bounds__(kT) void k_fn_walk(int64_t n, int Kc, const int4 *__restrict__ top, const int2 *__restrict__ rng, const double *__restrict__ carry,
                                                const double *__restrict__ link, const double *__restrict__ Gb, const double *__restrict__ ob,
                                                double *__restrict__ cb, double *__restrict__ U) {
    const int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x;
    const int64_t j = t / Kc;
    const int k = (int)(t - j * Kc);
    if (j >= n) return;
    double s[D];
    int32_t b, e;
    if constexpr (TOP) {
        const int4 p = top[j];
        b = p.x; e = p.y;
#pragma unroll
        for (int a = 0; a < D; a++) s[a] = 0.0;
    } else {
        const int2 r = rng[j];
        b = r.x; e = r.y;
#pragma unroll
        for (int a = 0; a < D; a++) s[a] = carry[(j * Kc + k) * D + a];
    }
    for (int32_t i = e - 1; i >= b; i--) {
        double ns[D];
        if constexpr (POS) {
            double tt[D];
            double *u = U + ((int64_t)i * Kc + k) * D;
#pragma unroll
            for (int a = 0; a < D; a++) { tt[a] = u[a] + s[a]; u[a] = tt[a]; }
            gt_mul<D>(link + (int64_t)i * LR<D>::N + LR<D>::G, tt, ns);
        } else {
#pragma unroll
            for (int a = 0; a < D; a++) cb[((int64_t)i * Kc + k) * D + a] = s[a];
            gt_mul<D>(Gb + (int64_t)i * D * D, s, ns);
#pragma unroll
            for (int a = 0; a < D; a++) ns[a] += ob[((int64_t)i * Kc + k) * D + a];
        }
#pragma unroll
        for (int a = 0; a < D; a++) s[a] = ns[a];
    }
}

// ---- the noise coordinates: g_q = M_q' u_q + Σ X_x' u_q' (the extra blocks that read q's ε), zero in a failed component -----------
template <int D>
__global__ __launch_bounds__(kT) void k_fn_noise(int64_t npos, int k0, int Kc, int K, const double *__restrict__ link, const int32_t *__restrict__ xt_off,
                                                 const int2 *__restrict__ xt_ent, const double *__restrict__ xblk, const int32_t *__restrict__ comp,
                                                 const uint8_t *__restrict__ cflag, const double *__restrict__ U, double *__restrict__ G) {
    const int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x;
    const int64_t q = t / Kc;
    const int k = (int)(t - q * Kc);
    if (q >= npos) return;
    double g[D];
#pragma unroll
    for (int j = 0; j < D; j++) g[j] = 0.0;
    if (!cflag[comp[q]]) {
        const double *m = link + q * LR<D>::N + LR<D>::M, *u = U + (q * Kc + k) * D;
#pragma unroll
        for (int j = 0; j < D; j++)
#pragma unroll
            for (int i = 0; i <= j; i++) g[j] += m[i * D + j] * u[i];
        if (xt_off) {
            for (int32_t a = xt_off[q]; a < xt_off[q + 1]; a++) {
                const int2 en = xt_ent[a];
                const double *b = xblk + (int64_t)en.y * D * D, *us = U + ((int64_t)en.x * Kc + k) * D;
#pragma unroll
                for (int j = 0; j < D; j++)
#pragma unroll
                    for (int i = 0; i < D; i++) g[j] += b[i * D + j] * us[i];
            }
        }
    }
    double *o = G + (q * K + k0 + k) * D;
#pragma unroll
    for (int j = 0; j < D; j++) o[j] = g[j];
}

// ---- cov[k][l] = Σ_q g_q^k · g_q^l ---------------------------------------------------------------------------------------------------
// block = (a block of kCovPos positions, a tile (ti, tj <= ti) of the lower triangle), the tile fastest; thread (a, b) = pair (16 ti + a, 16 tj + b)
template <int D>
__global__ __launch_bounds__(kCovTile * kCovTile) void k_fn_cov(int64_t npos, int K, int ntile, const double *__restrict__ G, double2 *__restrict__ part) {
    const int64_t blk = blockIdx.x / ntile;
    int ti = 0, rest = (int)(blockIdx.x - blk * ntile);
    while (rest > ti) { rest -= ti + 1; ti++; }
    const int k = ti * kCovTile + (int)threadIdx.x / kCovTile, l = rest * kCovTile + (int)threadIdx.x % kCovTile;
    if (k >= K || l > k) return;
    const int64_t q0 = blk * kCovPos, q1 = q0 + kCovPos < npos ? q0 + kCovPos : npos;
    double s = 0.0, c = 0.0;
    for (int64_t q = q0; q < q1; q++) {
        const double *gk = G + (q * K + k) * D, *gl = G + (q * K + l) * D;
        double u = 0.0;
#pragma unroll
        for (int j = 0; j < D; j++) u += gk[j] * gl[j];
        ev::neu(s, c, u);
    }
    part[(blk * K + k) * K + l] = make_double2(s, c);
}

__global__ __launch_bounds__(kT) void k_fn_cov_final(int64_t nblk, int K, const double2 *__restrict__ part, const ev::Part *__restrict__ fpart,
                                                     double *__restrict__ cov) {
    const int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (t >= (int64_t)K * K) return;
    const int k = (int)(t / K), l = (int)(t - (int64_t)k * K);
    if (l > k) return;
    double s = 0.0, c = 0.0;
    for (int64_t b = 0; b < nblk; b++) {
        const double2 p = part[(b * K + k) * K + l];
        ev::neu(s, c, p.x);
        c += p.y;
    }
    const double v = fpart[k].n[0] || fpart[l].n[0] ? __builtin_nan("") : s + c;
    cov[(int64_t)k * K + l] = v;
    cov[(int64_t)l * K + k] = v;
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
using sp::blocks;

template <int D>
void launch_adjoint(cx_handle *h, sp::Plan &P, int k0, int Kc, int K, int64_t e0, int64_t ne) {
    const int64_t nu = P.npos * Kc * D;
    (void)hipMemsetAsync(P.d_Z, 0, (size_t)nu * sizeof(double), h->stream);
    if (ne)
        hipLaunchKernelGGL(k_fn_scatter<D>, dim3(blocks(ne, kT)), dim3(kT), 0, h->stream, ne, e0, k0, Kc, P.d_fvar, P.d_ffun, P.d_fw, h->d_vinfo, P.d_var_pos,
                           P.d_Z);
    for (size_t di = P.depths.size(); di-- > 0;) {
        const sp::Depth &dp = P.depths[di];
        if (dp.n_att)
            hipLaunchKernelGGL(k_fn_inject<D>, dim3(blocks((dp.pos_end - dp.pos_beg) * Kc, kT)), dim3(kT), 0, h->stream, dp.pos_beg, dp.pos_end - dp.pos_beg, Kc,
                               P.d_att_off, P.d_att_head, P.d_link, P.d_Z);
        for (int l = 1; l <= dp.levels; l++) {
            const int64_t n = dp.n_items[(size_t)l - 1];
            const int2 *rng = P.d_rng + dp.rng_off[(size_t)l - 1];
            if (l == 1)
                hipLaunchKernelGGL((k_fn_compose<D, true>), dim3(blocks(n * (Kc + 1), kT)), dim3(kT), 0, h->stream, n, Kc, rng, P.d_link, P.d_Z, nullptr, nullptr,
                                   P.d_Gc[1], P.d_oc[1]);
            else
                hipLaunchKernelGGL((k_fn_compose<D, false>), dim3(blocks(n * (Kc + 1), kT)), dim3(kT), 0, h->stream, n, Kc, rng, P.d_link, P.d_Z,
                                   P.d_Gc[(size_t)l - 1], P.d_oc[(size_t)l - 1], P.d_Gc[(size_t)l], P.d_oc[(size_t)l]);
        }
        const int4 *top = P.d_top + dp.top_off;
        const int L = dp.levels;
        if (L == 0)
            hipLaunchKernelGGL((k_fn_walk<D, true, true>), dim3(blocks(dp.n_paths * Kc, kT)), dim3(kT), 0, h->stream, dp.n_paths, Kc, top, nullptr, nullptr, P.d_link,
                               nullptr, nullptr, nullptr, P.d_Z);
        else
            hipLaunchKernelGGL((k_fn_walk<D, false, true>), dim3(blocks(dp.n_paths * Kc, kT)), dim3(kT), 0, h->stream, dp.n_paths, Kc, top, nullptr, nullptr, P.d_link,
                               P.d_Gc[(size_t)L], P.d_oc[(size_t)L], P.d_carry[(size_t)L], P.d_Z);
        for (int l = L; l >= 1; l--) {
            const int64_t n = dp.n_items[(size_t)l - 1];
            const int2 *rng = P.d_rng + dp.rng_off[(size_t)l - 1];
            if (l == 1)
                hipLaunchKernelGGL((k_fn_walk<D, true, false>), dim3(blocks(n * Kc, kT)), dim3(kT), 0, h->stream, n, Kc, nullptr, rng, P.d_carry[1], P.d_link, nullptr,
                                   nullptr, nullptr, P.d_Z);
            else
                hipLaunchKernelGGL((k_fn_walk<D, false, false>), dim3(blocks(n * Kc, kT)), dim3(kT), 0, h->stream, n, Kc, nullptr, rng, P.d_carry[(size_t)l], P.d_link,
                                   P.d_Gc[(size_t)l - 1], P.d_oc[(size_t)l - 1], P.d_carry[(size_t)l - 1], P.d_Z);
        }
    }
    hipLaunchKernelGGL(k_fn_noise<D>, dim3(blocks(P.npos * Kc, kT)), dim3(kT), 0, h->stream, P.npos, k0, Kc, K, P.d_link, P.n_klink ? P.d_xt_off.get() : nullptr,
                       P.d_xt_ent, P.d_xblk, P.d_comp, P.d_cflag, P.d_Z, P.d_fg);
}

template <int D>
void launch_mean(cx_handle *h, const ev::Cache &E, sp::Plan &P, int K) {
    // z⁰: the sampler's scan with one sample whose ε is zero
    const sp::Gen g{P.d_noise, h->nv * D, 0, 0};
    sp::launch_cond<D>(h, E, P);
    sp::launch_samples<D>(h, P, 1, g);
    hipLaunchKernelGGL(k_fn_mean<D>, dim3((unsigned)K), dim3(kT), 0, h->stream, P.d_foff, P.d_fvar, P.d_fw, h->d_vinfo, P.d_dslot, P.d_var_pos, P.d_comp, P.d_cflag,
                       ev::v2f_of(h), E.d_W, P.d_Z, P.d_fpart);
}

template <int D>
void launch_cov(cx_handle *h, sp::Plan &P, int K, int64_t nblk) {
    const int nt = (K + kCovTile - 1) / kCovTile;
    const int ntile = nt * (nt + 1) / 2;
    hipLaunchKernelGGL(k_fn_cov<D>, dim3((unsigned)(nblk * ntile)), dim3(kCovTile * kCovTile), 0, h->stream, P.npos, K, ntile, P.d_fg, P.d_fcpart);
    hipLaunchKernelGGL(k_fn_cov_final, dim3(blocks((int64_t)K * K, kT)), dim3(kT), 0, h->stream, nblk, K, P.d_fcpart, P.d_fpart, P.d_fcov);
}

}  // namespace fn
}  // namespace cx

using namespace cxh;

extern "C" int32_t cx_linear_moments(cx_handle *h, int64_t n_functionals, const int64_t *offsets, const int64_t *variable_ids, const double *weights,
                                     double *mean, double *cov, int64_t *counts4) {
    const std::string who = "cx_linear_moments";
    try {
        cx::ev::Cache *Ep = nullptr;
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
        if ((rc = cx::ev::prepare(h, who, bad, Ep)) != CX_OK) return rc;
        CX_REQUIRE(h, !h->offsets_nonzero, CX_ERR_UNSUPPORTED, who + ": the handle has non-zero factor offsets (cx_set_factor_offsets), which this call does not implement");
        cx::ev::Cache &E = *Ep;
        cx::sp::Plan *Pp = nullptr;
        if ((rc = cx::sp::plan_of(h, E, who, Pp)) != CX_OK) return rc;
        cx::sp::Plan &P = *Pp;
        const int d = h->cfg.dim;
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
        int64_t und = 0, npd = 0, n_nan = 0;
        if (K > 0) {
            // chunks of functionals: u and the level buffers under 2^27 doubles.  CX_FN_CHUNK (tests, A/B) caps a chunk: a call of more
            // functionals than that runs in several, which must not change a bit of the result
            int64_t per = P.npos;
            for (size_t l = 1; l < P.level_cap.size(); l++) per += 2 * P.level_cap[l];
            per = std::max<int64_t>(per * d, 1);
            int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(K, ((int64_t)1 << 27) / per));
            if (const char *e = std::getenv("CX_FN_CHUNK")) chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, std::atoll(e)));
            if (cov && K * P.npos * d > cx::fn::kMaxG)
                return fail(h, CX_ERR_OUT_OF_MEMORY, who + ": the noise coordinates of " + std::to_string(K) + " functionals over " + std::to_string(P.npos) +
                                                         " variables pass 2^30 doubles: ask for fewer functionals per call");
            const int64_t nblk = (P.npos + cx::fn::kCovPos - 1) / cx::fn::kCovPos;
            if (cov && nblk * K * K > cx::fn::kMaxPart)
                return fail(h, CX_ERR_OUT_OF_MEMORY, who + ": the block partials of a " + std::to_string(K) + " x " + std::to_string(K) + " covariance over " +
                                                         std::to_string(P.npos) + " variables pass 2^28 pairs: ask for fewer functionals per call");
            if ((rc = cx::sp::ensure_chunk(h, P, cov ? chunk : 1, 0, false)) != CX_OK) return rc;
            if ((rc = P.d_noise.ensure(h, h->nv * d)) != CX_OK) return rc;
            if ((rc = P.d_foff.upload(h, foff)) != CX_OK || (rc = P.d_fvar.upload(h, fvar)) != CX_OK || (rc = P.d_ffun.upload(h, ffun)) != CX_OK ||
                (rc = P.d_fw.upload(h, fw)) != CX_OK || (rc = P.d_fpart.ensure(h, K)) != CX_OK) return rc;
            if (cov && ((rc = P.d_fg.ensure(h, std::max<int64_t>(K * P.npos * d, 1))) != CX_OK || (rc = P.d_fcov.ensure(h, K * K)) != CX_OK ||
                        (rc = P.d_fcpart.ensure(h, std::max<int64_t>(nblk, 1) * K * K)) != CX_OK)) return rc;
            CX_HIP(h, hipMemsetAsync(P.d_noise, 0, (size_t)(h->nv * d) * sizeof(double), h->stream));
            CX_HIP(h, hipStreamSynchronize(h->stream));
            cx::ev::var_pass(h, E);
            cx::ev::with_dim(d, [&](auto D) { cx::fn::launch_mean<D()>(h, E, P, (int)K); });
            CX_HIP(h, hipGetLastError());
            if (cov) {
                for (int64_t k0 = 0; k0 < K; k0 += chunk) {
                    const int Kc = (int)std::min<int64_t>(chunk, K - k0);
                    const int64_t e0 = foff[(size_t)k0], ne = foff[(size_t)(k0 + Kc)] - e0;
                    cx::ev::with_dim(d, [&](auto D) { cx::fn::launch_adjoint<D()>(h, P, (int)k0, Kc, (int)K, e0, ne); });
                    CX_HIP(h, hipGetLastError());
                }
                cx::ev::with_dim(d, [&](auto D) { cx::fn::launch_cov<D()>(h, P, (int)K, nblk); });
                CX_HIP(h, hipGetLastError());
                CX_HIP(h, hipMemcpyAsync(cov, P.d_fcov, (size_t)(K * K) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            }
            std::vector<cx::ev::Part> part((size_t)K);
            CX_HIP(h, hipMemcpyAsync(part.data(), P.d_fpart, (size_t)K * sizeof(cx::ev::Part), hipMemcpyDeviceToHost, h->stream));
            CX_HIP(h, hipStreamSynchronize(h->stream));      // (the host vectors die here)
            for (int64_t k = 0; k < K; k++) {
                const bool failed = part[(size_t)k].n[0] != 0;
                n_nan += failed;
                mean[k] = failed ? std::nan("") : part[(size_t)k].s + part[(size_t)k].c;
            }
        } else {
            // no functional: the status alone
            cx::ev::var_pass(h, E);
            cx::ev::with_dim(d, [&](auto D) { cx::sp::launch_cond<D()>(h, E, P); });
            CX_HIP(h, hipGetLastError());
        }
        if (P.n_comp) CX_HIP(h, hipMemcpy(P.h_cflag.data(), P.d_cflag, (size_t)P.n_comp, hipMemcpyDeviceToHost));
        for (uint8_t c : P.h_cflag) { und += (c & 1) != 0; npd += (c & 1) == 0 && (c & 2) != 0; }
        counts4[0] = P.n_comp;
        counts4[1] = und + npd;
        counts4[2] = n_nan;
        counts4[3] = P.npos;
        return CX_OK;
    } catch (const std::bad_alloc &) { return fail(h, CX_ERR_OUT_OF_MEMORY, who + ": host allocation failed"); }
}
