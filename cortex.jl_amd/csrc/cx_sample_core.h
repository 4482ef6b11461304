// cx_sample_core.h — what cx_sample_posterior (cx_sample.hip) and cx_linear_moments (cx_functional.hip) share: the forest plan (heavy
// paths by light depth, positions, tiles), the links of every position (k_sp_cond, k_sp_cond_kary), the status pass (k_sp_flag) and the
// forward blocked scan (k_sp_compose, k_sp_walk).  One plan per handle (cx_handle::sample), whichever entry builds it first.  The
// derivation is DESIGN.md §4g; the adjoint of the scan is §4i.  The forest part of the plan (build_forest) and the status pass also serve
// cx_sample_posterior_mfma (cx_sample_mfma.hip, §4r), which has its own links and scan on the matrix cores.
#pragma once
#include "cx_evidence_core.h"
#include "cx_tree_plan.h"

namespace cx {
namespace sp {

using ev::Lay;

constexpr int kT = 256;        // threads per block of the scan, gather and pairwise passes
constexpr int kKT = 16;        // threads per block of the k-ary pass: each thread's joint lives in LDS
constexpr int kTile = 64;      // items per tile of the blocked scan
constexpr double kTwoPi = 6.28318530717958647693;

template <int D>
struct LR {
    static constexpr int G = 0, OFF = D * D, M = D * D + D, N = 2 * D * D + D;      // a link: G (D x D) | off (D) | L⁻ᵀ (D x D, upper)
};

// ---- the generator: Philox4x32-10 (Salmon et al., SC'11), Box–Muller over two 53-bit uniforms in (0, 1) ------------------------
__host__ __device__ __forceinline__ uint4 philox(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c.x, p1 = (uint64_t)0xCD9E8D57u * c.z;
        c = make_uint4((uint32_t)(p1 >> 32) ^ c.y ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k1, (uint32_t)p0);
    }
    return c;
}

// components 2j and 2j + 1 of variable v in sample s: counter (j, v, s lo, s hi), key (seed lo, seed hi)
__device__ __forceinline__ void normal_pair(uint64_t seed, uint64_t s, uint32_t v, uint32_t j, double &n0, double &n1) {
    const uint4 x = philox(make_uint4(j, v, (uint32_t)s, (uint32_t)(s >> 32)), (uint32_t)seed, (uint32_t)(seed >> 32));
    const double u1 = ((double)((((uint64_t)x.y << 32) | x.x) >> 11) + 0.5) * 0x1p-53;
    const double u2 = ((double)((((uint64_t)x.w << 32) | x.z) >> 11) + 0.5) * 0x1p-53;
    const double r = sqrt(-2.0 * log(u1));
    double sn, cs;
    sincos(kTwoPi * u2, &sn, &cs);
    n0 = r * cs; n1 = r * sn;
}

struct Gen {
    const double *noise;       // caller's ε of this chunk of samples, [S_chunk][nv][D]; null: Philox
    int64_t nvd;               // nv * D
    uint64_t seed;
    int64_t s0;                // global index of the chunk's first sample
};

template <int D>
__device__ __forceinline__ void eps_of(const Gen &g, int64_t sl, int32_t v, double (&e)[D]) {
    if (g.noise) {
        const double *p = g.noise + sl * g.nvd + (int64_t)v * D;
#pragma unroll
        for (int k = 0; k < D; k++) e[k] = p[k];
    } else {
#pragma unroll
        for (int j = 0; j < (D + 1) / 2; j++) {
            double a, b;
            normal_pair(g.seed, (uint64_t)(g.s0 + sl), (uint32_t)v, (uint32_t)j, a, b);
            e[2 * j] = a;
            if (2 * j + 1 < D) e[2 * j + 1] = b;
        }
    }
}

// z <- G z + off + L⁻ᵀ ε_v (+ the extra blocks of a k-ary child: its later siblings' ε)
template <int D>
__device__ __forceinline__ void link_step(const double *__restrict__ link, int64_t q, const int32_t *__restrict__ pos_var, const int32_t *__restrict__ xoff,
                                          const int32_t *__restrict__ xvar, const double *__restrict__ xblk, const Gen &g, int64_t sl, double (&z)[D]) {
    const double *l = link + q * LR<D>::N;
    double e[D], n[D];
    eps_of<D>(g, sl, pos_var[q], e);
#pragma unroll
    for (int i = 0; i < D; i++) {
        double t = l[LR<D>::OFF + i];
#pragma unroll
        for (int j = 0; j < D; j++) t += l[LR<D>::G + i * D + j] * z[j];
#pragma unroll
        for (int j = i; j < D; j++) t += l[LR<D>::M + i * D + j] * e[j];
        n[i] = t;
    }
    if (xoff) {
        for (int32_t x = xoff[q]; x < xoff[q + 1]; x++) {
            double f[D];
            eps_of<D>(g, sl, xvar[x], f);
            const double *b = xblk + (int64_t)x * D * D;
#pragma unroll
            for (int i = 0; i < D; i++)
#pragma unroll
                for (int j = 0; j < D; j++) n[i] += b[i * D + j] * f[j];
        }
    }
#pragma unroll
    for (int i = 0; i < D; i++) z[i] = n[i];
}

template <int D>
__device__ __forceinline__ void put_link(double *__restrict__ link, int64_t q, const double (&G)[D][D], const double (&off)[D], const double (&M)[D][D]) {
    double *l = link + q * LR<D>::N;
#pragma unroll
    for (int i = 0; i < D; i++) {
        l[LR<D>::OFF + i] = off[i];
#pragma unroll
        for (int j = 0; j < D; j++) { l[LR<D>::G + i * D + j] = G[i][j]; l[LR<D>::M + i * D + j] = j >= i ? M[i][j] : 0.0; }
    }
}

// ---- conditional pass: roots and two-variable links, one thread each -------------------------------------------------------------
// roots[k] = the position of a root; plink[k] = (pair row of cx_evidence.hip's table, child is the row's OUT end, child position, -)
// st[q] = 0 ok, 1 an undefined input, 2 not positive definite
template <int D>
__global__ __launch_bounds__(kT) void k_sp_cond(int64_t n_root, int64_t n_link, const int32_t *__restrict__ roots, const int4 *__restrict__ plink,
                                                const int32_t *__restrict__ pos_var, ev::PairTab tab, ev::Msgs msg, double *__restrict__ link,
                                                uint8_t *__restrict__ st) {
    constexpr int K = Lay<D>::K;
    const int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (t >= n_root + n_link) return;
    double G[D][D], off[D], L[D][D], M[D][D];
#pragma unroll
    for (int i = 0; i < D; i++) {
        off[i] = 0.0;
#pragma unroll
        for (int j = 0; j < D; j++) G[i][j] = 0.0;
    }
    int status = 0;
    int64_t q;
    if (t < n_root) {
        // the root's belief: precision Λ_r (the sum of its stored messages), centre μ_r; z_r = L_r⁻ᵀ ε
        q = roots[t];
        const double *w = msg.W + (int64_t)pos_var[q] * K;
        bool undef = false;
#pragma unroll
        for (int i = 0; i < D; i++) undef = undef || __builtin_isnan(w[i]);
#pragma unroll
        for (int i = 0; i < D; i++)
#pragma unroll
            for (int j = 0; j < D; j++) {
                L[i][j] = i >= j ? w[D + tri<D>(j, i)] : 0.0;
                undef = undef || __builtin_isnan(L[i][j]);
            }
        if (undef) status = 1;
        else if (!ev::chol<D>(L)) status = 2;
    } else {
        const int4 lk = plink[t - n_root];
        q = lk.z;
        // the factor belief, centred, over (out, in).  Both ends are free: the plan makes a link only between two free variables and
        // is rebuilt when the observed flags change
        ev::PairJoint<D> B;
        ev::pair_joint<D>(lk.x, tab, msg, B);
        // the child's block C and the parent's block p (selects, not a runtime offset: the arrays stay in registers)
        const bool child_out = lk.y != 0;
        double hc[D], Jcp[D][D];
#pragma unroll
        for (int i = 0; i < D; i++) {
            hc[i] = child_out ? B.h[i] : B.h[D + i];
#pragma unroll
            for (int j = 0; j < D; j++) {
                L[i][j] = child_out ? B.J[i][j] : B.J[D + i][D + j];
                Jcp[i][j] = child_out ? B.J[i][D + j] : B.J[D + i][j];
            }
        }
        if (!B.ok) status = 1;
        else if (!ev::chol<D>(L)) status = 2;
        else {
            ev::chol_solve<D>(L, hc, off);
#pragma unroll
            for (int k = 0; k < D; k++) {
                double b[D], x[D];
#pragma unroll
                for (int i = 0; i < D; i++) b[i] = -Jcp[i][k];
                ev::chol_solve<D>(L, b, x);
#pragma unroll
                for (int i = 0; i < D; i++) G[i][k] = x[i];
            }
        }
    }
    if (status == 0) ev::inv_t<D>(L, M);
    else {
#pragma unroll
        for (int i = 0; i < D; i++)
#pragma unroll
            for (int j = 0; j < D; j++) M[i][j] = 0.0;
    }
    put_link<D>(link, q, G, off, M);
    st[q] = (uint8_t)status;
}

// ---- conditional pass: factors of 3 .. 7 variables -------------------------------------------------------------------------------
// klink[k] = kary row | parent entry | child position per entry (-1: not a child), 10 int32.  The joint over the free entries is
// k_ev_kary's (cx_evidence.hip), packed in LDS; J_CC is factored in place through an index map that skips the parent's block.
template <int D>
__global__ __launch_bounds__(kKT) void k_sp_cond_kary(int64_t n, const int32_t *__restrict__ klink, ev::KaryTab tab, ev::Msgs msg,
                                                      const int32_t *__restrict__ xoff, double *__restrict__ link, double *__restrict__ xblk,
                                                      uint8_t *__restrict__ st) {
    constexpr int NP = ev::KLay<D>::NP, NM = ev::KLay<D>::NM;
    __shared__ double sJ[NP * kKT], sh[NM * kKT], sy[NM * kKT];
    __shared__ int32_t sp[7 * kKT];
    const int t = threadIdx.x;
    double *J = sJ + t, *hv = sh + t, *yv = sy + t;      // element k at [k * kKT]
    int32_t *pos = sp + t;                                 // the child positions, child b at [b * kKT]
    const int64_t f = (int64_t)blockIdx.x * kKT + t;
    if (f >= n) return;
    const int32_t *kl = klink + f * 10, *cpos = kl + 2;
    const int32_t row = kl[0], ep = kl[1];
    double Qi[D][D], ldq, bp[D], g[D], cq;
    unsigned freemask;
    int nfree;
    bool ok;
    ev::kary_joint<D, kKT>(row, tab, msg, J, hv, Qi, ldq, bp, g, cq, freemask, nfree, ok);
    const int fpo = __builtin_popcount(freemask & ((1u << ep) - 1u));      // the parent's ordinal among the free entries
    // the child space: joint index of child index r (the parent's block is skipped)
    const int m = (nfree - 1) * D;
    auto mapi = [&](int r) { return r / D < fpo ? r : r + D; };
    auto JC = [&](int r, int c) -> double & { return J[ev::pk(mapi(r), mapi(c)) * kKT]; };      // r >= c
    auto y = [&](int i) -> double & { return yv[i * kKT]; };
    const int status = !ok ? 1 : ev::chol_at(m, JC) ? 0 : 2;
    // the child positions, in child order
    int nc = 0;
    for (int e = 0; e < 8; e++)
        if (((freemask >> e) & 1) && e != ep) pos[(nc++) * kKT] = cpos[e];
    const double nan = __builtin_nan("");
    for (int b = 0; b < nc; b++) {
        double *l = link + (int64_t)pos[b * kKT] * LR<D>::N;
        for (int k = 0; k < LR<D>::N; k++) l[k] = status ? nan : 0.0;
        st[pos[b * kKT]] = (uint8_t)status;
    }
    if (status) return;
    // off = J_CC⁻¹ h_C
    for (int i = 0; i < m; i++) yv[i * kKT] = hv[mapi(i) * kKT];
    ev::chol_solve_at(m, JC, y);
    for (int i = 0; i < m; i++) link[(int64_t)pos[(i / D) * kKT] * LR<D>::N + LR<D>::OFF + i % D] = yv[i * kKT];
    // G = -J_CC⁻¹ J_Cp, column by column
    for (int k = 0; k < D; k++) {
        const int pj = fpo * D + k;
        for (int i = 0; i < m; i++) {
            const int a = mapi(i);
            yv[i * kKT] = -(a >= pj ? J[ev::pk(a, pj) * kKT] : J[ev::pk(pj, a) * kKT]);
        }
        ev::chol_solve_at(m, JC, y);
        for (int i = 0; i < m; i++) link[(int64_t)pos[(i / D) * kKT] * LR<D>::N + LR<D>::G + (i % D) * D + k] = yv[i * kKT];
    }
    // L⁻ᵀ row by row: row r = column r of L⁻¹; entry (r, c) goes to the own block (c / D == r / D) or to sibling c / D's extra block
    for (int r = 0; r < m; r++) {
        for (int c = r; c < m; c++) {
            double u = c == r ? 1.0 : 0.0;
            for (int k = r; k < c; k++) u -= JC(c, k) * yv[k * kKT];
            yv[c * kKT] = u / JC(c, c);
            const int bi = r / D, bj = c / D;
            if (bj == bi) link[(int64_t)pos[bi * kKT] * LR<D>::N + LR<D>::M + (r % D) * D + c % D] = yv[c * kKT];
            else xblk[((int64_t)xoff[pos[bi * kKT]] + (bj - bi - 1)) * D * D + (r % D) * D + c % D] = yv[c * kKT];
        }
    }
}

// ---- the status of every component: one block per chunk of at most kFlagChunk of its positions (cpos[cbeg[k] .. cbeg[k + 1])), then one
// thread per component over its chunks (ccb[c] .. ccb[c + 1])
constexpr int kFlagChunk = 8192;

static __global__ __launch_bounds__(kT) void k_sp_flag(const int32_t *__restrict__ cbeg, const int32_t *__restrict__ cpos, const uint8_t *__restrict__ st,
                                                uint8_t *__restrict__ cpart) {
    __shared__ unsigned sm[kT];
    const int t = threadIdx.x;
    unsigned m = 0;
    for (int32_t k = cbeg[blockIdx.x] + t; k < cbeg[blockIdx.x + 1]; k += kT) m |= st[cpos[k]];
    sm[t] = m;
    __syncthreads();
    for (int w = kT / 2; w > 0; w >>= 1) {
        if (t < w) sm[t] |= sm[t + w];
        __syncthreads();
    }
    if (t == 0) cpart[blockIdx.x] = (uint8_t)sm[0];
}

static __global__ __launch_bounds__(kT) void k_sp_flag_comp(int64_t n_comp, const int32_t *__restrict__ ccb, const uint8_t *__restrict__ cpart,
                                                     uint8_t *__restrict__ cflag) {
    const int64_t c = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (c >= n_comp) return;
    unsigned m = 0;
    for (int32_t k = ccb[c]; k < ccb[c + 1]; k++) m |= cpart[k];
    cflag[c] = (uint8_t)m;
}

// ---- the blocked scan ------------------------------------------------------------------------------------------------------------
// level-l buffers: Gc [item][D*D], oc and carry [item][S][D].  Items of level 1 are tiles of positions (links), of level l > 1 tiles of
// level l - 1 items; rng[j] = the range of item j's children.
template <int D, bool POS>
__global__ __launch_bounds__(kT) void k_sp_compose(int64_t n, int S, const int2 *__restrict__ rng, const double *__restrict__ link,
                                                   const int32_t *__restrict__ pos_var, const int32_t *__restrict__ xoff, const int32_t *__restrict__ xvar,
                                                   const double *__restrict__ xblk, Gen gen, const double *__restrict__ Gb, const double *__restrict__ ob,
                                                   double *__restrict__ Gc, double *__restrict__ oc) {
    const int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x;
    const int64_t j = t / (S + 1);
    const int s = (int)(t - j * (S + 1));
    if (j >= n) return;
    const int2 r = rng[j];
    if (s == S) {
        // the product of the items' G, last one leftmost: shared by all samples
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
                    for (int k = 0; k < D; k++) u += g[a * D + k] * P[k][b];
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
    double z[D];
#pragma unroll
    for (int k = 0; k < D; k++) z[k] = 0.0;
    for (int32_t i = r.x; i < r.y; i++) {
        if constexpr (POS) link_step<D>(link, i, pos_var, xoff, xvar, xblk, gen, s, z);
        else {
            const double *g = Gb + (int64_t)i * D * D, *o = ob + ((int64_t)i * S + s) * D;
            double nz[D];
#pragma unroll
            for (int a = 0; a < D; a++) {
                double u = o[a];
#pragma unroll
                for (int k = 0; k < D; k++) u += g[a * D + k] * z[k];
                nz[a] = u;
            }
#pragma unroll
            for (int a = 0; a < D; a++) z[a] = nz[a];
        }
    }
#pragma unroll
    for (int k = 0; k < D; k++) oc[(j * S + s) * D + k] = z[k];
}

// TOP: item j is a path, top[j] = (range of its top-level items, the position of its head's parent (-1: a root), -), the carry in is
// the parent's z; otherwise the carry of item j of this level.  POS: the children are positions (z written to Z), else items of the
// level below (their carries written to cb).
template <int D, bool POS, bool TOP>
__global__ __launch_bounds__(kT) void k_sp_walk(int64_t n, int S, const int4 *__restrict__ top, const int2 *__restrict__ rng, const double *__restrict__ carry,
                                                const double *__restrict__ link, const int32_t *__restrict__ pos_var, const int32_t *__restrict__ xoff,
                                                const int32_t *__restrict__ xvar, const double *__restrict__ xblk, Gen gen, const double *__restrict__ Gb,
                                                const double *__restrict__ ob, double *__restrict__ cb, double *__restrict__ Z) {
    const int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x;
    const int64_t j = t / S;
    const int s = (int)(t - j * S);
    if (j >= n) return;
    double z[D];
    int32_t b, e;
    if constexpr (TOP) {
        const int4 p = top[j];
        b = p.x; e = p.y;
#pragma unroll
        for (int k = 0; k < D; k++) z[k] = p.z >= 0 ? Z[((int64_t)p.z * S + s) * D + k] : 0.0;
    } else {
        const int2 r = rng[j];
        b = r.x; e = r.y;
#pragma unroll
        for (int k = 0; k < D; k++) z[k] = carry[(j * S + s) * D + k];
    }
    for (int32_t i = b; i < e; i++) {
        if constexpr (POS) {
            link_step<D>(link, i, pos_var, xoff, xvar, xblk, gen, s, z);
#pragma unroll
            for (int k = 0; k < D; k++) Z[((int64_t)i * S + s) * D + k] = z[k];
        } else {
            const double *g = Gb + (int64_t)i * D * D, *o = ob + ((int64_t)i * S + s) * D;
            double nz[D];
#pragma unroll
            for (int a = 0; a < D; a++) {
                cb[((int64_t)i * S + s) * D + a] = z[a];
                double u = o[a];
#pragma unroll
                for (int k = 0; k < D; k++) u += g[a * D + k] * z[k];
                nz[a] = u;
            }
#pragma unroll
            for (int a = 0; a < D; a++) z[a] = nz[a];
        }
    }
}

// ---- out[s][i] = c + z (the datum of an observed variable, NaN in a failed component) --------------------------------------------
template <int D>
__global__ __launch_bounds__(kT) void k_sp_gather(int64_t n, int S, const int32_t *__restrict__ vids, const uint8_t *__restrict__ vinfo,
                                                  const int32_t *__restrict__ dslot, const int32_t *__restrict__ var_pos, const int32_t *__restrict__ comp,
                                                  const uint8_t *__restrict__ cflag, const double *__restrict__ v2f, const double *__restrict__ W,
                                                  const double *__restrict__ Z, double *__restrict__ out) {
    constexpr int NT = Lay<D>::NT, K = Lay<D>::K;
    const int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (t >= n * S) return;
    const int64_t s = t / n, i = t - s * n;
    const int32_t v = vids ? vids[i] : (int32_t)i;
    double x[D];
    if (vinfo[v] & kClamped) ev::datum<D>(v2f, dslot[v], x);
    else {
        const int32_t q = var_pos[v];
        const bool bad = cflag[comp[q]] != 0;
        const double *w = W + (int64_t)v * K;
        const bool pd = D == 1 ? w[D] > 0.0 : w[D + NT] != 0.0;
#pragma unroll
        for (int k = 0; k < D; k++) x[k] = bad ? __builtin_nan("") : (pd ? w[k] : 0.0) + Z[((int64_t)q * S + s) * D + k];
    }
    double *o = out + t * D;
#pragma unroll
    for (int k = 0; k < D; k++) __builtin_nontemporal_store(x[k], o + k);
}

// ---- host: the plan ----------------------------------------------------------------------------------------------------------------
struct Depth {
    int64_t n_paths = 0;
    int levels = 0;                           // tile levels above the positions
    std::vector<int64_t> rng_off, n_items;    // per level 1 .. levels: offset into d_rng, items
    int64_t top_off = 0;                      // offset into d_top
    int64_t pos_beg = 0, pos_end = 0;         // the depth's positions (contiguous)
    int64_t n_att = 0;                        // paths of the next depth that attach to them
};

// the plan's device side; a rebuild starts from a default-constructed one
// The forest part of a plan — rooting, heavy paths by light depth, positions, tile levels, components and their chunks of the status
// pass, the slot of every datum — never looks at the dim or at the kind of a factor: cx_sample_posterior / cx_linear_moments (the plan
// below) and cx_sample_posterior_mfma (cx_sample_mfma.hip) build it with build_forest and keep it in these three parts
struct ForestDims {
    int64_t npos = 0, n_comp = 0, n_root = 0, n_chunk = 0;
    std::vector<Depth> depths;
    std::vector<int64_t> level_cap;           // per level (index 1 ..): the most items any depth has there
};
// the host side: the variable tree (parent variable, parent factor and component of every free variable; order: parents before
// children) and what goes to the device
struct Forest {
    std::vector<int32_t> order, vpar, vfac, vcomp, pos_var, var_pos, roots, pcomp, cpos, cbeg, ccb, dslot;
    std::vector<int4> top;
    std::vector<int2> rngs;
};
struct ForestDev {
    DevBuf<int32_t> d_pos_var, d_var_pos, d_comp, d_cpos, d_cbeg, d_dslot, d_roots;
    DevBuf<int32_t> d_ccb;                    // per component: its chunks of the status pass
    DevBuf<int4> d_top;
    DevBuf<int2> d_rng;
    DevBuf<uint8_t> d_st, d_cflag, d_cpart;
};

struct PlanDev : ForestDev {
    DevBuf<int32_t> d_klink, d_xoff, d_xvar;
    DevBuf<int4> d_plink;
    DevBuf<double> d_link, d_xblk;
    // the scan run leaf-to-root (cx_functional.hip): per position the heads of the light paths that hang on it (d_att_off, d_att_head)
    // and the extra blocks that read its ε, as (position of the earlier sibling, entry of d_xblk) (d_xt_off, d_xt_ent)
    DevBuf<int32_t> d_att_off, d_att_head, d_xt_off;
    DevBuf<int2> d_xt_ent;
    // per call, grown on demand: z, the level buffers, the caller's noise, the requested variables, the output
    DevBuf<double> d_Z, d_noise, d_out;
    std::vector<DevBuf<double>> d_Gc, d_oc, d_carry;      // per level
    DevBuf<int32_t> d_vid;
    // cx_linear_moments, per call: the functionals (offsets, entries, weights), the noise coordinates g of every functional, the
    // block partials of the means and of the covariance, the covariance
    DevBuf<int64_t> d_foff;
    DevBuf<int32_t> d_fvar, d_ffun;
    DevBuf<double> d_fw, d_fg, d_fcov;
    DevBuf<ev::Part> d_fpart;
    DevBuf<double2> d_fcpart;
};

struct Plan : PlanDev, ForestDims {
    bool valid = false;
    int64_t nv = -1, ne = -1;
    std::vector<uint8_t> vinfo;               // what the plan was built for (the observed flags)
    int64_t n_plink = 0, n_klink = 0, n_xent = 0;
    std::vector<uint8_t> h_cflag;
};

// the forest of the free variables of h, cut into tiles of `tile` items: P's dims and F
inline int32_t build_forest(cx_handle *h, ForestDims &P, Forest &F, const std::string &who, const int tile = kTile) {
    using namespace cxh;
    const int64_t nv = h->nv;
    treeplan::Rooted R;
    std::string err;
    int32_t rc = treeplan::root_forest(h, R, err, true);
    if (rc != CX_OK) {
        if (rc != CX_ERR_UNSUPPORTED) return fail(h, rc, who + ": " + err);
        // root_forest names the component ("... of variable <id>) ..."): the same variable, in this call's words
        std::string var = "?";
        const size_t at = err.find("variable ");
        if (at != std::string::npos) {
            const size_t b = at + 9, e = err.find_first_not_of("-0123456789", b);
            var = err.substr(b, e == std::string::npos ? std::string::npos : e - b);
        }
        return fail(h, CX_ERR_UNSUPPORTED, who + ": the non-observed variables form a cycle (through the component of variable " + var +
                                               "): no sampler is defined on a loopy graph");
    }
    auto is_free = [&](int32_t v) { return !(h->vinfo[v] & (kClamped | kGhost)); };
    // the variable tree: parent variable and parent factor of every free variable (members: parents before children)
    std::vector<int32_t> &vpar = F.vpar, &vfac = F.vfac, &vcomp = F.vcomp, &order = F.order;
    vpar.assign((size_t)nv, -1); vfac.assign((size_t)nv, -1); vcomp.assign((size_t)nv, -1); order.clear();
    int32_t comp = -1;
    for (int32_t n : R.members) {
        if (n >= nv) continue;
        if (R.level[n] == 0) comp++;
        vcomp[n] = comp;
        order.push_back(n);
        const int32_t e = R.parent_edge[n];
        if (e < 0) continue;
        const int32_t f = R.efac[e];
        vfac[n] = f;
        vpar[n] = h->edge_var[R.parent_edge[nv + f]];
    }
    P.n_comp = comp + 1;
    // heavy children
    std::vector<int64_t> size((size_t)nv, 1);
    std::vector<int32_t> heavy((size_t)nv, -1);
    for (size_t k = order.size(); k-- > 0;) {
        const int32_t v = order[k], p = vpar[v];
        if (p < 0) continue;
        size[p] += size[v];
        if (heavy[p] < 0 || size[v] > size[heavy[p]]) heavy[p] = v;
    }
    std::vector<int32_t> koff((size_t)nv + 1, 0), kid((size_t)order.size());
    for (int32_t v : order) if (vpar[v] >= 0) koff[vpar[v] + 1]++;
    for (int64_t v = 0; v < nv; v++) koff[v + 1] += koff[v];
    {
        std::vector<int32_t> at(koff.begin(), koff.end() - 1);
        for (int32_t v : order) if (vpar[v] >= 0) kid[at[vpar[v]]++] = v;
    }
    // paths by light depth: heads of depth l + 1 are the light children of the variables on the paths of depth l
    std::vector<int32_t> &pos_var = F.pos_var, &var_pos = F.var_pos, &roots = F.roots;
    std::vector<int4> &top = F.top;
    std::vector<int2> &rngs = F.rngs;
    pos_var.clear(); var_pos.assign((size_t)nv, -1); roots.clear(); top.clear(); rngs.clear();
    P.depths.clear();
    P.level_cap.assign(1, 0);
    std::vector<int32_t> heads;
    for (int32_t v : order) if (vpar[v] < 0) heads.push_back(v);
    while (!heads.empty()) {
        Depth dp;
        std::vector<int32_t> next;
        std::vector<int2> pr;            // per path: its positions
        std::vector<int32_t> ppar;       // per path: the position of the head's parent
        for (int32_t hd : heads) {
            const int32_t b = (int32_t)pos_var.size();
            for (int32_t v = hd; v >= 0; v = heavy[v]) {
                var_pos[v] = (int32_t)pos_var.size();
                pos_var.push_back(v);
                for (int32_t k = koff[v]; k < koff[v + 1]; k++) if (kid[k] != heavy[v]) next.push_back(kid[k]);
            }
            pr.push_back(make_int2(b, (int32_t)pos_var.size()));
            ppar.push_back(vpar[hd] < 0 ? -1 : var_pos[vpar[hd]]);
            if (vpar[hd] < 0) roots.push_back(b);
        }
        // tile levels until every path has at most `tile` items
        int64_t longest = 0;
        for (const int2 &r : pr) longest = std::max<int64_t>(longest, r.y - r.x);
        while (longest > tile) {
            std::vector<int2> up;
            const int64_t off = (int64_t)rngs.size();
            longest = 0;
            for (int2 &r : pr) {
                const int32_t b = (int32_t)up.size();
                for (int32_t a = r.x; a < r.y; a += tile) { rngs.push_back(make_int2(a, std::min<int32_t>(a + tile, r.y))); up.push_back(rngs.back()); }
                r = make_int2(b, (int32_t)up.size());
                longest = std::max<int64_t>(longest, r.y - r.x);
            }
            dp.levels++;
            dp.rng_off.push_back(off);
            dp.n_items.push_back((int64_t)up.size());
            if ((int64_t)P.level_cap.size() <= dp.levels) P.level_cap.push_back(0);
            P.level_cap[(size_t)dp.levels] = std::max<int64_t>(P.level_cap[(size_t)dp.levels], (int64_t)up.size());
        }
        dp.top_off = (int64_t)top.size();
        dp.n_paths = (int64_t)pr.size();
        dp.pos_end = (int64_t)pos_var.size();
        dp.pos_beg = P.depths.empty() ? 0 : P.depths.back().pos_end;
        if (!P.depths.empty()) P.depths.back().n_att = vpar[heads[0]] < 0 ? 0 : dp.n_paths;
        for (size_t k = 0; k < pr.size(); k++) top.push_back(make_int4(pr[k].x, pr[k].y, ppar[k], 0));
        P.depths.push_back(dp);
        heads.swap(next);
    }
    P.npos = (int64_t)pos_var.size();
    for (int64_t v = 0; v < nv; v++)      // (every variable is on an edge, so root_forest places every free one: the gather relies on it)
        if (is_free((int32_t)v) && var_pos[v] < 0) return fail(h, CX_ERR_STATE, who + ": variable " + std::to_string(h->var_ids[v]) + " is on no factor");
    P.n_root = (int64_t)roots.size();
    // components: their positions, contiguous, in chunks of at most kFlagChunk
    std::vector<int32_t> coff((size_t)P.n_comp + 1, 0), &cpos = F.cpos, &pcomp = F.pcomp, &cbeg = F.cbeg, &ccb = F.ccb;
    cpos.assign((size_t)P.npos, 0); pcomp.assign((size_t)P.npos, 0); cbeg.clear(); ccb.clear();
    for (int64_t q = 0; q < P.npos; q++) { pcomp[q] = vcomp[pos_var[q]]; coff[pcomp[q] + 1]++; }
    for (int64_t c = 0; c < P.n_comp; c++) coff[c + 1] += coff[c];
    {
        std::vector<int32_t> at(coff.begin(), coff.end() - 1);
        for (int64_t q = 0; q < P.npos; q++) cpos[at[pcomp[q]]++] = (int32_t)q;
    }
    for (int64_t c = 0; c < P.n_comp; c++) {
        ccb.push_back((int32_t)cbeg.size());
        for (int32_t a = coff[c]; a < coff[c + 1]; a += kFlagChunk) cbeg.push_back(a);
    }
    ccb.push_back((int32_t)cbeg.size());
    P.n_chunk = (int64_t)cbeg.size();
    cbeg.push_back((int32_t)P.npos);
    // a slot of every observed variable (its datum)
    F.dslot.assign((size_t)nv, 0);
    std::vector<int32_t> &dslot = F.dslot;
    for (int64_t v = 0; v < nv; v++) if (h->var_off[v + 1] > h->var_off[v]) dslot[v] = slot_of_edge(h, h->var_off[v]);
    return CX_OK;
}

// the forest's device side (the status bytes and flags with it)
inline int32_t upload_forest(cx_handle *h, ForestDev &P, const ForestDims &D, const Forest &F) {
    using namespace cxh;
    int32_t rc;
    if ((rc = dev_upload(h, &P.d_pos_var, F.pos_var)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &P.d_var_pos, F.var_pos)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &P.d_comp, F.pcomp)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &P.d_cpos, F.cpos)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &P.d_cbeg, F.cbeg)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &P.d_ccb, F.ccb)) != CX_OK) return rc;
    if ((rc = dev_alloc(h, &P.d_cpart, D.n_chunk)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &P.d_dslot, F.dslot)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &P.d_roots, F.roots)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &P.d_top, F.top)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &P.d_rng, F.rngs)) != CX_OK) return rc;
    if ((rc = dev_alloc(h, &P.d_st, D.npos)) != CX_OK) return rc;
    return dev_alloc(h, &P.d_cflag, D.n_comp);
}

inline int32_t build_plan(cx_handle *h, const ev::Cache &E, Plan &P, const std::string &who) {
    using namespace cxh;
    const int64_t nv = h->nv, nf = h->nf;
    Forest F;
    int32_t rc = build_forest(h, P, F, who);
    if (rc != CX_OK) return rc;
    const std::vector<int32_t> &order = F.order, &vpar = F.vpar, &vfac = F.vfac, &pos_var = F.pos_var, &var_pos = F.var_pos;
    const std::vector<int4> &top = F.top;
    const std::vector<int2> &rngs = F.rngs;
    auto is_free = [&](int32_t v) { return !(h->vinfo[v] & (kClamped | kGhost)); };
    // links: two-variable factors and factors of 3 .. 7 variables (their children's extra noise blocks)
    // (E.pair, E.krec: the pair rows (out slot, in slot, out var, in var) and k-ary rows (slots | vars) of cx_evidence.hip, on the host)
    std::vector<int4> plink;
    std::vector<int32_t> klink, xcnt((size_t)P.npos, 0);
    std::vector<std::pair<int32_t, int32_t>> kfac;       // (factor, parent variable) of every k-ary link factor
    std::vector<uint8_t> seen((size_t)nf, 0);
    for (int32_t v : order) {
        const int32_t f = vfac[v];
        if (f < 0 || seen[f]) continue;
        seen[f] = 1;
        if (E.row_of_fac[f] >= 0) {
            const int32_t r = E.row_of_fac[f];
            plink.push_back(make_int4(r, E.pair[r].z == v ? 1 : 0, var_pos[v], 0));
        } else if (E.kary_row_of_fac[f] >= 0) {
            kfac.push_back({f, vpar[v]});
        } else return fail(h, CX_ERR_STATE, who + ": factor " + std::to_string(h->fac_ids[f]) + " joins two free variables but has no Gaussian table row");
    }
    std::vector<int32_t> xoff((size_t)P.npos + 1, 0), xvar;
    std::vector<std::vector<int32_t>> kchild;
    for (auto &kp : kfac) {
        const int32_t row = E.kary_row_of_fac[kp.first];
        const int32_t *vr = &E.krec[(size_t)row * 16 + 8], *sl = &E.krec[(size_t)row * 16];
        int32_t rec[10];
        rec[0] = row; rec[1] = -1;
        std::vector<int32_t> ch;
        for (int e = 0; e < 8; e++) {
            rec[2 + e] = -1;
            if (sl[e] < 0 || !is_free(vr[e])) continue;
            if (vr[e] == kp.second) rec[1] = e;
            else {
                if (vfac[vr[e]] != kp.first) return fail(h, CX_ERR_STATE, who + ": the forest plan lost a child of factor " + std::to_string(h->fac_ids[kp.first]));
                rec[2 + e] = var_pos[vr[e]];
                ch.push_back(vr[e]);
            }
        }
        if (rec[1] < 0) return fail(h, CX_ERR_STATE, who + ": the forest plan lost the parent of factor " + std::to_string(h->fac_ids[kp.first]));
        klink.insert(klink.end(), rec, rec + 10);
        for (size_t i = 0; i < ch.size(); i++) xcnt[var_pos[ch[i]]] = (int32_t)(ch.size() - 1 - i);
        kchild.push_back(ch);
    }
    for (int64_t q = 0; q < P.npos; q++) xoff[q + 1] = xoff[q] + xcnt[q];
    xvar.assign((size_t)xoff[P.npos], 0);
    for (auto &ch : kchild)
        for (size_t i = 0; i < ch.size(); i++)
            for (size_t j = i + 1; j < ch.size(); j++) xvar[(size_t)xoff[var_pos[ch[i]]] + (j - i - 1)] = ch[j];
    P.n_plink = (int64_t)plink.size();
    P.n_klink = (int64_t)klink.size() / 10;
    P.n_xent = (int64_t)xvar.size();
    // the same two relations read from the other end: a position's light paths (in path order), the extra blocks that read a variable's ε
    std::vector<int32_t> att_off((size_t)P.npos + 1, 0), att_head, xt_off((size_t)P.npos + 1, 0);
    std::vector<int2> xt_ent((size_t)P.n_xent);
    for (const int4 &t : top) if (t.z >= 0) att_off[(size_t)t.z + 1]++;
    for (int64_t q = 0; q < P.npos; q++) for (int32_t x = xoff[q]; x < xoff[q + 1]; x++) xt_off[(size_t)var_pos[xvar[x]] + 1]++;
    for (int64_t q = 0; q < P.npos; q++) { att_off[q + 1] += att_off[q]; xt_off[q + 1] += xt_off[q]; }
    att_head.assign((size_t)att_off[P.npos], 0);
    {
        std::vector<int32_t> at(att_off.begin(), att_off.end() - 1), xt(xt_off.begin(), xt_off.end() - 1);
        for (const Depth &dp : P.depths)
            for (int64_t k = 0; k < dp.n_paths; k++) {
                const int4 &t = top[(size_t)(dp.top_off + k)];
                if (t.z < 0) continue;
                // the path's first position: of its first tile at every level, down to the positions
                int32_t b = t.x;
                for (int l = dp.levels; l >= 1; l--) b = rngs[(size_t)(dp.rng_off[(size_t)l - 1] + b)].x;
                att_head[(size_t)at[t.z]++] = b;
            }
        for (int64_t q = 0; q < P.npos; q++)
            for (int32_t x = xoff[q]; x < xoff[q + 1]; x++) xt_ent[(size_t)xt[var_pos[xvar[x]]]++] = make_int2((int32_t)q, x);
    }
    static_cast<PlanDev &>(P) = PlanDev();
    P.valid = false;
    const int d = h->cfg.dim, ln = 2 * d * d + d;
    if ((rc = upload_forest(h, P, P, F)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &P.d_plink, plink)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &P.d_att_off, att_off)) != CX_OK) return rc;
    if (!att_head.empty() && (rc = dev_upload(h, &P.d_att_head, att_head)) != CX_OK) return rc;
    if (P.n_klink) {
        if ((rc = dev_upload(h, &P.d_klink, klink)) != CX_OK) return rc;
        if ((rc = dev_upload(h, &P.d_xoff, xoff)) != CX_OK) return rc;
        if ((rc = dev_upload(h, &P.d_xvar, xvar)) != CX_OK) return rc;
        if ((rc = dev_upload(h, &P.d_xt_off, xt_off)) != CX_OK) return rc;
        if (!xt_ent.empty() && (rc = dev_upload(h, &P.d_xt_ent, xt_ent)) != CX_OK) return rc;
        if ((rc = dev_alloc(h, &P.d_xblk, std::max<int64_t>(P.n_xent, 1) * d * d)) != CX_OK) return rc;
    }
    if ((rc = dev_alloc(h, &P.d_link, std::max<int64_t>(P.npos, 1) * ln)) != CX_OK) return rc;
    const int levels = (int)P.level_cap.size() - 1;
    P.d_Gc.resize((size_t)levels + 1); P.d_oc.resize((size_t)levels + 1); P.d_carry.resize((size_t)levels + 1);
    for (int l = 1; l <= levels; l++)
        if ((rc = dev_alloc(h, &P.d_Gc[(size_t)l], P.level_cap[(size_t)l] * d * d)) != CX_OK) return rc;
    CX_HIP(h, hipStreamSynchronize(h->stream));      // (the host vectors die here)
    P.h_cflag.assign((size_t)P.n_comp, 0);
    P.nv = nv; P.ne = h->ne;
    P.vinfo = h->vinfo;
    P.valid = true;
    return CX_OK;
}

// the handle's plan, rebuilt when the graph or the observed flags have changed (a new graph frees it)
inline int32_t plan_of(cx_handle *h, const ev::Cache &E, const std::string &who, Plan *&Pp) {
    if (!h->sample) h->sample.reset(new Plan());
    Plan &P = *h->sample;
    if (!P.valid || P.nv != h->nv || P.ne != h->ne || P.vinfo != h->vinfo) {
        P.valid = false;
        const int32_t rc = build_plan(h, E, P, who);
        if (rc != CX_OK) return rc;
    }
    Pp = &P;
    return CX_OK;
}

// the per-call buffers for a chunk of S samples
inline int32_t ensure_chunk(cx_handle *h, Plan &P, int64_t S, int64_t n_out, bool noise) {
    using namespace cxh;
    const int d = h->cfg.dim;
    int32_t rc;
    if ((rc = P.d_Z.ensure(h, P.npos * S * d)) != CX_OK) return rc;
    for (size_t l = 1; l < P.level_cap.size(); l++)
        if ((rc = P.d_oc[l].ensure(h, std::max<int64_t>(P.level_cap[l] * S * d, 1))) != CX_OK ||
            (rc = P.d_carry[l].ensure(h, std::max<int64_t>(P.level_cap[l] * S * d, 1))) != CX_OK) return rc;
    if (noise && (rc = P.d_noise.ensure(h, S * h->nv * d)) != CX_OK) return rc;
    return P.d_out.ensure(h, S * n_out * d);
}

inline unsigned blocks(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }

template <int D>
void launch_cond(cx_handle *h, const ev::Cache &E, Plan &P) {
    const ev::Msgs msg = ev::msgs_of(h, E);
    if (P.n_root + P.n_plink)
        hipLaunchKernelGGL(k_sp_cond<D>, dim3(blocks(P.n_root + P.n_plink, kT)), dim3(kT), 0, h->stream, P.n_root, P.n_plink, P.d_roots, P.d_plink,
                           P.d_pos_var, E.pair_tab(), msg, P.d_link, P.d_st);
    if (P.n_klink)
        hipLaunchKernelGGL(k_sp_cond_kary<D>, dim3(blocks(P.n_klink, kKT)), dim3(kKT), 0, h->stream, P.n_klink, P.d_klink, E.kary_tab(), msg, P.d_xoff,
                           P.d_link, P.d_xblk, P.d_st);
    if (P.n_comp) {
        hipLaunchKernelGGL(k_sp_flag, dim3((unsigned)P.n_chunk), dim3(kT), 0, h->stream, P.d_cbeg, P.d_cpos, P.d_st, P.d_cpart);
        hipLaunchKernelGGL(k_sp_flag_comp, dim3(blocks(P.n_comp, kT)), dim3(kT), 0, h->stream, P.n_comp, P.d_ccb, P.d_cpart, P.d_cflag);
    }
}

template <int D>
void launch_samples(cx_handle *h, Plan &P, int S, const Gen &g) {
    const int32_t *xo = P.n_klink ? P.d_xoff : nullptr;
    for (const Depth &dp : P.depths) {
        // up: the tiles' composed maps, level by level
        for (int l = 1; l <= dp.levels; l++) {
            const int64_t n = dp.n_items[(size_t)l - 1];
            const int2 *rng = P.d_rng + dp.rng_off[(size_t)l - 1];
            if (l == 1)
                hipLaunchKernelGGL((k_sp_compose<D, true>), dim3(blocks(n * (S + 1), kT)), dim3(kT), 0, h->stream, n, S, rng, P.d_link, P.d_pos_var, xo,
                                   P.d_xvar, P.d_xblk, g, nullptr, nullptr, P.d_Gc[1], P.d_oc[1]);
            else
                hipLaunchKernelGGL((k_sp_compose<D, false>), dim3(blocks(n * (S + 1), kT)), dim3(kT), 0, h->stream, n, S, rng, P.d_link, P.d_pos_var, xo,
                                   P.d_xvar, P.d_xblk, g, P.d_Gc[(size_t)l - 1], P.d_oc[(size_t)l - 1], P.d_Gc[(size_t)l], P.d_oc[(size_t)l]);
        }
        // the paths from their heads' parents
        const int4 *top = P.d_top + dp.top_off;
        const int L = dp.levels;
        if (L == 0)
            hipLaunchKernelGGL((k_sp_walk<D, true, true>), dim3(blocks(dp.n_paths * S, kT)), dim3(kT), 0, h->stream, dp.n_paths, S, top, nullptr, nullptr,
                               P.d_link, P.d_pos_var, xo, P.d_xvar, P.d_xblk, g, nullptr, nullptr, nullptr, P.d_Z);
        else
            hipLaunchKernelGGL((k_sp_walk<D, false, true>), dim3(blocks(dp.n_paths * S, kT)), dim3(kT), 0, h->stream, dp.n_paths, S, top, nullptr, nullptr,
                               P.d_link, P.d_pos_var, xo, P.d_xvar, P.d_xblk, g, P.d_Gc[(size_t)L], P.d_oc[(size_t)L], P.d_carry[(size_t)L], P.d_Z);
        // down: from every tile's carry
        for (int l = L; l >= 1; l--) {
            const int64_t n = dp.n_items[(size_t)l - 1];
            const int2 *rng = P.d_rng + dp.rng_off[(size_t)l - 1];
            if (l == 1)
                hipLaunchKernelGGL((k_sp_walk<D, true, false>), dim3(blocks(n * S, kT)), dim3(kT), 0, h->stream, n, S, nullptr, rng, P.d_carry[1], P.d_link,
                                   P.d_pos_var, xo, P.d_xvar, P.d_xblk, g, nullptr, nullptr, nullptr, P.d_Z);
            else
                hipLaunchKernelGGL((k_sp_walk<D, false, false>), dim3(blocks(n * S, kT)), dim3(kT), 0, h->stream, n, S, nullptr, rng, P.d_carry[(size_t)l],
                                   P.d_link, P.d_pos_var, xo, P.d_xvar, P.d_xblk, g, P.d_Gc[(size_t)l - 1], P.d_oc[(size_t)l - 1], P.d_carry[(size_t)l - 1],
                                   P.d_Z);
        }
    }
}

template <int D>
void launch_gather(cx_handle *h, const ev::Cache &E, Plan &P, int64_t n, int S, const int32_t *vids) {
    hipLaunchKernelGGL(k_sp_gather<D>, dim3(blocks(n * S, kT)), dim3(kT), 0, h->stream, n, S, vids, h->d_vinfo, P.d_dslot, P.d_var_pos, P.d_comp, P.d_cflag,
                       ev::v2f_of(h), E.d_W, P.d_Z, P.d_out);
}

template <int D>
void launch_all(cx_handle *h, const ev::Cache &E, Plan &P, int S, const Gen &g, int64_t n, const int32_t *vids, bool cond) {
    if (cond) launch_cond<D>(h, E, P);
    launch_samples<D>(h, P, S, g);
    launch_gather<D>(h, E, P, n, S, vids);
}

}  // namespace sp
}  // namespace cx
