// cx_evidence.hip — cx_log_evidence: log p(data) of a Gaussian model (dim 1 .. 4) from the stored factor→variable messages, on the
// device.  No counterpart in the reference (Cortex.jl computes no numbers); the derivation is DESIGN.md §4e.
//
//   log Z = Σ_o c_o + Σ_a log z_a + Σ_i (1 - d_i) log z_i
//
// M_i = the product of variable i's stored factor→variable messages (natural parameters), d_i = its factors that carry a rule,
// z_a = ∫ f_a Π m_{i→a} with m_{i→a} = M_i / m_{a→i}, z_i = ∫ M_i, c_o = the log-normaliser of a caller-set (opaque) message.
// Every term is evaluated in coordinates centred on the belief mean μ_i of each variable (x_i = μ_i + u_i): the constants that the
// shift pulls out of the terms of one variable sum to those of its opaque messages alone (the leave-one-out messages add up to
// d_i M_i minus the rule messages), so nothing of size ½ η'Λ⁻¹η — 10^12 for data of size 10^6 — is formed and cancelled.
//
//   pass 1 (k_ev_var)   one thread per variable: M_i over its SELL slots, μ_i, the variable term (Cholesky log-det) and the centred
//                       opaque terms log N(μ_i; μ_o, Λ_o⁻¹); writes (μ_i | η_i, Λ_i, positive-definite flag) to a per-variable scratch
//   pass 2 (k_ev_pair)  one thread per two-variable factor: the factor belief's joint precision (2d x 2d, registers), its log-det and
//                       quadratic form — a flat leaf message is a zero block of a matrix that stays positive definite
//          (k_ev_kary)  one thread per factor of 3 .. 7 variables, its joint precision (up to 28 x 28) packed in LDS
//   k_ev_final          the per-block partial sums (compensated, f64) in a fixed order: two calls on one state are bit-identical
// The counters travel with the partial sums (per block, then in index order): no atomics at all.
//
// cx_log_evidence_components: the same terms summed per connected component of the graph — the passes' term entries
// write one term per thread, k_ev_seg / k_ev_span add them up over the terms sorted by component (a segmented scan; no atomics either).
#include "cx_components.h"
#include "cx_evidence_core.h"

namespace cx {
namespace ev {

constexpr int kKB = 16;        // threads per block of the k-ary pass: each thread's joint precision lives in LDS
constexpr int kFB = 1024;      // threads of the one block of the final sum (C4: 23 k block partials)

// Every pass has two entries over one body: the one cx_log_evidence launches (TERMS false: the block's Part, block_part) and the term
// entry of cx_log_evidence_components (TERMS true: the thread's term and flag bits at its index, coalesced; the caller passes the
// arrays offset to the pass's first term)
template <bool TERMS>
using PassOut = std::conditional_t<TERMS, TermOut, Part *__restrict__>;
__device__ __forceinline__ void put_term(const TermOut &o, int64_t i, double s, double c, bool vterm, bool undef, bool npd, bool ghost) {
    o.val[i] = s + c;
    o.flag[i] = (uint8_t)((vterm ? kTermVar : 0u) | (undef ? kTermUndef : 0u) | (npd ? kTermNpd : 0u) | (ghost ? kTermGhost : 0u));
}

// ---- pass 1: variables ----------------------------------------------------------------------------------------------------------
// vrec[v] = d_v (low 24 bits) | opaque mask of the SELL slots (bits 24..31); variables of the CSR tail read tail_opq[slot - tail0]
template <int D, bool TERMS = false>
__global__ __launch_bounds__(kB) void k_ev_var(int64_t nv, const int32_t *__restrict__ vbase, const int32_t *__restrict__ vdeg,
                                               const uint8_t *__restrict__ vinfo, const int32_t *__restrict__ vrec,
                                               const uint8_t *__restrict__ tail_opq, int32_t tail0, const double *__restrict__ f2v,
                                               double *__restrict__ W, PassOut<TERMS> partial) {
    constexpr int NT = Lay<D>::NT, K = Lay<D>::K;
    const int64_t v = (int64_t)blockIdx.x * kB + threadIdx.x;
    double s = 0.0, c = 0.0;
    bool ghost = false, vterm = false, undef_t = false, npd_t = false;
    if (v < nv) {
        const int info = vinfo[v];
        ghost = (info & kGhost) != 0;
        if (!ghost && !(info & kClamped)) {
            const int deg = vdeg[v], b = vbase[v], rec = vrec[v];
            const bool big = (info & kDegMask) == kBigDeg;
            const int stride = big ? 1 : kBlock, di = rec & 0xffffff, mask = (rec >> 24) & 0xff;
            double eta[D], lam[NT];
#pragma unroll
            for (int k = 0; k < D; k++) eta[k] = 0.0;
#pragma unroll
            for (int k = 0; k < NT; k++) lam[k] = 0.0;
            for (int k = 0; k < deg; k++) {
                double e[D], l[NT];
                ld_msg<D>(f2v, b + k * stride, e, l);
#pragma unroll
                for (int q = 0; q < D; q++) eta[q] += e[q];
#pragma unroll
                for (int q = 0; q < NT; q++) lam[q] += l[q];
            }
            bool undef = false;
#pragma unroll
            for (int q = 0; q < D; q++) undef = undef || __builtin_isnan(eta[q]);
#pragma unroll
            for (int q = 0; q < NT; q++) undef = undef || __builtin_isnan(lam[q]);
            double L[D][D], y[D], mu[D], logdet, quad;
#pragma unroll
            for (int i = 0; i < D; i++) {
                y[i] = eta[i]; mu[i] = 0.0;
#pragma unroll
                for (int j = 0; j < D; j++) L[i][j] = lam_at<D>(lam, i, j);
            }
            const bool pd = !undef && chol_quad<D>(L, y, logdet, quad);
            if (pd) back_solve<D>(L, y, mu);
            double *w = W + v * K;
#pragma unroll
            for (int i = 0; i < D; i++) w[i] = pd ? mu[i] : eta[i];
#pragma unroll
            for (int i = 0; i < NT; i++) w[D + i] = lam[i];
            if constexpr (D > 1) {
                w[D + NT] = pd ? 1.0 : 0.0;
                if (K > D + NT + 1) w[K - 1] = 0.0;
            }
            if (di != 1) {
                vterm = true;
                undef_t = undef;
                npd_t = !undef && !pd;
                if (pd) neu(s, c, (double)(1 - di) * 0.5 * (D * kLog2Pi - logdet));
            }
            // the opaque messages, centred on μ_i: c_o + η_o'μ - ½ μ'Λ_o μ = log N(μ_i; μ_o, Λ_o⁻¹) when Λ_o is positive definite,
            // η_o'μ - ½ μ'Λ_o μ otherwise (c_o = 0); an undefined one is skipped
            for (int k = 0; k < deg; k++) {
                const bool opq = big ? tail_opq[b + k - tail0] != 0 : ((mask >> k) & 1) != 0;
                if (!opq) continue;
                double e[D], l[NT];
                ld_msg<D>(f2v, b + k * stride, e, l);
                bool u = false;
#pragma unroll
                for (int q = 0; q < D; q++) u = u || __builtin_isnan(e[q]);
#pragma unroll
                for (int q = 0; q < NT; q++) u = u || __builtin_isnan(l[q]);
                if (u) continue;
                double Lo[D][D], r[D], ld, qd;
#pragma unroll
                for (int i = 0; i < D; i++) {
                    double t = e[i];
#pragma unroll
                    for (int j = 0; j < D; j++) { Lo[i][j] = lam_at<D>(l, i, j); t -= Lo[i][j] * mu[j]; }
                    r[i] = t;
                }
                if (chol_quad<D>(Lo, r, ld, qd)) {
                    neu(s, c, -0.5 * qd + 0.5 * ld - 0.5 * D * kLog2Pi);
                } else {
                    double t = 0.0;
#pragma unroll
                    for (int i = 0; i < D; i++) {
                        double lm = 0.0;
#pragma unroll
                        for (int j = 0; j < D; j++) lm += lam_at<D>(l, i, j) * mu[j];
                        t += mu[i] * (e[i] - 0.5 * lm);
                    }
                    neu(s, c, t);
                }
            }
        }
    }
    if constexpr (TERMS) { if (v < nv) put_term(partial, v, s, c, vterm, undef_t, npd_t, ghost); }
    else block_part<kB>(s, c, vterm, undef_t, npd_t, ghost, partial);
}

// ---- pass 2: factors of two variables -------------------------------------------------------------------------------------------
// x_out = A x_in + b + N(0, Q): log z_a = -½ rc'Q⁻¹rc - ½ log det 2πQ + ½ h'J⁻¹h - ½ log det J + (free entries) ½ log 2π, with J, h of
// ev::pair_joint.  Both ends free: the 2d x 2d joint; one end observed (half the factors of a state-space chain): its d x d block
template <int D, bool TERMS = false>
__global__ __launch_bounds__(kB) void k_ev_pair(int64_t n, PairTab tab, Msgs msg, PassOut<TERMS> partial) {
    const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
    double s = 0.0, c = 0.0;
    bool undef_t = false, npd_t = false;
    if (i < n) {
        PairJoint<D> B;
        pair_joint<D>(i, tab, msg, B);
        double cq = 0.0;
#pragma unroll
        for (int p = 0; p < D; p++) cq -= B.rc[p] * B.g[p];
        double lz = -0.5 * cq - 0.5 * B.ldq, logdet = 0.0, quad = 0.0;
        bool pd = true;
        if (B.fo && B.fi) {
            pd = chol_quad<2 * D>(B.J, B.h, logdet, quad);
            lz += 0.5 * quad - 0.5 * logdet + D * kLog2Pi;
        } else if (B.fo || B.fi) {
            double J[D][D], h[D];
#pragma unroll
            for (int p = 0; p < D; p++) {
                h[p] = B.fo ? B.h[p] : B.h[D + p];
#pragma unroll
                for (int q = 0; q < D; q++) J[p][q] = B.fo ? B.J[p][q] : B.J[D + p][D + q];
            }
            pd = chol_quad<D>(J, h, logdet, quad);
            lz += 0.5 * quad - 0.5 * logdet + 0.5 * D * kLog2Pi;
        }
        undef_t = !B.ok;
        npd_t = B.ok && !pd;
        if (B.ok && pd) neu(s, c, lz);
    }
    if constexpr (TERMS) { if (i < n) put_term(partial, i, s, c, false, undef_t, npd_t, false); }
    else block_part<kB>(s, c, 0, undef_t, npd_t, 0, partial);
}

// ---- pass 2: factors of 3 .. 7 variables ----------------------------------------------------------------------------------------
// The joint precision over the free entries (ev::kary_joint: packed lower triangle, up to 28 x 28) and its right-hand side live in LDS,
// thread-interleaved.
template <int D, bool TERMS = false>
__global__ __launch_bounds__(kKB) void k_ev_kary(int64_t n, KaryTab tab, Msgs msg, PassOut<TERMS> partial) {
    constexpr int NP = KLay<D>::NP, NM = KLay<D>::NM;
    __shared__ double sJ[NP * kKB], sh[NM * kKB];
    const int t = threadIdx.x;
    double *J = sJ + t, *hv = sh + t;      // element k at [k * kKB]
    const int64_t f = (int64_t)blockIdx.x * kKB + t;
    double s = 0.0, c = 0.0;
    bool undef_t = false, npd_t = false;
    if (f < n) {
        double Qi[D][D], ldq, bp[D], g[D], cq;
        unsigned freemask;
        int nfree;
        bool ok;
        kary_joint<D, kKB>(f, tab, msg, J, hv, Qi, ldq, bp, g, cq, freemask, nfree, ok);
        double lz = -0.5 * cq - 0.5 * ldq;
        const int N = nfree * D;
        auto at = [&](int i, int j) -> double & { return J[pk(i, j) * kKB]; };
        auto y = [&](int i) -> double & { return hv[i * kKB]; };
        double logdet = 0.0, quad = 0.0;
        const bool pd = chol_at(N, at, &logdet);
        if (pd) {
            fwd_solve_at(N, at, y);
            for (int i = 0; i < N; i++) quad += y(i) * y(i);
        }
        lz += 0.5 * quad - 0.5 * logdet + 0.5 * N * kLog2Pi;
        undef_t = !ok;
        npd_t = ok && !pd;
        if (ok && pd) neu(s, c, lz);
    }
    if constexpr (TERMS) { if (f < n) put_term(partial, f, s, c, false, undef_t, npd_t, false); }
    else block_part<kKB>(s, c, 0, undef_t, npd_t, 0, partial);
}

// ---- the partial sums and counters in index order; out = value | counters[kNCnt] (u64) ------------------------------------------
__global__ __launch_bounds__(kFB) void k_ev_final(int64_t n, const Part *__restrict__ partial, double *__restrict__ out) {
    __shared__ double ss[kFB], cs[kFB];
    __shared__ unsigned long long ns[kNCnt][kFB];
    const int t = threadIdx.x;
    double s = 0.0, c = 0.0;
    unsigned long long m[kNCnt] = {0, 0, 0, 0};
    for (int64_t i = t; i < n; i += kFB) {
        const Part p = partial[i];
        neu(s, c, p.s);
        c += p.c;
#pragma unroll
        for (int k = 0; k < kNCnt; k++) m[k] += p.n[k];
    }
    ss[t] = s; cs[t] = c;
#pragma unroll
    for (int k = 0; k < kNCnt; k++) ns[k][t] = m[k];
    __syncthreads();
    for (int w = kFB / 2; w > 0; w >>= 1) {
        if (t < w) {
            double a = ss[t], ac = cs[t];
            neu(a, ac, ss[t + w]);
            ss[t] = a; cs[t] = ac + cs[t + w];
#pragma unroll
            for (int k = 0; k < kNCnt; k++) ns[k][t] += ns[k][t + w];
        }
        __syncthreads();
    }
    if (t == 0) out[0] = ss[0] + cs[0];
    if (t < kNCnt) reinterpret_cast<unsigned long long *>(out)[1 + t] = ns[t][0];
}

// ---- the terms summed per component (cx_log_evidence_components) ---------------------------------------------------
// The terms sorted by (component, term index) lie at the positions of comp::sort_terms, cut into tiles of kTile positions, one block
// each.  A block reduces every run of one component inside its tile by a segmented scan (head flag: the component differs from the
// position before; the tile's first position is a head): four positions per thread in order, the threads' aggregates by wave64
// shuffles, the waves' through LDS.  A component of up to kTile terms lies inside one tile (its alignment) and goes straight to cval /
// ccnt; a longer one starts a tile, is the first run of every tile it reaches, leaves one TilePart per tile, and k_ev_span adds those up
// in tile order.  Every sum is compensated (neu) and taken in an order that the component's own terms fix (the alignment again): no
// atomics, two calls are bit-identical, and a component's value does not depend on which others share the graph.
constexpr int kSB = 256, kSI = 4, kTile = kSB * kSI;

struct Acc {
    double s, c;
    unsigned long long n;      // the four counters, 16 bits each (a tile holds 1024 terms)
};
__device__ __forceinline__ void acc_add(Acc &a, const Acc &b) {      // a <- a + b, a's terms first
    neu(a.s, a.c, b.s);
    a.c += b.c;
    a.n += b.n;
}
__device__ __forceinline__ Acc acc_shfl_up(const Acc &a, int off) { return {__shfl_up(a.s, off), __shfl_up(a.c, off), __shfl_up(a.n, off)}; }
__device__ __forceinline__ void put_comp(const Acc &a, int k, double *__restrict__ cval, unsigned long long *__restrict__ ccnt) {
    cval[k] = a.s + a.c;
#pragma unroll
    for (int q = 0; q < kNCnt; q++) ccnt[(int64_t)k * kNCnt + q] = (a.n >> (16 * q)) & 0xffffull;
}

// perm, key [npos], npos a multiple of kSI (the threads load four at once); -1: a position without a term
__global__ __launch_bounds__(kSB) void k_ev_seg(int64_t npos, const int32_t *__restrict__ perm, const int32_t *__restrict__ key,
                                                const int64_t *__restrict__ sbeg, const int64_t *__restrict__ send, const double *__restrict__ tval,
                                                const uint8_t *__restrict__ tflag, TilePart *__restrict__ tpart, double *__restrict__ cval,
                                                unsigned long long *__restrict__ ccnt) {
    __shared__ Acc wv[kSB / 64];
    __shared__ int wf[kSB / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t tile0 = (int64_t)blockIdx.x * kTile, tile1 = tile0 + kTile < npos ? tile0 + kTile : npos;
    const int64_t p0 = tile0 + (int64_t)t * kSI;
    int k[kSI + 1], kprev = -1;      // k[kSI]: the component of the position after the thread's (-1: no term there, -2: past the tile)
    Acc x[kSI];
#pragma unroll
    for (int j = 0; j < kSI; j++) { k[j] = -2; x[j] = {0.0, 0.0, 0ull}; }
    k[kSI] = -2;
    if (p0 < tile1) {
        const int4 pp = reinterpret_cast<const int4 *>(perm)[p0 / kSI], kk = reinterpret_cast<const int4 *>(key)[p0 / kSI];
        const int pj[kSI] = {pp.x, pp.y, pp.z, pp.w}, kj[kSI] = {kk.x, kk.y, kk.z, kk.w};
#pragma unroll
        for (int j = 0; j < kSI; j++)
            if (p0 + j < tile1 && kj[j] >= 0 && pj[j] >= 0) {
                k[j] = kj[j];
                const unsigned f = tflag[pj[j]];
                x[j] = {tval[pj[j]], 0.0,
                        (unsigned long long)(f & 1u) | (unsigned long long)((f >> 1) & 1u) << 16 | (unsigned long long)((f >> 2) & 1u) << 32 |
                            (unsigned long long)((f >> 3) & 1u) << 48};
            }
        if (p0 > tile0) kprev = key[p0 - 1];
        if (p0 + kSI < tile1) k[kSI] = key[p0 + kSI];
    }
    // the thread's aggregate: the sum of its positions after its last head (all of them without one) and whether it holds a head
    Acc v = {0.0, 0.0, 0ull};
    int fl = 0;
#pragma unroll
    for (int j = 0; j < kSI; j++) {
        if (k[j] < 0) continue;
        if (k[j] != (j ? k[j - 1] : kprev)) { fl = 1; v = x[j]; }
        else acc_add(v, x[j]);
    }
    // inclusive segmented scan of the aggregates over the wave, then over the block's waves
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        Acc u = acc_shfl_up(v, off);
        const int uf = __shfl_up(fl, off);
        if (lane >= off) {
            if (!fl) { acc_add(u, v); v = u; }
            fl |= uf;
        }
    }
    if (lane == 63) { wv[w] = v; wf[w] = fl; }
    __syncthreads();
    Acc carry = {0.0, 0.0, 0ull};      // the run that reaches the thread's first position from the positions before it
    for (int i = 0; i < w; i++) {
        if (wf[i]) carry = wv[i];
        else acc_add(carry, wv[i]);
    }
    {
        const Acc e = acc_shfl_up(v, 1);
        const int ef = __shfl_up(fl, 1);
        if (lane > 0) {
            if (ef) carry = e;
            else acc_add(carry, e);
        }
    }
    // the runs that end at one of the thread's positions
#pragma unroll
    for (int j = 0; j < kSI; j++) {
        if (k[j] < 0) continue;
        if (k[j] != (j ? k[j - 1] : kprev)) carry = x[j];
        else acc_add(carry, x[j]);
        const int knext = p0 + j + 1 < tile1 ? k[j + 1] : -2;
        if (knext == k[j]) continue;
        if (sbeg[k[j]] >= tile0 && send[k[j]] <= tile1) put_comp(carry, k[j], cval, ccnt);
        else tpart[blockIdx.x] = {carry.s, carry.c, carry.n};
    }
}

// one wave per component of more than kTile terms: its pieces in tile order, lanes striding the tiles, then a fixed shuffle tree
__global__ __launch_bounds__(kSB) void k_ev_span(int64_t ns, const int32_t *__restrict__ span, const int64_t *__restrict__ sbeg, const int64_t *__restrict__ send,
                                                 const TilePart *__restrict__ tpart, double *__restrict__ cval, unsigned long long *__restrict__ ccnt) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (kSB / 64) + (threadIdx.x >> 6);
    if (i >= ns) return;      // (the whole wave)
    const int k = span[i];
    const int64_t t0 = sbeg[k] / kTile, t1 = (send[k] - 1) / kTile;
    double s = 0.0, c = 0.0;
    unsigned long long m[kNCnt] = {0, 0, 0, 0};
    for (int64_t tt = t0 + lane; tt <= t1; tt += 64) {
        const TilePart p = tpart[tt];
        neu(s, c, p.s);
        c += p.c;
#pragma unroll
        for (int q = 0; q < kNCnt; q++) m[q] += (p.n >> (16 * q)) & 0xffffull;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double s2 = __shfl_down(s, off), c2 = __shfl_down(c, off);
        neu(s, c, s2);
        c += c2;
#pragma unroll
        for (int q = 0; q < kNCnt; q++) m[q] += __shfl_down(m[q], off);
    }
    if (lane == 0) {
        cval[k] = s + c;
#pragma unroll
        for (int q = 0; q < kNCnt; q++) ccnt[(int64_t)k * kNCnt + q] = m[q];
    }
}

// ---- host: the work lists -------------------------------------------------------------------------------------------------------

int32_t build(cx_handle *h, Cache &C, const std::string &who) {
    using namespace cxh;
    const int d = h->cfg.dim;
    const int64_t nv = h->nv, ne = h->ne, nf = h->nf;
    std::vector<int32_t> slot_var((size_t)h->nslots, -1), fe1((size_t)nf, -1), fe2((size_t)nf, -1), efac((size_t)ne);
    for (int64_t e = 0; e < ne; e++) {
        slot_var[slot_of_edge(h, e)] = h->edge_var[e];
        const int64_t f = find_factor(h, h->edge_fac_id[e]);
        efac[e] = (int32_t)f;
        if (fe1[f] < 0) fe1[f] = (int32_t)e; else if (fe2[f] < 0) fe2[f] = (int32_t)e;
    }
    // variables: d_i and which slots hold opaque messages
    const bool has_tail = !h->big_vars.empty();
    std::vector<int32_t> vrec((size_t)nv, 0);
    std::vector<uint8_t> tail(has_tail ? (size_t)(h->nslots - h->big_start) : 1, 0);
    for (int64_t v = 0; v < nv; v++) {
        const bool big = (h->vinfo[v] & kDegMask) == kBigDeg;
        int32_t di = 0, mask = 0;
        for (int32_t e = h->var_off[v]; e < h->var_off[v + 1]; e++) {
            const int k = e - h->var_off[v];
            if (h->fac_kind[efac[e]] == CX_FACTOR_OPAQUE) {
                if (big) tail[slot_of_edge(h, e) - h->big_start] = 1;
                else mask |= 1 << k;
            } else di++;
        }
        vrec[v] = di | (mask << 24);
    }
    // factors
    // (C is a fresh Cache: prepare drops a Cache whose build failed, so the rows below are appended to empty vectors)
    std::vector<int4> &pair = C.pair;
    std::vector<int32_t> &pair_ps = C.pair_ps, &krec = C.krec;
    std::vector<int64_t> &pair_fac = C.pair_fac;
    std::vector<double> pq, pa, pb;
    bool any_ab = false;
    C.row_of_fac.assign((size_t)nf, -1); C.kary_row_of_fac.assign((size_t)nf, -1);
    C.zero_noise_fac = -1; C.unsupported_fac = -1;
    int64_t row = 0;
    for (int64_t f = 0; f < nf; f++) {
        const int32_t kind = h->fac_kind[f];
        const double *p = &h->fac_params[f * CX_NPARAM];
        if (kind == CX_FACTOR_OPAQUE) continue;
        if (kind == CX_FACTOR_GAUSS_LINEAR_N) {
            for (int e = 0; e < 8; e++) krec.push_back(h->kary_slot[8 * row + e]);
            for (int e = 0; e < 8; e++) { const int32_t s = h->kary_slot[8 * row + e]; krec.push_back(s < 0 ? -1 : slot_var[s]); }
            if (d == 1 && !(h->kary_qb[2 * row] > 0.0) && C.zero_noise_fac < 0) C.zero_noise_fac = h->fac_ids[f];
            C.kary_row_of_fac[(size_t)f] = (int32_t)row++;
            continue;
        }
        if ((kind != CX_FACTOR_GAUSS_ADDITIVE && kind != CX_FACTOR_GAUSS_LINEAR) || fe2[f] < 0) { if (C.unsupported_fac < 0) C.unsupported_fac = h->fac_ids[f]; continue; }
        const int32_t s1 = slot_of_edge(h, fe1[f]), s2 = slot_of_edge(h, fe2[f]);
        int32_t so = s1, si = s2;
        if (d > 1) {
            if ((h->spdir[s1] & 1) == 0) { so = s2; si = s1; }      // spdir[in slot] = 2 * set (the message it sends goes forward)
            pair_ps.push_back(h->spdir[si] >> 1);
        } else {
            if (kind == CX_FACTOR_GAUSS_LINEAR && !h->lin_out_is_second[f]) { so = s1; si = s2; }
            else if (kind == CX_FACTOR_GAUSS_LINEAR) { so = s2; si = s1; }
            const double a = kind == CX_FACTOR_GAUSS_LINEAR ? p[1] : 1.0, b = kind == CX_FACTOR_GAUSS_LINEAR ? p[2] : 0.0;
            pq.push_back(p[0]); pa.push_back(a); pb.push_back(b);
            any_ab = any_ab || a != 1.0 || b != 0.0;
            if (!(p[0] > 0.0) && C.zero_noise_fac < 0) C.zero_noise_fac = h->fac_ids[f];
        }
        C.row_of_fac[(size_t)f] = (int32_t)pair.size();
        pair.push_back(make_int4(so, si, slot_var[so], slot_var[si]));
        pair_fac.push_back(f);
    }
    if (row != h->n_kary) return fail(h, CX_ERR_STATE, who + ": the k-ary table does not match the factors");
    C.n_pair = (int64_t)pair.size(); C.n_kary = row;
    int32_t rc;
    if ((rc = dev_upload(h, &C.d_vrec, vrec)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &C.d_tail, tail)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &C.d_pair, pair)) != CX_OK) return rc;
    if (d > 1) { if ((rc = dev_upload(h, &C.d_pair_ps, pair_ps)) != CX_OK) return rc; }
    else {
        if ((rc = dev_upload(h, &C.d_pq, pq)) != CX_OK) return rc;
        if (any_ab) {
            if ((rc = dev_upload(h, &C.d_pa, pa)) != CX_OK) return rc;
            if ((rc = dev_upload(h, &C.d_pb, pb)) != CX_OK) return rc;
        }
    }
    if ((rc = dev_upload(h, &C.d_krec, krec)) != CX_OK) return rc;
    if ((rc = dev_alloc(h, &C.d_W, nv * with_dim(d, [](auto D) { return Lay<D()>::K; }))) != CX_OK) return rc;
    C.nb = (nv + kB - 1) / kB + (C.n_pair + kB - 1) / kB + (C.n_kary + kKB - 1) / kKB;
    if ((rc = dev_alloc(h, &C.d_partial, C.nb)) != CX_OK) return rc;
    if ((rc = dev_alloc(h, &C.d_out, 1 + kNCnt)) != CX_OK) return rc;
    CX_HIP(h, hipHostMalloc((void **)&C.h_out, (1 + kNCnt) * sizeof(double), hipHostMallocDefault));
    CX_HIP(h, hipStreamSynchronize(h->stream));      // (the local host vectors die here)
    C.built = true;
    C.epoch = ~0ull;
    return CX_OK;
}

// the parameters that may change after cx_graph_create: k-ary coefficients (dim 1), (A, Q) sets and the k-ary edges' sets (dim > 1)
int32_t refresh_params(cx_handle *h, Cache &C, const std::string &who) {
    using namespace cxh;
    if (C.epoch == h->param_epoch) return CX_OK;
    const int d = h->cfg.dim;
    int32_t rc;
    if (d == 1) {
        std::vector<double> kc((size_t)C.n_kary * 10);
        for (int64_t r = 0; r < C.n_kary; r++) {
            for (int e = 0; e < 8; e++) kc[r * 10 + e] = h->kary_coef[8 * r + e];
            kc[r * 10 + 8] = h->kary_qb[2 * r]; kc[r * 10 + 9] = h->kary_qb[2 * r + 1];
        }
        if ((rc = dev_upload(h, &C.d_kc, kc)) != CX_OK) return rc;
    } else {
        std::vector<int32_t> kps((size_t)C.n_kary * 8, 0);
        std::vector<char> used;
        auto use = [&](int32_t s) { if ((size_t)s >= used.size()) used.resize((size_t)s + 1, 0); used[(size_t)s] = 1; };
        for (int32_t s : C.pair_ps) use(s);
        for (int64_t r = 0; r < C.n_kary; r++)
            for (int e = 0; e < 8; e++) {
                const int32_t s = h->kary_slot[8 * r + e] < 0 ? 0 : h->kary_pset[8 * r + e];
                kps[r * 8 + e] = s;
                if (h->kary_slot[8 * r + e] >= 0) use(s);
            }
        const int64_t nsets = (int64_t)used.size(), per = 2 * d * d + 2;
        std::vector<double> tab((size_t)std::max<int64_t>(nsets, 1) * per, 0.0);
        for (int64_t s = 0; s < nsets; s++) {
            if (!used[s]) continue;
            if (s >= (int64_t)h->psets.size() || h->psets[s].empty())
                return fail(h, CX_ERR_STATE, who + ": parameter set " + std::to_string(s) + " was never set (cx_set_factor_matrices)");
            const double *A = h->psets[s].data(), *Q = A + d * d;
            // Q = L L': log det 2πQ and Q⁻¹ (Q is symmetric positive definite: cx_set_factor_matrices checks it)
            double L[4][4] = {}, Li[4][4] = {}, ld = d * kLog2Pi;
            for (int j = 0; j < d; j++) {
                double t = Q[j * d + j];
                for (int k = 0; k < j; k++) t -= L[j][k] * L[j][k];
                L[j][j] = std::sqrt(t); ld += std::log(t);
                for (int i = j + 1; i < d; i++) {
                    double u = 0.5 * (Q[i * d + j] + Q[j * d + i]);
                    for (int k = 0; k < j; k++) u -= L[i][k] * L[j][k];
                    L[i][j] = u / L[j][j];
                }
            }
            for (int c = 0; c < d; c++)
                for (int i = 0; i < d; i++) {
                    double u = i == c ? 1.0 : 0.0;
                    for (int k = 0; k < i; k++) u -= L[i][k] * Li[k][c];
                    Li[i][c] = u / L[i][i];
                }
            double *o = &tab[(size_t)(s * per)];
            for (int k = 0; k < d * d; k++) o[k] = A[k];
            for (int i = 0; i < d; i++)
                for (int j = 0; j < d; j++) {
                    double u = 0.0;
                    for (int k = 0; k < d; k++) u += Li[k][i] * Li[k][j];
                    o[d * d + i * d + j] = u;
                }
            o[2 * d * d] = ld;
        }
        // the factors' offsets by pair row (cx_set_factor_offsets); none while every offset is zero: the kernels then run as without them
        if (h->offsets_nonzero) {
            std::vector<double> pb((size_t)C.n_pair * d);
            for (int64_t r = 0; r < C.n_pair; r++) std::copy_n(&h->offsets[(size_t)C.pair_fac[(size_t)r] * d], d, &pb[(size_t)r * d]);
            if ((rc = dev_upload(h, &C.d_pb, pb)) != CX_OK) return rc;
            CX_HIP(h, hipStreamSynchronize(h->stream));      // (pb dies here)
        } else C.d_pb.reset();
        if ((rc = C.d_ptab.ensure(h, (int64_t)tab.size())) != CX_OK) return rc;
        CX_HIP(h, hipMemcpyAsync(C.d_ptab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, h->stream));
        if ((rc = dev_upload(h, &C.d_kps, kps)) != CX_OK) return rc;
        CX_HIP(h, hipStreamSynchronize(h->stream));
    }
    C.epoch = h->param_epoch;
    return CX_OK;
}

template <int D>
void launch_var(cx_handle *h, Cache &C) {
    const int64_t nb_v = (h->nv + kB - 1) / kB;
    if (nb_v)
        hipLaunchKernelGGL(k_ev_var<D>, dim3((unsigned)nb_v), dim3(kB), 0, h->stream, h->nv, h->d_vbase, h->d_var_deg, h->d_vinfo, C.d_vrec,
                           C.d_tail, h->big_start, f2v_of(h), C.d_W, C.d_partial);
}

void final_sum(cx_handle *h, int64_t n, const Part *partial, double *out) { hipLaunchKernelGGL(k_ev_final, dim3(1), dim3(kFB), 0, h->stream, n, partial, out); }

void var_pass(cx_handle *h, Cache &C) { with_dim(h->cfg.dim, [&](auto D) { launch_var<D()>(h, C); }); }

template <int D>
void launch(cx_handle *h, Cache &C) {
    const int64_t nb_v = (h->nv + kB - 1) / kB, nb_p = (C.n_pair + kB - 1) / kB, nb_k = (C.n_kary + kKB - 1) / kKB;
    Part *part = C.d_partial;
    const Msgs msg = msgs_of(h, C);
    launch_var<D>(h, C);
    if (nb_p) hipLaunchKernelGGL(k_ev_pair<D>, dim3((unsigned)nb_p), dim3(kB), 0, h->stream, C.n_pair, C.pair_tab(), msg, part + nb_v);
    if (nb_k) hipLaunchKernelGGL(k_ev_kary<D>, dim3((unsigned)nb_k), dim3(kKB), 0, h->stream, C.n_kary, C.kary_tab(), msg, part + nb_v + nb_p);
    final_sum(h, C.nb, part, C.d_out);
}

// ---- the per-component sum of a term array: shared with cx_log_evidence_components_mfma (cx_evidence_mfma.hip) ----------
int32_t plan_components(cx_handle *h, CompPlan &P, int64_t n_comp, const std::vector<int32_t> &term_label, const std::string &who) {
    using namespace cxh;
    CX_REQUIRE(h, (int64_t)term_label.size() < (int64_t)0x3fffffff, CX_ERR_UNSUPPORTED, who + ": more than 2^30 terms");
    std::vector<int32_t> perm, key, span;
    std::vector<int64_t> beg, end;
    P.n_comp = n_comp;
    P.n_pos = comp::sort_terms(n_comp, term_label, kTile, kSI, perm, key, beg, end);
    for (int64_t k = 0; k < n_comp; k++)
        if (end[(size_t)k] - beg[(size_t)k] > kTile) span.push_back((int32_t)k);
    P.n_tile = (P.n_pos + kTile - 1) / kTile; P.n_span = (int64_t)span.size();
    P.h_cout.assign((size_t)(n_comp * (1 + kNCnt)), 0.0);
    int32_t rc;
    if ((rc = dev_upload(h, &P.d_perm, perm)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &P.d_key, key)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &P.d_sbeg, beg)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &P.d_send, end)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &P.d_span, span)) != CX_OK) return rc;
    if ((rc = dev_alloc(h, &P.d_tpart, P.n_tile)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &P.d_cout, P.h_cout)) != CX_OK) return rc;      // (zeros: a component without a term is never written)
    CX_HIP(h, hipStreamSynchronize(h->stream));      // (the local host vectors die here)
    return CX_OK;
}

void reduce_components(cx_handle *h, const CompPlan &P, const double *tval, const uint8_t *tflag) {
    double *cval = P.d_cout;
    unsigned long long *ccnt = reinterpret_cast<unsigned long long *>(cval + P.n_comp);
    if (P.n_tile)
        k_ev_seg<<<dim3((unsigned)P.n_tile), dim3(kSB), 0, h->stream>>>(P.n_pos, P.d_perm, P.d_key, P.d_sbeg, P.d_send, tval, tflag, P.d_tpart, cval, ccnt);
    if (P.n_span)
        k_ev_span<<<dim3((unsigned)((P.n_span + kSB / 64 - 1) / (kSB / 64))), dim3(kSB), 0, h->stream>>>(P.n_span, P.d_span, P.d_sbeg, P.d_send, P.d_tpart, cval, ccnt);
}

int32_t read_components(cx_handle *h, CompPlan &P, const std::string &who, int64_t n_fac_terms, const std::vector<int64_t> &comp_fac_terms, int64_t cap,
                        double *values, int64_t *comp_counts4, int64_t *n_components, int64_t *counts4) {
    using namespace cxh;
    CX_HIP(h, hipGetLastError());
    const int64_t nc = P.n_comp;
    if (nc) CX_HIP(h, hipMemcpyAsync(P.h_cout.data(), P.d_cout, (size_t)(nc * (1 + kNCnt)) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    CX_HIP(h, hipStreamSynchronize(h->stream));
    // the whole graph's counters are the sums of the components'
    const double *val = P.h_cout.data();
    const uint64_t *cnt = reinterpret_cast<const uint64_t *>(val + nc);
    uint64_t tot[kNCnt] = {0, 0, 0, 0};
    for (int64_t k = 0; k < nc; k++)
        for (int q = 0; q < kNCnt; q++) tot[q] += cnt[k * kNCnt + q];
    CX_REQUIRE(h, tot[3] == 0, CX_ERR_UNSUPPORTED, who + ": the graph holds stand-in variables of a partition");
    counts4[0] = n_fac_terms;
    for (int q = 1; q < 4; q++) counts4[q] = (int64_t)tot[q - 1];
    *n_components = nc;
    for (int64_t k = 0; k < std::min(cap, nc); k++) {
        const uint64_t *c = cnt + k * kNCnt;
        values[k] = c[1] + c[2] > 0 ? kNaN : val[k];
        if (comp_counts4) {
            comp_counts4[4 * k] = comp_fac_terms[(size_t)k];
            for (int q = 1; q < 4; q++) comp_counts4[4 * k + q] = (int64_t)c[q - 1];
        }
    }
    return CX_OK;
}

// the plan of cx_log_evidence_components: the labels, the terms sorted by (component, term index) into aligned positions, every
// component's first and last position, the components of more than a tile (plan_components), and the call's scratch
int32_t build_components(cx_handle *h, Cache &C, const std::string &who) {
    using namespace cxh;
    const int64_t nv = h->nv, nf = h->nf, ne = h->ne, nt = nv + C.n_pair + C.n_kary;
    std::vector<int32_t> efac((size_t)ne);
    for (int64_t e = 0; e < ne; e++) efac[(size_t)e] = (int32_t)find_factor(h, h->edge_fac_id[(size_t)e]);
    const int64_t n_comp = comp::label(nv, nf, ne, h->edge_var.data(), efac.data(), C.var_label, C.fac_label);
    std::vector<int32_t> term_label((size_t)nt);
    std::copy(C.var_label.begin(), C.var_label.end(), term_label.begin());
    C.comp_fac_terms.assign((size_t)n_comp, 0);
    for (int64_t f = 0; f < nf; f++) {
        const int32_t rp = C.row_of_fac[(size_t)f], rk = C.kary_row_of_fac[(size_t)f];
        if (rp < 0 && rk < 0) continue;
        term_label[(size_t)(rp >= 0 ? nv + rp : nv + C.n_pair + rk)] = C.fac_label[(size_t)f];
        C.comp_fac_terms[(size_t)C.fac_label[(size_t)f]]++;
    }
    int32_t rc;
    if ((rc = plan_components(h, C.comp, n_comp, term_label, who)) != CX_OK) return rc;
    if ((rc = dev_alloc(h, &C.d_tval, nt)) != CX_OK) return rc;
    if ((rc = dev_alloc(h, &C.d_tflag, nt)) != CX_OK) return rc;
    C.n_term = nt;
    C.comp_built = true;
    return CX_OK;
}

template <int D>
void launch_components(cx_handle *h, Cache &C) {
    const int64_t nv = h->nv, nb_v = (nv + kB - 1) / kB, nb_p = (C.n_pair + kB - 1) / kB, nb_k = (C.n_kary + kKB - 1) / kKB;
    const Msgs msg = msgs_of(h, C);
    double *tv = C.d_tval;
    uint8_t *tf = C.d_tflag;
    if (nb_v)
        k_ev_var<D, true><<<dim3((unsigned)nb_v), dim3(kB), 0, h->stream>>>(nv, h->d_vbase, h->d_var_deg, h->d_vinfo, C.d_vrec, C.d_tail, h->big_start,
                                                                           f2v_of(h), C.d_W, TermOut{tv, tf});
    if (nb_p) k_ev_pair<D, true><<<dim3((unsigned)nb_p), dim3(kB), 0, h->stream>>>(C.n_pair, C.pair_tab(), msg, TermOut{tv + nv, tf + nv});
    if (nb_k)
        k_ev_kary<D, true><<<dim3((unsigned)nb_k), dim3(kKB), 0, h->stream>>>(C.n_kary, C.kary_tab(), msg, TermOut{tv + nv + C.n_pair, tf + nv + C.n_pair});
    reduce_components(h, C.comp, C.d_tval, C.d_tflag);
}

}  // namespace ev

template <> void Deleter<ev::Cache>::operator()(ev::Cache *C) const { delete C; }

int32_t ev::prepare(cx_handle *h, const std::string &who, const char *bad_args, ev::Cache *&Cp, const char *family_note) {
    using namespace cxh;
    CX_REQUIRE(h, !h || h->cfg.family == CX_FAMILY_GAUSSIAN, CX_ERR_UNSUPPORTED, who + ": the Gaussian family only" + family_note);
    CX_REQUIRE(h, h && h->has_graph, CX_ERR_STATE, who + ": no graph");
    CX_REQUIRE(h, !bad_args, CX_ERR_INVALID_ARGUMENT, who + ": " + bad_args);
    CX_REQUIRE(h, h->cfg.dim >= 1 && h->cfg.dim <= 4 && !h->user_dim, CX_ERR_UNSUPPORTED, who + ": dim 1, 2, 3 and 4 (the matrix-core dims are not implemented)");
    CX_REQUIRE(h, !h->chain_partition && !h->halo_state && h->send_slots.empty() && h->recv_slots.empty(), CX_ERR_UNSUPPORTED,
               who + ": not for a partitioned handle (halo lists or stand-in variables: its terms would need owners)");
    CX_HIP(h, hipSetDevice(h->cfg.device));
    if (h->stream) {
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        CX_HIP(h, hipStreamIsCapturing(h->stream, &st));
        CX_REQUIRE(h, st == hipStreamCaptureStatusNone, CX_ERR_STATE, who + ": the handle's stream is being captured (the call is synchronous)");
    }
    if (!h->evidence) h->evidence.reset(new ev::Cache());
    ev::Cache &C = *h->evidence;
    int32_t rc;
    if (!C.built && (rc = ev::build(h, C, who)) != CX_OK) { h->evidence.reset(); return rc; }
    if (C.unsupported_fac >= 0)
        return fail(h, CX_ERR_UNSUPPORTED, who + ": factor " + std::to_string(C.unsupported_fac) + " has no sum-product rule (Gaussian factors and opaque messages only)");
    if (C.zero_noise_fac >= 0)
        return fail(h, CX_ERR_UNSUPPORTED, who + ": factor " + std::to_string(C.zero_noise_fac) + " has zero noise (q = 0): its density is degenerate");
    if ((rc = ev::refresh_params(h, C, who)) != CX_OK) return rc;
    if (h->cfg.dim > 1 && (rc = mv_ensure_chain_msgs(h)) != CX_OK) return rc;      // (chain scan, dim 2..4: the messages go to their slots on demand)
    Cp = &C;
    return CX_OK;
}

}  // namespace cx

using namespace cxh;

extern "C" int32_t cx_log_evidence(cx_handle *h, double *value, int64_t *counts4) {
    try {
        cx::ev::Cache *Cp = nullptr;
        int32_t rc;
        if ((rc = cx::ev::prepare(h, "cx_log_evidence", value && counts4 ? nullptr : "null argument", Cp,
                                  " (no variational free energy, no Beta-Bernoulli evidence)")) != CX_OK) return rc;
        cx::ev::Cache &C = *Cp;
        cx::ev::with_dim(h->cfg.dim, [&](auto D) { cx::ev::launch<D()>(h, C); });
        CX_HIP(h, hipGetLastError());
        CX_HIP(h, hipMemcpyAsync(C.h_out, C.d_out, (1 + cx::ev::kNCnt) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        CX_HIP(h, hipStreamSynchronize(h->stream));
        uint64_t cnt[cx::ev::kNCnt];
        std::memcpy(cnt, C.h_out + 1, sizeof(cnt));
        CX_REQUIRE(h, cnt[3] == 0, CX_ERR_UNSUPPORTED, "cx_log_evidence: the graph holds stand-in variables of a partition");
        counts4[0] = C.n_pair + C.n_kary;
        for (int k = 1; k < 4; k++) counts4[k] = (int64_t)cnt[k - 1];
        *value = counts4[2] + counts4[3] > 0 ? kNaN : C.h_out[0];
        return CX_OK;
    } catch (const std::bad_alloc &) { return fail(h, CX_ERR_OUT_OF_MEMORY, "cx_log_evidence: host allocation failed"); }
}

extern "C" int32_t cx_graph_components(cx_handle *h, int64_t n, const int64_t *variable_ids, int64_t *component, int64_t *n_components) {
    try {
        CX_NOT_VMP(h, "cx_graph_components");
        CX_REQUIRE(h, h && h->has_graph, CX_ERR_STATE, "cx_graph_components: no graph");
        CX_REQUIRE(h, n_components && (!variable_ids || n >= 0), CX_ERR_INVALID_ARGUMENT, "cx_graph_components: null n_components or n < 0");
        // (the named variables are looked up first: a refused call writes nothing)
        std::vector<int64_t> idx;
        if (variable_ids && component)
            for (int64_t i = 0; i < n; i++) {
                const int64_t v = find_var(h, variable_ids[i]);
                if (v < 0) return fail(h, CX_ERR_NOT_FOUND, "cx_graph_components: no variable " + std::to_string(variable_ids[i]));
                idx.push_back(v);
            }
        // the labels of the evidence plan when a component call has built it (a handle has one graph for life), else a union-find now
        std::vector<int32_t> mine, fl;
        const bool planned = h->evidence && h->evidence->comp_built;
        if (planned) *n_components = h->evidence->comp.n_comp;
        else {
            std::vector<int32_t> efac((size_t)h->ne);
            for (int64_t e = 0; e < h->ne; e++) efac[(size_t)e] = (int32_t)find_factor(h, h->edge_fac_id[(size_t)e]);
            *n_components = cx::comp::label(h->nv, h->nf, h->ne, h->edge_var.data(), efac.data(), mine, fl);
        }
        const std::vector<int32_t> &vl = planned ? h->evidence->var_label : mine;
        if (component && variable_ids) for (int64_t i = 0; i < n; i++) component[i] = vl[(size_t)idx[(size_t)i]];
        else if (component) std::copy(vl.begin(), vl.end(), component);
        return CX_OK;
    } catch (const std::bad_alloc &) { return fail(h, CX_ERR_OUT_OF_MEMORY, "cx_graph_components: host allocation failed"); }
}

extern "C" int32_t cx_log_evidence_components(cx_handle *h, int64_t cap, double *values, int64_t *comp_counts4, int64_t *n_components, int64_t *counts4) {
    try {
        namespace ev = cx::ev;
        ev::Cache *Cp = nullptr;
        int32_t rc;
        const char *bad = !n_components || !counts4 ? "null n_components or counts4" : cap < 0 ? "cap < 0" : cap > 0 && !values ? "cap > 0 with null values" : nullptr;
        if ((rc = ev::prepare(h, "cx_log_evidence_components", bad, Cp, " (no variational free energy, no Beta-Bernoulli evidence)")) != CX_OK) return rc;
        ev::Cache &C = *Cp;
        if (!C.comp_built && (rc = ev::build_components(h, C, "cx_log_evidence_components")) != CX_OK) return rc;
        ev::with_dim(h->cfg.dim, [&](auto D) { ev::launch_components<D()>(h, C); });
        return ev::read_components(h, C.comp, "cx_log_evidence_components", C.n_pair + C.n_kary, C.comp_fac_terms, cap, values, comp_counts4, n_components, counts4);
    } catch (const std::bad_alloc &) { return fail(h, CX_ERR_OUT_OF_MEMORY, "cx_log_evidence_components: host allocation failed"); }
}
