// cx_evidence_core.h — what the read-outs of the stored messages share (cx_evidence.hip, cx_learn.hip, cx_sample.hip, cx_predict.hip): the dimension
// dispatch, the per-variable scratch of the variable pass, compensated sums, message loads, the small-matrix kit (Cholesky, triangular
// solves and inverses, in registers and on the packed joint in LDS), the centred leave-one-out message of one factor edge, the belief
// joints of a two-variable and of a k-ary factor, and the cached tables of a handle.  Derivations: DESIGN.md §4e, §4f and §4g.
#pragma once
#include <type_traits>
#include "cx_host.h"
#include "cx_mv_core.h"

namespace cx {
namespace ev {

constexpr int kB = 256;        // threads per block of the variable, pairwise and final passes
constexpr double kLog2Pi = 1.83787706640934548356;

// f(std::integral_constant<int, d>) for d = 1 .. 4 (ev::prepare has refused every other dim): the only switch on the dimension
template <class F>
decltype(auto) with_dim(int d, F &&f) {
    switch (d) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 3: return f(std::integral_constant<int, 3>());
    default: return f(std::integral_constant<int, 4>());
    }
}

template <int D>
struct Lay {
    static constexpr int NT = D * (D + 1) / 2;
    static constexpr int K = D == 1 ? 2 : ((D + NT + 1) + 1) / 2 * 2;      // doubles per variable of the scratch: a[D] | Λ[NT] | flag
};
// a = μ_i when Λ_i is positive definite (flag 1; D = 1: Λ > 0), η_i otherwise (flag 0, centre 0)

// ---- compensated sums -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void neu(double &s, double &c, double x) {
    const double t = s + x;
    c += fabs(s) >= fabs(x) ? (s - t) + x : (x - t) + s;
    s = t;
}

// per block: the compensated sum and the counters of its terms (variable terms, undefined input, not positive definite, stand-ins);
// k_ev_final adds the blocks up in index order: no floating-point atomic, no atomic at all
struct Part {
    double s, c;
    unsigned n[4];
};

// counters read back: 0 variable terms, 1 terms with an undefined input, 2 terms whose belief is not positive definite, 3 stand-in
// variables met (a halo handle: refused); the factor terms are known on the host
constexpr int kNCnt = 4;

// one term of cx_log_evidence_components: its flag bits, in the counters' order
constexpr unsigned kTermVar = 1, kTermUndef = 2, kTermNpd = 4, kTermGhost = 8;
// where the term entry of a pass writes: the term's value (the thread's compensated sum as one double) and flag bits at its term index
struct TermOut {
    double *val;
    uint8_t *flag;
};
// the piece of one component inside one tile of the sorted term list: a compensated sum and the four counters, 16 bits each
struct TilePart {
    double s, c;
    unsigned long long n;
};

// fixed-order tree over the block's threads; thread 0 writes the block's Part
template <int NB>
__device__ __forceinline__ void block_part(double s, double c, unsigned n0, unsigned n1, unsigned n2, unsigned n3, Part *__restrict__ out) {
    __shared__ double ss[NB], cs[NB];
    __shared__ unsigned ns[4][NB];
    const int t = threadIdx.x;
    ss[t] = s; cs[t] = c; ns[0][t] = n0; ns[1][t] = n1; ns[2][t] = n2; ns[3][t] = n3;
    __syncthreads();
#pragma unroll
    for (int w = NB / 2; w > 0; w >>= 1) {
        if (t < w) {
            double a = ss[t], ac = cs[t];
            neu(a, ac, ss[t + w]);
            ss[t] = a; cs[t] = ac + cs[t + w];
#pragma unroll
            for (int k = 0; k < 4; k++) ns[k][t] += ns[k][t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        Part p;
        p.s = ss[0]; p.c = cs[0];
#pragma unroll
        for (int k = 0; k < 4; k++) p.n[k] = ns[k][0];
        out[blockIdx.x] = p;
    }
}

// ---- messages -------------------------------------------------------------------------------------------------------------------
template <int D>
__device__ __forceinline__ void ld_msg(const double *__restrict__ buf, int slot, double (&eta)[D], double (&lam)[Lay<D>::NT]) {
    if constexpr (D == 1) {
        const double2 m = reinterpret_cast<const double2 *>(buf)[slot];
        eta[0] = m.x; lam[0] = m.y;
    } else {
        const Msg<D> m = slot_load<D, false>(buf, slot);
#pragma unroll
        for (int k = 0; k < D; k++) eta[k] = m.eta[k];
#pragma unroll
        for (int k = 0; k < Lay<D>::NT; k++) lam[k] = m.lam[k];
    }
}

template <int D>
__device__ __forceinline__ double lam_at(const double (&lam)[Lay<D>::NT], int i, int j) { return i <= j ? lam[tri<D>(i, j)] : lam[tri<D>(j, i)]; }

// ---- the small-matrix kit ---------------------------------------------------------------------------------------------------------
// Register form (N a template parameter, every loop unrolled) and accessor form (n at run time, the matrix behind at(i, j) -> double &
// with i >= j, vectors behind y(i) -> double &: the packed joint in LDS).  Same operations in the same order in both.
#define CX_LA __host__ __device__ __forceinline__

// A = L L' in place (the lower triangle is read and written); logdet, if given, gains log det A.  false: not positive definite
template <int N>
CX_LA bool chol(double (&A)[N][N], double *logdet = nullptr) {
#pragma unroll
    for (int j = 0; j < N; j++) {
        double d = A[j][j];
#pragma unroll
        for (int k = 0; k < j; k++) d -= A[j][k] * A[j][k];
        if (!(d > 0.0)) return false;
        if (logdet) *logdet += log(d);
        const double l = sqrt(d), il = 1.0 / l;
        A[j][j] = l;
#pragma unroll
        for (int i = j + 1; i < N; i++) {
            double s = A[i][j];
#pragma unroll
            for (int k = 0; k < j; k++) s -= A[i][k] * A[j][k];
            A[i][j] = s * il;
        }
    }
    return true;
}

// y <- L⁻¹ y
template <int N>
CX_LA void fwd_solve(const double (&L)[N][N], double (&y)[N]) {
#pragma unroll
    for (int i = 0; i < N; i++) {
        double s = y[i];
#pragma unroll
        for (int k = 0; k < i; k++) s -= L[i][k] * y[k];
        y[i] = s / L[i][i];
    }
}

// x = L⁻ᵀ y
template <int N>
CX_LA void back_solve(const double (&L)[N][N], const double (&y)[N], double (&x)[N]) {
#pragma unroll
    for (int i = N - 1; i >= 0; i--) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < N; k++) s -= L[k][i] * x[k];
        x[i] = s / L[i][i];
    }
}

// J = L L' in place, h <- L⁻¹ h: log det J and h'J⁻¹h.  false: not positive definite
template <int N>
CX_LA bool chol_quad(double (&J)[N][N], double (&h)[N], double &logdet, double &quad) {
    logdet = 0.0; quad = 0.0;
    if (!chol<N>(J, &logdet)) return false;
    fwd_solve<N>(J, h);
#pragma unroll
    for (int i = 0; i < N; i++) quad += h[i] * h[i];
    return true;
}

// x = (L L')⁻¹ b
template <int N>
CX_LA void chol_solve(const double (&L)[N][N], const double (&b)[N], double (&x)[N]) {
    double y[N];
#pragma unroll
    for (int i = 0; i < N; i++) y[i] = b[i];
    fwd_solve<N>(L, y);
    back_solve<N>(L, y, x);
}

// The two inverses reach L⁻¹ by different orders of operations and differ in the last bits: each caller keeps the one it was checked with.
// L <- L⁻¹ in place, row by row (row i reads L's row i to the right of the entry it writes, and the rows of L⁻¹ above it)
template <int N>
CX_LA void inv_lower(double (&L)[N][N]) {
#pragma unroll
    for (int i = 0; i < N; i++) {
#pragma unroll
        for (int j = 0; j < i; j++) {
            double s = 0.0;
#pragma unroll
            for (int k = j; k < i; k++) s += L[i][k] * L[k][j];
            L[i][j] = -s / L[i][i];
        }
        L[i][i] = 1.0 / L[i][i];
    }
}

// the lower triangle of S = Li' Li for a lower Li: (L L')⁻¹ from inv_lower's L⁻¹
template <int N>
CX_LA void gram_lower(const double (&Li)[N][N], double (&S)[N][N]) {
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = 0; j <= i; j++) {
            double s = 0.0;
#pragma unroll
            for (int k = i; k < N; k++) s += Li[k][i] * Li[k][j];
            S[i][j] = s;
        }
}

// M = L⁻ᵀ (upper), by a forward solve per unit vector: row r of M = column r of L⁻¹
template <int N>
CX_LA void inv_t(const double (&L)[N][N], double (&M)[N][N]) {
#pragma unroll
    for (int r = 0; r < N; r++) {
        double y[N];
#pragma unroll
        for (int c = 0; c < N; c++) {
            double s = c == r ? 1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < c; k++) s -= L[c][k] * y[k];
            y[c] = c < r ? 0.0 : s / L[c][c];
        }
#pragma unroll
        for (int c = 0; c < N; c++) M[r][c] = y[c];
    }
}

// the same on a matrix behind at(i, j)
template <class At>
CX_LA bool chol_at(int n, At at, double *logdet = nullptr) {
    for (int j = 0; j < n; j++) {
        double d = at(j, j);
        for (int k = 0; k < j; k++) { const double l = at(j, k); d -= l * l; }
        if (!(d > 0.0)) return false;
        if (logdet) *logdet += log(d);
        const double l = sqrt(d), il = 1.0 / l;
        at(j, j) = l;
        for (int i = j + 1; i < n; i++) {
            double u = at(i, j);
            for (int k = 0; k < j; k++) u -= at(i, k) * at(j, k);
            at(i, j) = u * il;
        }
    }
    return true;
}

// y <- L⁻¹ y
template <class At, class Y>
CX_LA void fwd_solve_at(int n, At at, Y y) {
    for (int i = 0; i < n; i++) {
        double u = y(i);
        for (int k = 0; k < i; k++) u -= at(i, k) * y(k);
        y(i) = u / at(i, i);
    }
}

// y <- L⁻ᵀ y
template <class At, class Y>
CX_LA void back_solve_at(int n, At at, Y y) {
    for (int i = n - 1; i >= 0; i--) {
        double u = y(i);
        for (int k = i + 1; k < n; k++) u -= at(k, i) * y(k);
        y(i) = u / at(i, i);
    }
}

// y <- (L L')⁻¹ y
template <class At, class Y>
CX_LA void chol_solve_at(int n, At at, Y y) {
    fwd_solve_at(n, at, y);
    back_solve_at(n, at, y);
}
#undef CX_LA

// ---- pass 2 helpers -------------------------------------------------------------------------------------------------------------
// one non-observed edge of a factor: the centred leave-one-out message m~_{i→a} (η~, Λ~) and the centre μ_i
template <int D>
__device__ __forceinline__ bool free_edge(const double *__restrict__ f2v, const double *__restrict__ W, int slot, int var, double (&mu)[D],
                                          double (&et)[D], double (&lm)[Lay<D>::NT]) {
    constexpr int NT = Lay<D>::NT, K = Lay<D>::K;
    double e[D], l[NT];
    ld_msg<D>(f2v, slot, e, l);
    const double *w = W + (int64_t)var * K;
    double a[D], L[NT];
#pragma unroll
    for (int i = 0; i < D; i++) a[i] = w[i];
#pragma unroll
    for (int i = 0; i < NT; i++) L[i] = w[D + i];
    const bool pd = D == 1 ? L[0] > 0.0 : w[D + NT] != 0.0;
    bool undef = false;
#pragma unroll
    for (int i = 0; i < D; i++) {
        mu[i] = pd ? a[i] : 0.0;
        undef = undef || __builtin_isnan(a[i]) || __builtin_isnan(e[i]);
    }
#pragma unroll
    for (int i = 0; i < NT; i++) { lm[i] = L[i] - l[i]; undef = undef || __builtin_isnan(L[i]) || __builtin_isnan(l[i]); }
#pragma unroll
    for (int i = 0; i < D; i++) {
        double t = e[i];
#pragma unroll
        for (int j = 0; j < D; j++) t -= lam_at<D>(l, i, j) * mu[j];
        et[i] = (pd ? 0.0 : a[i]) - t;
    }
    return !undef;
}

template <int D>
__device__ __forceinline__ void datum(const double *__restrict__ v2f, int slot, double (&y)[D]) {
    double l[Lay<D>::NT];
    ld_msg<D>(v2f, slot, y, l);
}

// ---- the tables and the messages, as the kernels take them (filled by Cache::pair_tab / kary_tab and msgs_of) --------------------------
// pair row p: rec[p] = (slot out, slot in, var out, var in) of x_out = A x_in + b + N(0, Q).  dim 1: (q, a, b) per row (pa, pb may be
// null: a = 1, b = 0); dim > 1: the row's parameter set pset[p] in ptab = [set][A | Q⁻¹ | log det 2πQ, 0] and its offset pb[p * d ..)
// (cx_set_factor_offsets; pb null: b = 0)
struct PairTab {
    const int4 *rec;
    const int32_t *pset;
    const double *pq, *pa, *pb, *ptab;
};
// k-ary row f: x_out = Σ A_k x_k + b + N(0, Q), entries in the k-ary table's order (OUT first).  krec[f] = slots[8] | vars[8] (-1: none).
// dim 1: kc[f] = C_e[8] (+1 OUT, -a_i IN) | q | b.  dim > 1: kps[f] = parameter set per entry (IN: its A; OUT: Q); ptab as PairTab's
struct KaryTab {
    const int32_t *krec;
    const double *kc;
    const int32_t *kps;
    const double *ptab;
};
// the observed flags, the stored messages of both directions and the scratch of the variable pass
struct Msgs {
    const uint8_t *vinfo;
    const double *f2v, *v2f, *W;
};

// ---- the belief of pair row p, centred on its ends' centres c (a free end: its belief mean, free_edge; an observed end: its datum):
// precision J and right-hand side h over (out, in), 2d x 2d, with rc = c_out - A c_in - b, g = -Q⁻¹ rc and η~, Λ~ the centred
// leave-one-out messages of the free ends.  An observed end (fo / fi false) is an identity block with h = 0, so the D x D block of
// the free end of a factor with one observed end is that factor's whole joint.  ok: every input is defined.
template <int D>
struct PairJoint {
    bool fo, fi, ok;
    double A[D][D], c[2 * D], rc[D], g[D], ldq;      // ldq = log det 2πQ
    double J[2 * D][2 * D], h[2 * D];
};

template <int D>
__device__ __forceinline__ void pair_joint(int64_t p, const PairTab &T, const Msgs &M, PairJoint<D> &B) {
    constexpr int NT = Lay<D>::NT;
    double (&A)[D][D] = B.A;
    double Qi[D][D], bb[D];
    if constexpr (D == 1) {
        const double q = T.pq[p];
        A[0][0] = T.pa ? T.pa[p] : 1.0; Qi[0][0] = 1.0 / q; B.ldq = log(q) + kLog2Pi; bb[0] = T.pb ? T.pb[p] : 0.0;
    } else {
        const double *t = T.ptab + (int64_t)T.pset[p] * (2 * D * D + 2);
#pragma unroll
        for (int i = 0; i < D; i++) {
            bb[i] = T.pb ? T.pb[p * D + i] : 0.0;      // (cx_set_factor_offsets; null: no offset is non-zero)
#pragma unroll
            for (int j = 0; j < D; j++) { A[i][j] = t[i * D + j]; Qi[i][j] = t[D * D + i * D + j]; }
        }
        B.ldq = t[2 * D * D];
    }
    const int4 r = T.rec[p];
    const bool fo = B.fo = !(M.vinfo[r.z] & kClamped), fi = B.fi = !(M.vinfo[r.w] & kClamped);
    double mo[D], eo[D], lo[NT], mi[D], ei[D], li[NT];
    B.ok = true;
    if (fo) B.ok = free_edge<D>(M.f2v, M.W, r.x, r.z, mo, eo, lo) && B.ok;
    else datum<D>(M.v2f, r.x, mo);
    if (fi) B.ok = free_edge<D>(M.f2v, M.W, r.y, r.w, mi, ei, li) && B.ok;
    else datum<D>(M.v2f, r.y, mi);
    double T_[D][D];       // Q⁻¹ A
#pragma unroll
    for (int i = 0; i < D; i++) {
        B.c[i] = mo[i]; B.c[D + i] = mi[i];
        double t = mo[i] - bb[i];
#pragma unroll
        for (int j = 0; j < D; j++) t -= A[i][j] * mi[j];
        B.rc[i] = t;
    }
#pragma unroll
    for (int i = 0; i < D; i++) {
        double t = 0.0;
#pragma unroll
        for (int j = 0; j < D; j++) t -= Qi[i][j] * B.rc[j];
        B.g[i] = t;
#pragma unroll
        for (int j = 0; j < D; j++) {
            double u = 0.0;
#pragma unroll
            for (int k = 0; k < D; k++) u += Qi[i][k] * A[k][j];
            T_[i][j] = u;
        }
    }
#pragma unroll
    for (int i = 0; i < D; i++) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < D; k++) t += A[k][i] * B.g[k];
        B.h[i] = fo ? B.g[i] + eo[i] : 0.0;
        B.h[D + i] = fi ? -t + ei[i] : 0.0;
#pragma unroll
        for (int j = 0; j < D; j++) {
            double u = 0.0;
#pragma unroll
            for (int k = 0; k < D; k++) u += A[k][i] * T_[k][j];
            B.J[i][j] = fo ? Qi[i][j] + lam_at<D>(lo, i, j) : (i == j ? 1.0 : 0.0);
            B.J[D + i][D + j] = fi ? u + lam_at<D>(li, i, j) : (i == j ? 1.0 : 0.0);
            B.J[D + i][j] = fo && fi ? -T_[j][i] : 0.0;
            B.J[j][D + i] = B.J[D + i][j];
        }
    }
}

// ---- the joint of a factor of 3 .. 7 variables (k-ary table row f), shared by k_ev_kary and the sampler's k_sp_cond_kary -----------
// Writes the joint precision over the free entries (packed lower triangle, element k at J[k * NB]) and its right-hand side (hv), in
// coordinates centred on the free entries' belief means; returns Q⁻¹, log det 2πQ, b'' = b - Σ C_e x_e at the data / the centres,
// g = Q⁻¹ b'', cq = b'' g, the mask and count of the free entries and whether every input is defined.
template <int D>
struct KLay {
    static constexpr int NM = 7 * D, NP = NM * (NM + 1) / 2;
};
__device__ __forceinline__ int pk(int i, int j) { return i * (i + 1) / 2 + j; }      // i >= j

template <int D>
__device__ __forceinline__ double cel(const double *__restrict__ Ae, double ce, int p, int q) {      // C_e[p][q]
    if constexpr (D == 1) return ce;
    else return Ae ? -Ae[p * D + q] : (p == q ? 1.0 : 0.0);
}

template <int D, int NB>
__device__ __forceinline__ void kary_joint(int64_t f, const KaryTab &T, const Msgs &M, double *__restrict__ J, double *__restrict__ hv,
                                           double (&Qi)[D][D], double &ldq, double (&bp)[D], double (&g)[D], double &cq, unsigned &freemask, int &nfree,
                                           bool &ok) {
    constexpr int NT = Lay<D>::NT, PS = 2 * D * D + 2;
    const int32_t *sl = T.krec + f * 16, *vr = sl + 8;
    // C_e of entry e: dim 1 the coefficient, dim > 1 I (OUT) or -A of the entry's set (read where used: no per-thread arrays)
    auto Aof = [&](int e) -> const double * {
        if constexpr (D == 1) return nullptr;
        else return e == 0 ? nullptr : T.ptab + (int64_t)T.kps[f * 8 + e] * PS;
    };
    auto Cof = [&](int e) -> double {
        if constexpr (D == 1) return T.kc[f * 10 + e];
        else return 0.0;
    };
    if constexpr (D == 1) {
        const double *k = T.kc + f * 10;
        Qi[0][0] = 1.0 / k[8]; ldq = log(k[8]) + kLog2Pi; bp[0] = k[9];
    } else {
        const double *tq = T.ptab + (int64_t)T.kps[f * 8] * PS;
#pragma unroll
        for (int p = 0; p < D; p++) {
            bp[p] = 0.0;
#pragma unroll
            for (int q = 0; q < D; q++) Qi[p][q] = tq[D * D + p * D + q];
        }
        ldq = tq[2 * D * D];
    }
    freemask = 0;
    nfree = 0;
    ok = true;
    for (int e = 0; e < 8; e++) {
        if (sl[e] < 0) continue;
        double x[D];
        if (M.vinfo[vr[e]] & kClamped) datum<D>(M.v2f, sl[e], x);
        else {
            double et[D], lm[NT];
            ok = free_edge<D>(M.f2v, M.W, sl[e], vr[e], x, et, lm) && ok;
            const int o = nfree * D;
            for (int r = 0; r < D; r++) {
                hv[(o + r) * NB] = et[r];
                for (int q = 0; q <= r; q++) J[pk(o + r, o + q) * NB] = lam_at<D>(lm, r, q);
                for (int j = 0; j < o; j++) J[pk(o + r, j) * NB] = 0.0;
            }
            freemask |= 1u << e;
            nfree++;
        }
        // b'' -= C_e x
#pragma unroll
        for (int p = 0; p < D; p++) {
            double u = 0.0;
#pragma unroll
            for (int q = 0; q < D; q++) u += cel<D>(Aof(e), Cof(e), p, q) * x[q];
            bp[p] -= u;
        }
    }
    cq = 0.0;
#pragma unroll
    for (int p = 0; p < D; p++) {
        double u = 0.0;
#pragma unroll
        for (int q = 0; q < D; q++) u += Qi[p][q] * bp[q];
        g[p] = u; cq += bp[p] * u;
    }
    // J += C_u' Q⁻¹ C_u, h += C_u' Q⁻¹ b''
    int jk = 0;
    for (int k = 0; k < 8; k++) {
        if (!((freemask >> k) & 1)) continue;
        double G[D][D];          // Q⁻¹ C_k
#pragma unroll
        for (int p = 0; p < D; p++)
#pragma unroll
            for (int q = 0; q < D; q++) {
                double u = 0.0;
#pragma unroll
                for (int m = 0; m < D; m++) u += Qi[p][m] * cel<D>(Aof(k), Cof(k), m, q);
                G[p][q] = u;
            }
#pragma unroll
        for (int r = 0; r < D; r++) {
            double u = 0.0;
#pragma unroll
            for (int p = 0; p < D; p++) u += cel<D>(Aof(k), Cof(k), p, r) * g[p];
            hv[(jk * D + r) * NB] += u;
        }
        int jj = 0;
        for (int j = 0; j <= k; j++) {
            if (!((freemask >> j) & 1)) continue;
            // block (k, j) of the lower triangle: C_k' Q⁻¹ C_j = G_k'... written as rows of k, columns of j
            for (int r = 0; r < D; r++)
                for (int q = 0; q < D; q++) {
                    if (jj == jk && q > r) continue;
                    double u = 0.0;
#pragma unroll
                    for (int p = 0; p < D; p++) u += cel<D>(Aof(j), Cof(j), p, q) * G[p][r];      // (C_j' Q⁻¹ C_k)[q][r] = (C_k' Q⁻¹ C_j)[r][q]
                    J[pk(jk * D + r, jj * D + q) * NB] += u;
                }
            jj++;
        }
        jk++;
    }
}

// ---- host: the per-component sum of a term array (cx_log_evidence_components, cx_log_evidence_components_mfma) ----------------------
// The terms sorted by (component, term index) into the aligned positions of comp::sort_terms, and the scratch and output of the
// segmented sum over them (k_ev_seg, k_ev_span: cx_evidence.hip).  Whose terms they are is the owner's business
struct CompPlan {
    int64_t n_comp = 0, n_pos = 0, n_tile = 0, n_span = 0;
    DevBuf<int32_t> d_perm, d_key;        // [n_pos] the term at every position and its component (-1: none; comp::sort_terms)
    DevBuf<int64_t> d_sbeg, d_send;       // [C] first position of every component and the one past its last
    DevBuf<int32_t> d_span;               // [n_span] the components of more than a tile of terms
    DevBuf<TilePart> d_tpart;             // [n_tile] the piece of the long component that reaches the tile
    DevBuf<double> d_cout;                // [C] values | [C][kNCnt] counters (u64)
    std::vector<double> h_cout;
};
// the plan of n_comp components from the component of every term (the terms keep their indices); `who` prefixes the error texts
int32_t plan_components(cx_handle *h, CompPlan &P, int64_t n_comp, const std::vector<int32_t> &term_label, const std::string &who);
// k_ev_seg, then k_ev_span for the components longer than a tile, on the handle's stream: tval / tflag [terms] -> P.d_cout.  The one
// launch site of the two kernels
void reduce_components(cx_handle *h, const CompPlan &P, const double *tval, const uint8_t *tflag);
// The tail of a component call: P.d_cout to the host in one copy, the stream waited for; counts4 = {n_fac_terms, the column sums of the
// components' counters}, *n_components, and for k < min(cap, C): values[k] (NaN when the component has an undefined or not positive
// definite term) and comp_counts4[4 k ..] = {comp_fac_terms[k], its three counters}
int32_t read_components(cx_handle *h, CompPlan &P, const std::string &who, int64_t n_fac_terms, const std::vector<int64_t> &comp_fac_terms, int64_t cap,
                        double *values, int64_t *comp_counts4, int64_t *n_components, int64_t *counts4);

// ---- host: the work lists -------------------------------------------------------------------------------------------------------
struct Cache {
    bool built = false;
    uint64_t epoch = ~0ull;
    int64_t zero_noise_fac = -1;          // a factor with q = 0 (dim 1): refused
    int64_t unsupported_fac = -1;         // a factor of a kind without a sum-product rule
    int64_t n_pair = 0, n_kary = 0, nb = 0;
    DevBuf<int32_t> d_vrec;
    DevBuf<uint8_t> d_tail;
    DevBuf<int4> d_pair;
    DevBuf<int32_t> d_pair_ps, d_krec, d_kps;
    DevBuf<double> d_pq, d_pa, d_pb, d_kc, d_ptab;
    std::vector<int4> pair;               // the pair rows (d_pair) and the k-ary rows (d_krec) as uploaded
    std::vector<int32_t> krec;
    std::vector<int32_t> pair_ps;         // dim > 1: parameter set per pair (what the table must hold)
    std::vector<int64_t> pair_fac;        // factor index of every pair row (rows in factor order)
    std::vector<int32_t> row_of_fac, kary_row_of_fac;      // pair row / k-ary row of every factor index (-1: none)
    DevBuf<double> d_W;
    DevBuf<Part> d_partial;
    DevBuf<double> d_out;
    double *h_out = nullptr;              // value | counters, pinned
    // cx_log_evidence_components: the plan of the first component call, dropped with the cache.  Terms: index v for
    // variable v, nv + pair row, nv + n_pair + k-ary row; sorted by (component, term index) into aligned positions
    bool comp_built = false;
    int64_t n_term = 0;
    std::vector<int32_t> var_label, fac_label;      // component of every variable / factor index
    std::vector<int64_t> comp_fac_terms;            // [C] the factor terms of every component
    CompPlan comp;
    DevBuf<double> d_tval;                // [n_term] the terms
    DevBuf<uint8_t> d_tflag;              // [n_term] their flag bits (kTermVar ..)
    Cache() = default;
    Cache(const Cache &) = delete;
    ~Cache() { if (h_out) (void)hipHostFree(h_out); }
    PairTab pair_tab() const { return {d_pair, d_pair_ps, d_pq, d_pa, d_pb, d_ptab}; }
    KaryTab kary_tab() const { return {d_krec, d_kc, d_kps, d_ptab}; }
};

// the checks every evidence-type call makes, in this order: family (its text ends in family_note), graph, the entry's own arguments
// (bad_args: what is wrong with them, null: nothing), dim, partitions, captured stream, rule kinds, zero noise; then the work lists,
// the parameter table and (chain scan, dim 2..4) the messages in their slots.  `who` prefixes every error text
int32_t prepare(cx_handle *h, const std::string &who, const char *bad_args, Cache *&C, const char *family_note = "");
// pass 1 only (k_ev_var) on the handle's stream: the per-variable scratch C.d_W; the handle's stored f2v messages
void var_pass(cx_handle *h, Cache &C);
// k_ev_final on the handle's stream: the n block partials in index order -> out = value | counters[kNCnt] (u64)
void final_sum(cx_handle *h, int64_t n, const Part *partial, double *out);
inline const double *f2v_of(const cx_handle *h) { return h->cfg.dim == 1 ? (const double *)h->d_f2v : h->d_mv_f2v; }
inline const double *v2f_of(const cx_handle *h) { return h->cfg.dim == 1 ? (const double *)h->d_v2f : h->d_mv_v2f; }
inline Msgs msgs_of(const cx_handle *h, const Cache &C) { return {h->d_vinfo, f2v_of(h), v2f_of(h), C.d_W}; }

}  // namespace ev
}  // namespace cx
