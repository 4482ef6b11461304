// cx_evidence_core.h — what the log-evidence (cx_evidence.hip) and the factor-statistics (cx_learn.hip) passes share: the
// per-variable scratch of the variable pass, compensated sums, message loads, small Cholesky solves, the centred leave-one-out
// message of one factor edge, and the cached work lists of a handle.  Derivations: DESIGN.md §4e and §4f.
#pragma once
#include "cx_host.h"
#include "cx_mv_core.h"

namespace cx {
namespace ev {

constexpr int kB = 256;        // threads per block of the variable, pairwise and final passes
constexpr double kLog2Pi = 1.83787706640934548356;

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

// in-place lower Cholesky of the full symmetric J (lower triangle read), then h <- L⁻¹ h: log det J and h'J⁻¹h.  false: not positive definite
template <int N>
__device__ __forceinline__ bool chol_quad(double (&J)[N][N], double (&h)[N], double &logdet, double &quad) {
    logdet = 0.0; quad = 0.0;
#pragma unroll
    for (int j = 0; j < N; j++) {
        double d = J[j][j];
#pragma unroll
        for (int k = 0; k < j; k++) d -= J[j][k] * J[j][k];
        if (!(d > 0.0)) return false;
        logdet += log(d);
        const double l = sqrt(d), il = 1.0 / l;
        J[j][j] = l;
#pragma unroll
        for (int i = j + 1; i < N; i++) {
            double s = J[i][j];
#pragma unroll
            for (int k = 0; k < j; k++) s -= J[i][k] * J[j][k];
            J[i][j] = s * il;
        }
    }
#pragma unroll
    for (int i = 0; i < N; i++) {
        double s = h[i];
#pragma unroll
        for (int k = 0; k < i; k++) s -= J[i][k] * h[k];
        h[i] = s / J[i][i];
        quad += h[i] * h[i];
    }
    return true;
}

// Λ μ = η by the factor chol_quad left in L (h = L⁻¹ η on entry): back substitution
template <int N>
__device__ __forceinline__ void back_solve(const double (&L)[N][N], const double (&y)[N], double (&x)[N]) {
#pragma unroll
    for (int i = N - 1; i >= 0; i--) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < N; k++) s -= L[k][i] * x[k];
        x[i] = s / L[i][i];
    }
}

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

// ---- host: the work lists -------------------------------------------------------------------------------------------------------
struct Cache {
    bool built = false;
    uint64_t epoch = ~0ull;
    int64_t zero_noise_fac = -1;          // a factor with q = 0 (dim 1): refused
    int64_t unsupported_fac = -1;         // a factor of a kind without a sum-product rule
    int64_t n_pair = 0, n_kary = 0, nb = 0;
    int32_t *d_vrec = nullptr;
    uint8_t *d_tail = nullptr;
    int4 *d_pair = nullptr;
    int32_t *d_pair_ps = nullptr, *d_krec = nullptr, *d_kps = nullptr;
    double *d_pq = nullptr, *d_pa = nullptr, *d_pb = nullptr, *d_kc = nullptr, *d_ptab = nullptr;
    int64_t ptab_cap = 0;
    std::vector<int32_t> pair_ps;         // dim > 1: parameter set per pair (what the table must hold)
    std::vector<int64_t> pair_fac;        // factor index of every pair row (rows in factor order)
    double *d_W = nullptr;
    Part *d_partial = nullptr;
    double *d_out = nullptr, *h_out = nullptr;      // value | counters; h_out: pinned
};

// the checks every evidence-type call makes (family, dim, partitions, captured stream, rule kinds, zero noise), then the work lists,
// the parameter table and (chain scan, dim 2..4) the messages in their slots; `who` prefixes every error text
int32_t prepare(cx_handle *h, const std::string &who, Cache *&C);
// pass 1 only (k_ev_var) on the handle's stream: the per-variable scratch C.d_W; the handle's stored f2v messages
void var_pass(cx_handle *h, Cache &C);
inline const double *f2v_of(const cx_handle *h) { return h->cfg.dim == 1 ? (const double *)h->d_f2v : h->d_mv_f2v; }
inline const double *v2f_of(const cx_handle *h) { return h->cfg.dim == 1 ? (const double *)h->d_v2f : h->d_mv_v2f; }

}  // namespace ev
}  // namespace cx
