// cx_predict.hip — cx_predictive and cx_predictive_rows: for every observation y_a that a Gaussian rule factor generates, the
// predictive distribution of that datum given other data, its log score and its squared standardised residual, dim 1 .. 4, from the
// stored factor→variable messages, on the device.  No counterpart in the reference (Cortex.jl computes no numbers); the derivation is
// DESIGN.md §4h.
//
// A row is a factor  y = Σ_i A_i x_i + b + N(0, Q)  whose datum end is its only observed variable.  With the cavity of every input,
//   m_{i\a} = M_i - m_{a→i} - (the messages the mode leaves out)  ->  (μ_i^c, Σ_i^c),
//   ŷ = Σ_i A_i μ_i^c + b,   S = Σ_i A_i Σ_i^c A_i' + Q,   log N(y; ŷ, S),   (y - ŷ)' S⁻¹ (y - ŷ).
// The cavity is formed as the evidence forms its leave-one-out messages (ev::free_edge): centred on the belief mean μ_i, so that
// μ_i^c = μ_i + (Λ_i^c)⁻¹ η~ with η~ of the size of the messages taken out, not of the size of the data.
//
//   k_ev_var      (cx_evidence.hip) one thread per variable: the belief means and precisions (scratch W)
//   k_pr_rows     one thread per row: at most six cavities (one d x d Cholesky and inverse each), S = L L', the row's d + d² + 2
//                 doubles, and the block's compensated partial sum of the log scores with its counters
//   k_ev_final    (cx_evidence.hip) the block partials in index order: two calls on one state are bit-identical, no atomics
#include "cx_evidence_core.h"

namespace cx {
namespace pr {

using ev::Lay;
using ev::kLog2Pi;

constexpr int kPB = 128;       // threads per block: one row each

// row r: rec[r] = (pair row or k-ary row of the evidence tables, flags, index of its first input in xoff, 0); flags bit 0: a k-ary row;
// bit 1: a pair row whose datum sits on the `in` end (CX_FACTOR_GAUSS_ADDITIVE, symmetric): the free end is `out`.
// The slots the mode leaves out of input j's cavity besides the row's own: xs[xoff[j] .. xoff[j + 1]) (xoff null: none, CX_PREDICT_LOO);
// a first entry of -1 says that NO message into the variable is left: the cavity is flat by structure, not by a difference that rounds to 0
constexpr int kKary = 1, kFlipped = 2;
struct Rows {
    const int4 *rec;
    const int32_t *xoff, *xs;
};

// A cavity is a DIFFERENCE of precisions: the belief's minus the messages taken out.  Where what is left is flat — the flat message
// behind a forecast's end, a direction no other datum informs — the difference is the rounding of its terms, a number of either sign
// around 1e-16 of the belief's own entry.  A Cholesky pivot below kFlatPivot (64 ulp: fewer than six bits of it are left) times the
// belief's diagonal entry is such a remainder, and the cavity improper, as with a pivot <= 0.
constexpr double kFlatPivot = 64 * 2.220446049250313e-16;

template <int D>
__device__ __forceinline__ bool resolved(const double (&A)[D][D], const double (&ref)[D]) {
    double L[D][D];
#pragma unroll
    for (int j = 0; j < D; j++) {
        double s = A[j][j];
#pragma unroll
        for (int k = 0; k < j; k++) s -= L[j][k] * L[j][k];
        if (!(s > kFlatPivot * fmax(ref[j], 0.0))) return false;
        L[j][j] = sqrt(s);
#pragma unroll
        for (int i = j + 1; i < D; i++) {
            double t = A[i][j];
#pragma unroll
            for (int k = 0; k < j; k++) t -= L[i][k] * L[j][k];
            L[i][j] = t / L[j][j];
        }
    }
    return true;
}

// the cavity of the free variable `var` behind `slot`: mean mc, covariance Sc.  0, 1 (an undefined input) or 2 (not positive definite)
template <int D>
__device__ __forceinline__ int cavity(const ev::Msgs &M, const Rows &R, int slot, int var, int input, double (&mc)[D], double (&Sc)[D][D]) {
    constexpr int NT = Lay<D>::NT;
    double mu[D], et[D], lm[NT];
    bool ok = ev::free_edge<D>(M.f2v, M.W, slot, var, mu, et, lm), flat = false;
    if (R.xoff) {
        for (int k = R.xoff[input]; k < R.xoff[input + 1]; k++) {
            const int xs = R.xs[k];
            if (xs < 0) { flat = true; continue; }      // (the list's first entry: every message into the variable is taken out)
            double e[D], l[NT];
            ev::ld_msg<D>(M.f2v, xs, e, l);
#pragma unroll
            for (int i = 0; i < D; i++) {
                double t = e[i];
#pragma unroll
                for (int j = 0; j < D; j++) t -= ev::lam_at<D>(l, i, j) * mu[j];
                et[i] -= t;
                ok = ok && !__builtin_isnan(e[i]);
            }
#pragma unroll
            for (int i = 0; i < NT; i++) { lm[i] -= l[i]; ok = ok && !__builtin_isnan(l[i]); }
        }
    }
    if (!ok) return 1;
    if (flat) return 2;      // nothing is left: a flat cavity by structure, whatever the rounding of M_i minus its own terms leaves behind
    double L[D][D], dl[D], ref[D], logdet, quad;
    const double *w = M.W + (int64_t)var * Lay<D>::K + D;      // the belief's precision (free_edge)
#pragma unroll
    for (int i = 0; i < D; i++) {
        ref[i] = w[tri<D>(i, i)];
#pragma unroll
        for (int j = 0; j < D; j++) L[i][j] = ev::lam_at<D>(lm, i, j);
    }
    if (!resolved<D>(L, ref)) return 2;
    if (!ev::chol_quad<D>(L, et, logdet, quad)) return 2;
    ev::back_solve<D>(L, et, dl);
    ev::inv_lower<D>(L);
    ev::gram_lower<D>(L, Sc);
#pragma unroll
    for (int i = 0; i < D; i++) {
        mc[i] = mu[i] + dl[i];
#pragma unroll
        for (int j = 0; j < i; j++) Sc[j][i] = Sc[i][j];
    }
    return 0;
}

// yh += A mc, S += A Sc A'  (A null: the identity)
template <int D>
__device__ __forceinline__ void push(const double *__restrict__ A, double a1, const double (&mc)[D], const double (&Sc)[D][D], double (&yh)[D],
                                     double (&S)[D][D]) {
    if constexpr (D == 1) {
        yh[0] += a1 * mc[0];
        S[0][0] += a1 * a1 * Sc[0][0];
    } else {
        double T[D][D];      // A Sc
#pragma unroll
        for (int i = 0; i < D; i++) {
            double t = 0.0;
#pragma unroll
            for (int k = 0; k < D; k++) t += A[i * D + k] * mc[k];
            yh[i] += t;
#pragma unroll
            for (int j = 0; j < D; j++) {
                double u = 0.0;
#pragma unroll
                for (int k = 0; k < D; k++) u += A[i * D + k] * Sc[k][j];
                T[i][j] = u;
            }
        }
#pragma unroll
        for (int i = 0; i < D; i++)
#pragma unroll
            for (int j = 0; j <= i; j++) {
                double u = 0.0;
#pragma unroll
                for (int k = 0; k < D; k++) u += T[i][k] * A[j * D + k];
                S[i][j] += u;
            }
    }
}

// S (lower) += Q, from the table's Q⁻¹ (dim > 1: Q = (Q⁻¹)⁻¹ through the kit; Q⁻¹ is positive definite, cx_set_factor_matrices checked Q)
template <int D>
__device__ __forceinline__ void add_noise(const double *__restrict__ Qi, double q1, double (&S)[D][D]) {
    if constexpr (D == 1) S[0][0] += q1;
    else {
        double L[D][D], Q[D][D];
#pragma unroll
        for (int i = 0; i < D; i++)
#pragma unroll
            for (int j = 0; j < D; j++) L[i][j] = Qi[i * D + j];
        (void)ev::chol<D>(L);
        ev::inv_lower<D>(L);
        ev::gram_lower<D>(L, Q);
#pragma unroll
        for (int i = 0; i < D; i++)
#pragma unroll
            for (int j = 0; j <= i; j++) S[i][j] += Q[i][j];
    }
}

template <int D>
__global__ __launch_bounds__(kPB) void k_pr_rows(int64_t n, Rows R, ev::PairTab PT, ev::KaryTab KT, ev::Msgs M, double *__restrict__ out,
                                                 ev::Part *__restrict__ partial) {
    constexpr int PS = 2 * D * D + 2, NO = D + D * D + 2;
    const int64_t i = (int64_t)blockIdx.x * kPB + threadIdx.x;
    double s = 0.0, c = 0.0;
    int st = -1;      // -1: no row, 0 scored, 1 an undefined input, 2 improper
    if (i < n) {
        const int4 rr = R.rec[i];
        double y[D], yh[D], S[D][D], mc[D], Sc[D][D];
#pragma unroll
        for (int p = 0; p < D; p++) {
            yh[p] = 0.0;
#pragma unroll
            for (int q = 0; q < D; q++) S[p][q] = 0.0;
        }
        st = 0;
        auto merge = [&](int t) { st = t == 1 || st == 1 ? 1 : (t == 2 ? 2 : st); };
        if (rr.y & kKary) {
            const int64_t f = rr.x;
            const int32_t *sl = KT.krec + f * 16, *vr = sl + 8;
            ev::datum<D>(M.v2f, sl[0], y);
            int input = rr.z;
            for (int e = 1; e < 8; e++) {
                if (sl[e] < 0) continue;
                const int t = cavity<D>(M, R, sl[e], vr[e], input++, mc, Sc);
                merge(t);
                if (t) continue;
                if constexpr (D == 1) push<D>(nullptr, -KT.kc[f * 10 + e], mc, Sc, yh, S);
                else push<D>(KT.ptab + (int64_t)KT.kps[f * 8 + e] * PS, 1.0, mc, Sc, yh, S);
            }
            if constexpr (D == 1) { yh[0] += KT.kc[f * 10 + 9]; add_noise<D>(nullptr, KT.kc[f * 10 + 8], S); }
            else add_noise<D>(KT.ptab + (int64_t)KT.kps[f * 8] * PS + D * D, 0.0, S);
        } else {
            const int64_t p = rr.x;
            const int4 r = PT.rec[p];      // (slot out, slot in, var out, var in)
            const bool fl = (rr.y & kFlipped) != 0;
            ev::datum<D>(M.v2f, fl ? r.y : r.x, y);
            merge(cavity<D>(M, R, fl ? r.x : r.y, fl ? r.z : r.w, rr.z, mc, Sc));
            if (st == 0) {
                if constexpr (D == 1) {
                    push<D>(nullptr, PT.pa ? PT.pa[p] : 1.0, mc, Sc, yh, S);      // (a flipped row is additive: a = 1, b = 0)
                    yh[0] += PT.pb ? PT.pb[p] : 0.0;
                    add_noise<D>(nullptr, PT.pq[p], S);
                } else {
                    const double *t = PT.ptab + (int64_t)PT.pset[p] * PS;
                    push<D>(t, 1.0, mc, Sc, yh, S);
                    if (PT.pb) {      // cx_set_factor_offsets: y^ = A mu + b
#pragma unroll
                        for (int q = 0; q < D; q++) yh[q] += PT.pb[p * D + q];
                    }
                    add_noise<D>(t + D * D, 0.0, S);
                }
            }
        }
        double e[D], Ls[D][D], logdet = 0.0, maha = 0.0;
#pragma unroll
        for (int p = 0; p < D; p++) {
            e[p] = y[p] - yh[p];
#pragma unroll
            for (int q = 0; q <= p; q++) { S[q][p] = S[p][q]; Ls[p][q] = S[p][q]; }
        }
        if (st == 0 && !ev::chol_quad<D>(Ls, e, logdet, maha)) st = 2;
        const double ld = -0.5 * (D * kLog2Pi + logdet + maha), nan = __builtin_nan("");
        if (out) {
            double *o = out + i * NO;
#pragma unroll
            for (int p = 0; p < D; p++) {
                o[p] = st ? nan : yh[p];
#pragma unroll
                for (int q = 0; q < D; q++) o[D + p * D + q] = st ? nan : S[p][q];
            }
            o[D + D * D] = st ? nan : ld;
            o[D + D * D + 1] = st ? nan : maha;
        }
        if (st == 0) ev::neu(s, c, ld);
    }
    ev::block_part<kPB>(s, c, st == 0, st == 1, st == 2, 0, partial);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
struct Plan {
    // what the rows were built for: the mode, the caller's ids (or none) and the observed flags
    bool valid = false, explicit_ids = false;
    int32_t mode = 0;
    std::vector<int64_t> ids;
    std::vector<uint8_t> vinfo;
    int64_t n_rows = 0, nb = 0;
    DevBuf<int4> d_rec;
    DevBuf<int32_t> d_xoff, d_xs;
    DevBuf<ev::Part> d_partial;
    DevBuf<double> d_rows, d_out;
    double *h_out = nullptr;      // value | counters, pinned
    Plan() = default;
    Plan(const Plan &) = delete;
    ~Plan() { if (h_out) (void)hipHostFree(h_out); }
};

int no_of(int d) { return d + d * d + 2; }

// what factor index f is: 0 no row, else 1 + its flags (kKary, kFlipped).  A row's datum end is its only observed variable: the OUT
// end, or either end of a CX_FACTOR_GAUSS_ADDITIVE (dim 1)
int classify(const cx_handle *h, const ev::Cache &E, int64_t f) {
    auto obs = [&](int32_t v) { return (h->vinfo[(size_t)v] & kClamped) != 0; };
    const int32_t p = E.row_of_fac[(size_t)f], k = E.kary_row_of_fac[(size_t)f];
    if (p >= 0) {
        const int4 r = E.pair[(size_t)p];
        if (obs(r.z) && !obs(r.w)) return 1;
        if (h->cfg.dim == 1 && h->fac_kind[(size_t)f] == CX_FACTOR_GAUSS_ADDITIVE && obs(r.w) && !obs(r.z)) return 1 + kFlipped;
        return 0;
    }
    if (k >= 0) {
        const int32_t *sl = &E.krec[(size_t)k * 16], *vr = sl + 8;
        if (sl[0] < 0 || !obs(vr[0])) return 0;
        for (int e = 1; e < 8; e++) if (sl[e] >= 0 && obs(vr[e])) return 0;
        return 1 + kKary;
    }
    return 0;
}

const char *kNotARow = " is not a row: a Gaussian rule factor whose CX_ROLE_OUT end (CX_FACTOR_GAUSS_ADDITIVE, dim 1: either end) is its only observed variable";

// the factor indices of the rows, checked: the caller's, in the caller's order, or every row in ascending factor id
int32_t list_rows(cx_handle *h, const ev::Cache &E, const std::string &who, int64_t n, const int64_t *ids, std::vector<int64_t> &fac, std::vector<int> &cls) {
    using namespace cxh;
    fac.clear(); cls.clear();
    if (!ids) {
        for (int64_t f = 0; f < h->nf; f++) {
            const int c = classify(h, E, f);
            if (c) { fac.push_back(f); cls.push_back(c - 1); }
        }
        return CX_OK;
    }
    for (int64_t i = 0; i < n; i++) {
        const int64_t f = find_factor(h, ids[i]);
        if (f < 0) return fail(h, CX_ERR_NOT_FOUND, who + ": no factor " + std::to_string(ids[i]));
        const int c = classify(h, E, f);
        if (!c) return fail(h, CX_ERR_UNSUPPORTED, who + ": factor " + std::to_string(ids[i]) + kNotARow);
        fac.push_back(f); cls.push_back(c - 1);
    }
    return CX_OK;
}

int32_t build_plan(cx_handle *h, const ev::Cache &E, Plan &P, int32_t mode, const std::vector<int64_t> &fac, const std::vector<int> &cls) {
    using namespace cxh;
    const int64_t n = (int64_t)fac.size();
    std::vector<int4> rec((size_t)n);
    std::vector<int32_t> xoff, xs;
    // CX_PREDICT_CAUSAL: the slots on which a variable is the IN end of a rule factor (the `in` slot of a pair row — ADDITIVE: the
    // higher variable id —, entries 1 .. of a k-ary row)
    std::vector<uint8_t> in_slot;
    if (mode == CX_PREDICT_CAUSAL) {
        in_slot.assign((size_t)h->nslots, 0);
        for (const int4 &r : E.pair) in_slot[(size_t)r.y] = 1;
        for (int64_t k = 0; k < E.n_kary; k++)
            for (int e = 1; e < 8; e++) if (E.krec[(size_t)k * 16 + e] >= 0) in_slot[(size_t)E.krec[(size_t)k * 16 + e]] = 1;
        xoff.push_back(0);
    }
    int64_t n_inputs = 0;
    auto input = [&](int32_t slot, int32_t var) {
        n_inputs++;
        if (mode != CX_PREDICT_CAUSAL) return;
        const int32_t deg = h->var_off[(size_t)var + 1] - h->var_off[(size_t)var], stride = slot_stride(h, var);
        int32_t kept = 0;
        for (int32_t k = 0; k < deg; k++) {
            const int32_t s = h->vbase[(size_t)var] + k * stride;
            kept += s != slot && !in_slot[(size_t)s];
        }
        if (kept == 0) xs.push_back(-1);      // every message into the variable is taken out: the cavity is flat (k_pr_rows: improper)
        for (int32_t k = 0; k < deg; k++) {
            const int32_t s = h->vbase[(size_t)var] + k * stride;
            if (s != slot && in_slot[(size_t)s]) xs.push_back(s);
        }
        xoff.push_back((int32_t)xs.size());
    };
    for (int64_t i = 0; i < n; i++) {
        const int64_t f = fac[(size_t)i];
        CX_REQUIRE(h, n_inputs < (int64_t)1 << 31 && xs.size() < (size_t)1 << 31, CX_ERR_UNSUPPORTED, "cx_predictive: more than 2^31 inputs");
        if (cls[(size_t)i] & kKary) {
            const int32_t k = E.kary_row_of_fac[(size_t)f];
            rec[(size_t)i] = make_int4(k, cls[(size_t)i], (int32_t)n_inputs, 0);
            for (int e = 1; e < 8; e++) if (E.krec[(size_t)k * 16 + e] >= 0) input(E.krec[(size_t)k * 16 + e], E.krec[(size_t)k * 16 + 8 + e]);
        } else {
            const int32_t p = E.row_of_fac[(size_t)f];
            const int4 r = E.pair[(size_t)p];
            rec[(size_t)i] = make_int4(p, cls[(size_t)i], (int32_t)n_inputs, 0);
            if (cls[(size_t)i] & kFlipped) input(r.x, r.z); else input(r.y, r.w);
        }
    }
    P.valid = false;
    reset_all(P.d_rec, P.d_xoff, P.d_xs, P.d_partial);
    int32_t rc;
    if ((rc = dev_upload(h, &P.d_rec, rec)) != CX_OK) return rc;
    if (mode == CX_PREDICT_CAUSAL) {
        if ((rc = dev_upload(h, &P.d_xoff, xoff)) != CX_OK) return rc;
        if ((rc = dev_upload(h, &P.d_xs, xs)) != CX_OK) return rc;
    }
    P.n_rows = n;
    P.nb = (n + kPB - 1) / kPB;
    if ((rc = dev_alloc(h, &P.d_partial, P.nb)) != CX_OK) return rc;
    if (!P.d_out && (rc = dev_alloc(h, &P.d_out, 1 + ev::kNCnt)) != CX_OK) return rc;
    if (!P.h_out) CX_HIP(h, hipHostMalloc((void **)&P.h_out, (1 + ev::kNCnt) * sizeof(double), hipHostMallocDefault));
    CX_HIP(h, hipStreamSynchronize(h->stream));      // (the host vectors die here)
    return CX_OK;
}

template <int D>
void launch(cx_handle *h, const ev::Cache &E, const Plan &P, double *d_rows) {
    if (P.nb)
        hipLaunchKernelGGL(k_pr_rows<D>, dim3((unsigned)P.nb), dim3(kPB), 0, h->stream, P.n_rows, Rows{P.d_rec, P.d_xoff, P.d_xs}, E.pair_tab(), E.kary_tab(),
                           ev::msgs_of(h, E), d_rows, P.d_partial.get());
    ev::final_sum(h, P.nb, P.d_partial, P.d_out);
}

}  // namespace pr

template <> void Deleter<pr::Plan>::operator()(pr::Plan *P) const { delete P; }

}  // namespace cx

using namespace cxh;

extern "C" int32_t cx_predictive_rows(cx_handle *h, int64_t cap, int64_t *factor_ids, int64_t *n_rows) {
    try {
        cx::ev::Cache *Ep = nullptr;
        int32_t rc;
        const char *bad = n_rows && cap >= 0 && (cap == 0 || factor_ids) ? nullptr : "null argument or negative capacity";
        if ((rc = cx::ev::prepare(h, "cx_predictive_rows", bad, Ep)) != CX_OK) return rc;
        std::vector<int64_t> fac;
        std::vector<int> cls;
        if ((rc = cx::pr::list_rows(h, *Ep, "cx_predictive_rows", 0, nullptr, fac, cls)) != CX_OK) return rc;
        *n_rows = (int64_t)fac.size();
        for (int64_t i = 0; i < std::min<int64_t>(cap, *n_rows); i++) factor_ids[i] = h->fac_ids[(size_t)fac[(size_t)i]];
        return CX_OK;
    } catch (const std::bad_alloc &) { return fail(h, CX_ERR_OUT_OF_MEMORY, "cx_predictive_rows: host allocation failed"); }
}

extern "C" int32_t cx_predictive(cx_handle *h, int32_t mode, int64_t n, const int64_t *factor_ids, double *out, double *total, int64_t *counts4) {
    try {
        cx::ev::Cache *Ep = nullptr;
        int32_t rc;
        const char *bad = !counts4 ? "counts4 is null"
                          : mode != CX_PREDICT_LOO && mode != CX_PREDICT_CAUSAL ? "mode is CX_PREDICT_LOO or CX_PREDICT_CAUSAL"
                          : factor_ids && n < 0 ? "negative count" : nullptr;
        if ((rc = cx::ev::prepare(h, "cx_predictive", bad, Ep)) != CX_OK) return rc;
        cx::ev::Cache &E = *Ep;
        if (!h->predict) h->predict.reset(new cx::pr::Plan());
        cx::pr::Plan &P = *h->predict;
        const bool same = P.valid && P.mode == mode && P.explicit_ids == (factor_ids != nullptr) && P.vinfo == h->vinfo &&
                          (!factor_ids || ((int64_t)P.ids.size() == n && std::equal(factor_ids, factor_ids + n, P.ids.begin())));
        if (!same) {
            P.valid = false;
            std::vector<int64_t> fac;
            std::vector<int> cls;
            if ((rc = cx::pr::list_rows(h, E, "cx_predictive", n, factor_ids, fac, cls)) != CX_OK) return rc;
            if ((rc = cx::pr::build_plan(h, E, P, mode, fac, cls)) != CX_OK) return rc;
            P.mode = mode;
            P.explicit_ids = factor_ids != nullptr;
            P.ids.assign(factor_ids, factor_ids ? factor_ids + n : factor_ids);
            P.vinfo = h->vinfo;
            P.valid = true;
        }
        const int d = h->cfg.dim, no = cx::pr::no_of(d);
        if (out && (rc = P.d_rows.ensure(h, P.n_rows * no)) != CX_OK) return rc;
        cx::ev::var_pass(h, E);
        cx::ev::with_dim(d, [&](auto D) { cx::pr::launch<D()>(h, E, P, out ? P.d_rows.get() : nullptr); });
        CX_HIP(h, hipGetLastError());
        if (out && P.n_rows) CX_HIP(h, hipMemcpyAsync(out, P.d_rows, (size_t)(P.n_rows * no) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        CX_HIP(h, hipMemcpyAsync(P.h_out, P.d_out, (1 + cx::ev::kNCnt) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        CX_HIP(h, hipStreamSynchronize(h->stream));
        uint64_t cnt[cx::ev::kNCnt];
        std::memcpy(cnt, P.h_out + 1, sizeof(cnt));
        counts4[0] = P.n_rows;
        for (int k = 1; k < 4; k++) counts4[k] = (int64_t)cnt[k - 1];
        if (total) *total = P.h_out[0];
        return CX_OK;
    } catch (const std::bad_alloc &) { return fail(h, CX_ERR_OUT_OF_MEMORY, "cx_predictive: host allocation failed"); }
}
