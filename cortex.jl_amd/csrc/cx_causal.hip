// cx_causal.hip — cx_causal_marginals: the predicted, filtered and fixed-lag-smoothed marginal of every non-observed variable of a
// Gaussian model (dim 1 .. 4), from the stored factor→variable messages, on the device.  No counterpart in the reference (Cortex.jl
// computes no numbers); the derivation is DESIGN.md §4j.
//
// Every stored message into a non-observed variable i is of one class (cx_predictive's conventions):
//   U  upstream: an opaque message, or a rule factor on which i is not a CX_ROLE_IN end
//   O  i's own observations: a rule factor on which i is a CX_ROLE_IN end and whose OUT end is observed (CX_FACTOR_GAUSS_ADDITIVE,
//      dim 1: the other end observed, whichever id is lower)
//   T  transitions onward: a rule factor on which i is a CX_ROLE_IN end and whose OUT end is not observed
//   predicted = Σ U,   filtered = Σ U + Σ O,   fixed lag L = Σ U + Σ O + Σ_T β^(L)
//   β_a^(0) = flat;  β_a^(s) = the factor's rule towards i applied to  Σ O_j + Σ_{a' ∈ T_j} β_{a'}^(s-1),  j the OUT end of a
// Sums of the messages that are kept, never the belief minus what is left out: nothing cancels.
//
//   k_cm_split    one thread per variable: Σ U and Σ O over its slots by the class byte of each slot (an undefined message makes the sum NaN)
//   k_cm_back     launched L times, one thread per T slot, double-buffered over β: reads β^(s-1), writes β^(s) — O(L x transitions) over
//                 the whole graph, whatever rows are asked for
//   k_cm_out      one thread per row: the parts added up, one d x d Cholesky, mean | covariance and the row's status
//   k_ev_final    (cx_evidence.hip) the block counters in index order: no atomics
#include "cx_evidence_core.h"
#include "cx_scalar_core.h"

namespace cx {
namespace cm {

using ev::Lay;

constexpr int kCB = 128;      // threads per block of the T-slot and row passes
constexpr uint8_t kU = 0, kO = 1, kT = 2;

// the variables' slots, their classes and, per T slot, its index in the β buffers (-1 elsewhere)
struct Graph {
    const int32_t *vbase, *vdeg;
    const uint8_t *vinfo, *cls;
    const int32_t *tidx;
};

template <int D>
__device__ __forceinline__ Msg<D> ld_slot(const double *__restrict__ f2v, int slot) {
    Msg<D> m;
    ev::ld_msg<D>(f2v, slot, m.eta, m.lam);
    return m;
}

template <int D>
__device__ __forceinline__ Msg<D> ld_row(const double *__restrict__ buf, int64_t row) {
    Msg<D> m;
    const double *p = buf + row * Msg<D>::NC;
#pragma unroll
    for (int k = 0; k < D; k++) m.eta[k] = p[k];
#pragma unroll
    for (int k = 0; k < Msg<D>::NT; k++) m.lam[k] = p[D + k];
    return m;
}

template <int D>
__device__ __forceinline__ void st_row(double *__restrict__ buf, int64_t row, const Msg<D> &m) {
    double *p = buf + row * Msg<D>::NC;
#pragma unroll
    for (int k = 0; k < D; k++) p[k] = m.eta[k];
#pragma unroll
    for (int k = 0; k < Msg<D>::NT; k++) p[D + k] = m.lam[k];
}

// m += Σ β[tidx[s]] over the T slots s of variable v
template <int D>
__device__ __forceinline__ void add_onward(const Graph &G, int v, const double *__restrict__ beta, Msg<D> &m) {
    const int deg = G.vdeg[v], b = G.vbase[v], stride = (G.vinfo[v] & kDegMask) == kBigDeg ? 1 : kBlock;
    for (int k = 0; k < deg; k++) {
        const int s = b + k * stride;
        if (G.cls[s] != kT) continue;
        const int t = G.tidx[s];
        if (t >= 0) msg_add<D>(m, ld_row<D>(beta, t));      // (a T slot of a factor of three or more variables has no entry: lag 0 only)
    }
}

// sums[2 v] = Σ U_v, sums[2 v + 1] = Σ O_v (rows of NC doubles)
template <int D>
__global__ __launch_bounds__(ev::kB) void k_cm_split(int64_t nv, Graph G, const double *__restrict__ f2v, double *__restrict__ sums) {
    const int64_t v = (int64_t)blockIdx.x * ev::kB + threadIdx.x;
    if (v >= nv) return;
    const int info = G.vinfo[v];
    if (info & (kClamped | kGhost)) return;
    const int deg = G.vdeg[v], b = G.vbase[v], stride = (info & kDegMask) == kBigDeg ? 1 : kBlock;
    Msg<D> u = msg_zero<D>(), o = msg_zero<D>();
    for (int k = 0; k < deg; k++) {
        const int s = b + k * stride;
        const uint8_t c = G.cls[s];
        if (c == kT) continue;
        const Msg<D> m = ld_slot<D>(f2v, s);
        if (c == kO) msg_add<D>(o, m); else msg_add<D>(u, m);
    }
    st_row<D>(sums, 2 * v, u);
    st_row<D>(sums, 2 * v + 1, o);
}

// T entry t: rec[t] = (receiving slot of i, variable j = the OUT end, dim > 1: the rule table of the message j sends to i, 0).
// dim 1: (q, a, b) of the receiving slot, as the sweeps read them (a, b null: additive factors only)
struct Rules {
    const double *q, *a, *b, *ptab;
};

template <int D>
__global__ __launch_bounds__(kCB) void k_cm_back(int64_t nt, const int4 *__restrict__ rec, Graph G, Rules R, const double *__restrict__ sums,
                                                 const double *__restrict__ prev, double *__restrict__ next) {
    const int64_t t = (int64_t)blockIdx.x * kCB + threadIdx.x;
    if (t >= nt) return;
    const int4 r = rec[t];
    Msg<D> m = ld_row<D>(sums, 2 * (int64_t)r.y + 1);
    if (prev) add_onward<D>(G, r.y, prev, m);      // (prev null: β^(0), flat)
    // nothing downstream has been seen: β stays flat exactly (the rule of dim > 1 would leave the rounding of C - Y'Y)
    bool flat = true;
#pragma unroll
    for (int k = 0; k < D; k++) flat = flat && m.eta[k] == 0.0;
#pragma unroll
    for (int k = 0; k < Msg<D>::NT; k++) flat = flat && m.lam[k] == 0.0;
    Msg<D> o = msg_zero<D>();
    if (!flat) {
        if constexpr (D == 1) {
            const double2 in = make_double2(m.eta[0], m.lam[0]);
            const double2 x = R.a ? factor_rule<kRuleLinear>(in, R.q[r.x], R.a[r.x], R.b[r.x]) : factor_rule<kRuleAdditive>(in, R.q[r.x], 1.0, 0.0);
            o.eta[0] = x.x; o.lam[0] = x.y;
        } else {
            o = mv_rule<D, false>(m, R.ptab + (int64_t)r.z * 3 * D * D);
        }
    }
    st_row<D>(next, t, o);
}

// row i of out: mean[D] | covariance[D][D]; rows null: variable i itself
template <int D>
__global__ __launch_bounds__(kCB) void k_cm_out(int64_t n, const int32_t *__restrict__ rows, Graph G, int filtered, const double *__restrict__ sums,
                                                const double *__restrict__ beta, const double *__restrict__ v2f, double *__restrict__ out,
                                                ev::Part *__restrict__ partial) {
    const int64_t i = (int64_t)blockIdx.x * kCB + threadIdx.x;
    int st = -1;      // -1: no row, 0 finite, 1 an undefined input, 2 improper
    if (i < n) {
        const int v = rows ? rows[i] : (int)i;
        const int info = G.vinfo[v];
        double mean[D], S[D][D];
        st = 0;
        if (info & kClamped) {
            if (G.vdeg[v] > 0) ev::datum<D>(v2f, G.vbase[v], mean);
            else st = 1;
#pragma unroll
            for (int p = 0; p < D; p++)
#pragma unroll
                for (int q = 0; q < D; q++) S[p][q] = 0.0;
        } else {
            Msg<D> m = ld_row<D>(sums, 2 * (int64_t)v);
            if (filtered) msg_add<D>(m, ld_row<D>(sums, 2 * (int64_t)v + 1));
            if (beta) add_onward<D>(G, v, beta, m);
            bool undef = false;
#pragma unroll
            for (int k = 0; k < D; k++) undef = undef || __builtin_isnan(m.eta[k]);
#pragma unroll
            for (int k = 0; k < Msg<D>::NT; k++) undef = undef || __builtin_isnan(m.lam[k]);
            double L[D][D], y[D], logdet, quad;
#pragma unroll
            for (int p = 0; p < D; p++) {
                y[p] = m.eta[p];
#pragma unroll
                for (int q = 0; q < D; q++) L[p][q] = ev::lam_at<D>(m.lam, p, q);
            }
            if (undef) st = 1;
            else if (!ev::chol_quad<D>(L, y, logdet, quad)) st = 2;
            else {
                ev::back_solve<D>(L, y, mean);
                ev::inv_lower<D>(L);
                ev::gram_lower<D>(L, S);
#pragma unroll
                for (int p = 0; p < D; p++)
#pragma unroll
                    for (int q = 0; q < p; q++) S[q][p] = S[p][q];
            }
        }
        const double nan = __builtin_nan("");
        double *o = out + i * (D + D * D);
#pragma unroll
        for (int p = 0; p < D; p++) {
            o[p] = st ? nan : mean[p];
#pragma unroll
            for (int q = 0; q < D; q++) o[D + p * D + q] = st ? nan : S[p][q];
        }
    }
    ev::block_part<kCB>(0.0, 0.0, st == 0, st == 1, st == 2, 0, partial);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// The plan follows the flattened graph and the observed flags (cx_derived.h: causal_plan_dirty); the rule parameters are read from the
// handle's tables by every call, the scratch is sized by the plan and the rows of the last call.
struct Plan {
    int64_t n_t = 0;                      // T slots
    int64_t multi_in_fac = -1;            // a transition through a factor of three or more variables (id): no fixed-lag recursion
    DevBuf<uint8_t> d_cls;
    DevBuf<int32_t> d_tidx, d_rows;
    DevBuf<int4> d_trec;
    DevBuf<double> d_sums, d_beta[2], d_rows_out, d_out;
    DevBuf<ev::Part> d_partial;
    double *h_out = nullptr;              // counters, pinned
    Plan() = default;
    Plan(const Plan &) = delete;
    ~Plan() { if (h_out) (void)hipHostFree(h_out); }
};

int32_t build_plan(cx_handle *h, const ev::Cache &E, Plan &P) {
    using namespace cxh;
    const int d = h->cfg.dim;
    auto obs = [&](int32_t v) { return (h->vinfo[(size_t)v] & kClamped) != 0; };
    std::vector<uint8_t> cls((size_t)std::max<int64_t>(h->nslots, 1), kU);
    std::vector<int32_t> tidx((size_t)std::max<int64_t>(h->nslots, 1), -1);
    std::vector<int4> trec;
    P.multi_in_fac = -1;
    for (size_t p = 0; p < E.pair.size(); p++) {
        const int4 r = E.pair[p];      // (slot out, slot in, var out, var in)
        if (!obs(r.w)) {
            cls[(size_t)r.y] = obs(r.z) ? kO : kT;
            if (!obs(r.z)) trec.push_back(make_int4(r.y, r.z, d > 1 ? h->spdir[(size_t)r.x] : 0, 0));
        } else if (d == 1 && !obs(r.z) && h->fac_kind[(size_t)E.pair_fac[p]] == CX_FACTOR_GAUSS_ADDITIVE) cls[(size_t)r.x] = kO;
    }
    for (int64_t k = 0; k < E.n_kary; k++) {
        const int32_t *sl = &E.krec[(size_t)k * 16], *vr = sl + 8;
        if (sl[0] < 0) continue;
        for (int e = 1; e < 8; e++) {
            if (sl[e] < 0 || obs(vr[e])) continue;
            cls[(size_t)sl[e]] = obs(vr[0]) ? kO : kT;
            if (!obs(vr[0]) && P.multi_in_fac < 0)
                for (int64_t f = 0; f < h->nf; f++) if (E.kary_row_of_fac[(size_t)f] == k) { P.multi_in_fac = h->fac_ids[(size_t)f]; break; }
        }
    }
    // the T slots in the order of the variable they gather from: neighbouring threads of k_cm_back read neighbouring rows of the sums
    std::stable_sort(trec.begin(), trec.end(), [](const int4 &a, const int4 &b) { return a.y < b.y; });
    CX_REQUIRE(h, trec.size() < (size_t)1 << 31, CX_ERR_UNSUPPORTED, "cx_causal_marginals: more than 2^31 transitions");
    for (size_t t = 0; t < trec.size(); t++) tidx[(size_t)trec[t].x] = (int32_t)t;
    P.n_t = (int64_t)trec.size();
    reset_all(P.d_cls, P.d_tidx, P.d_trec, P.d_sums, P.d_beta[0], P.d_beta[1]);
    int32_t rc;
    if ((rc = dev_upload(h, &P.d_cls, cls)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &P.d_tidx, tidx)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &P.d_trec, trec)) != CX_OK) return rc;
    if ((rc = dev_alloc(h, &P.d_sums, 2 * h->nv * (d + d * (d + 1) / 2))) != CX_OK) return rc;
    if (!P.d_out && (rc = dev_alloc(h, &P.d_out, 1 + ev::kNCnt)) != CX_OK) return rc;
    if (!P.h_out) CX_HIP(h, hipHostMalloc((void **)&P.h_out, (1 + ev::kNCnt) * sizeof(double), hipHostMallocDefault));
    CX_HIP(h, hipStreamSynchronize(h->stream));      // (the host vectors die here)
    return CX_OK;
}

// the three passes on the handle's stream; returns the buffer that holds β^(lag) (null: lag 0)
template <int D>
void launch(cx_handle *h, Plan &P, int filtered, int32_t lag, int64_t n, const int32_t *d_rows) {
    const Graph G{h->d_vbase, h->d_var_deg, h->d_vinfo, P.d_cls, P.d_tidx};
    const double *f2v = ev::f2v_of(h);
    const int64_t nb_v = (h->nv + ev::kB - 1) / ev::kB, nb_t = (P.n_t + kCB - 1) / kCB, nb_r = (n + kCB - 1) / kCB;
    if (nb_v) hipLaunchKernelGGL(k_cm_split<D>, dim3((unsigned)nb_v), dim3(ev::kB), 0, h->stream, h->nv, G, f2v, P.d_sums.get());
    const double *beta = nullptr;
    if (nb_t) {
        const Rules R{h->d_q, h->d_a, h->d_b, h->d_ptab};
        for (int32_t s = 0; s < lag; s++) {
            double *next = P.d_beta[s & 1];
            hipLaunchKernelGGL(k_cm_back<D>, dim3((unsigned)nb_t), dim3(kCB), 0, h->stream, P.n_t, P.d_trec.get(), G, R, P.d_sums.get(), beta, next);
            beta = next;
        }
    }
    if (nb_r)
        hipLaunchKernelGGL(k_cm_out<D>, dim3((unsigned)nb_r), dim3(kCB), 0, h->stream, n, d_rows, G, filtered, P.d_sums.get(), beta, ev::v2f_of(h),
                           P.d_rows_out.get(), P.d_partial.get());
    ev::final_sum(h, nb_r, P.d_partial, P.d_out);
}

}  // namespace cm

template <> void Deleter<cm::Plan>::operator()(cm::Plan *P) const { delete P; }

}  // namespace cx

using namespace cxh;

extern "C" int32_t cx_causal_marginals(cx_handle *h, int32_t mode, int32_t lag, int64_t n, const int64_t *variable_ids, double *out, int64_t *counts4) {
    try {
        cx::ev::Cache *Ep = nullptr;
        int32_t rc;
        const char *bad = !out || !counts4 ? "null argument"
                          : mode != CX_CAUSAL_PREDICTED && mode != CX_CAUSAL_FILTERED ? "mode is CX_CAUSAL_PREDICTED or CX_CAUSAL_FILTERED"
                          : lag < 0 ? "negative lag"
                          : lag > 0 && mode == CX_CAUSAL_PREDICTED ? "a lag goes with CX_CAUSAL_FILTERED"
                          : variable_ids && n < 0 ? "negative count" : nullptr;
        if ((rc = cx::ev::prepare(h, "cx_causal_marginals", bad, Ep)) != CX_OK) return rc;
        CX_REQUIRE(h, !h->offsets_nonzero, CX_ERR_UNSUPPORTED, "cx_causal_marginals: the handle has non-zero factor offsets (cx_set_factor_offsets), which this call does not implement");
        if (!h->causal) { h->causal.reset(new cx::cm::Plan()); h->causal_plan_dirty = true; }
        cx::cm::Plan &P = *h->causal;
        if (h->causal_plan_dirty) {
            if ((rc = cx::cm::build_plan(h, *Ep, P)) != CX_OK) { h->causal.reset(); return rc; }
            h->causal_plan_dirty = false;
        }
        CX_REQUIRE(h, lag == 0 || P.multi_in_fac < 0, CX_ERR_UNSUPPORTED,
                   "cx_causal_marginals: factor " + std::to_string(P.multi_in_fac) + " is a transition of three or more variables with a free CX_ROLE_OUT end: "
                   "the fixed-lag recursion has no single predecessor there (lag 0 only)");
        const int d = h->cfg.dim, nc = d + d * (d + 1) / 2, no = d + d * d;
        const int64_t rows = variable_ids ? n : h->nv;
        const int32_t *d_rows = nullptr;
        if (variable_ids) {
            std::vector<int32_t> idx((size_t)rows);
            for (int64_t i = 0; i < rows; i++) {
                const int64_t v = find_var(h, variable_ids[i]);
                if (v < 0) return fail(h, CX_ERR_NOT_FOUND, "cx_causal_marginals: no variable " + std::to_string(variable_ids[i]));
                idx[(size_t)i] = (int32_t)v;
            }
            if ((rc = P.d_rows.ensure(h, rows)) != CX_OK) return rc;
            if (rows) CX_HIP(h, hipMemcpy(P.d_rows, idx.data(), (size_t)rows * sizeof(int32_t), hipMemcpyHostToDevice));
            d_rows = P.d_rows;
        }
        if ((rc = P.d_rows_out.ensure(h, rows * no)) != CX_OK) return rc;
        if ((rc = P.d_partial.ensure(h, (rows + cx::cm::kCB - 1) / cx::cm::kCB)) != CX_OK) return rc;
        if (lag > 0)
            for (int k = 0; k < std::min<int32_t>(lag, 2); k++) if ((rc = P.d_beta[k].ensure(h, P.n_t * nc)) != CX_OK) return rc;
        cx::ev::with_dim(d, [&](auto D) { cx::cm::launch<D()>(h, P, mode == CX_CAUSAL_FILTERED, lag, rows, d_rows); });
        CX_HIP(h, hipGetLastError());
        if (rows) CX_HIP(h, hipMemcpyAsync(out, P.d_rows_out, (size_t)(rows * no) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        CX_HIP(h, hipMemcpyAsync(P.h_out, P.d_out, (1 + cx::ev::kNCnt) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        CX_HIP(h, hipStreamSynchronize(h->stream));
        uint64_t cnt[cx::ev::kNCnt];
        std::memcpy(cnt, P.h_out + 1, sizeof(cnt));
        counts4[0] = rows;
        for (int k = 1; k < 4; k++) counts4[k] = (int64_t)cnt[k - 1];
        return CX_OK;
    } catch (const std::bad_alloc &) { return fail(h, CX_ERR_OUT_OF_MEMORY, "cx_causal_marginals: host allocation failed"); }
}
