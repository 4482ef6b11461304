// cx_learn.hip — cx_factor_beliefs and cx_factor_statistics: the joint posterior of every two-variable Gaussian factor and the
// expected sufficient statistics of EM (Shumway–Stoffer), dim 1 .. 4, from the stored factor→variable messages, on the device.
// No counterpart in the reference (Cortex.jl computes no numbers); the derivation is DESIGN.md §4f.
//
// The factor belief of x_out = A x_in + b + N(0, Q) is the pairwise pass of cx_log_evidence (k_ev_pair): in coordinates centred on
// the variables' belief means c (x = c + u) its precision J and right-hand side h; here J = L L' (Cholesky), δ = J⁻¹ h and Σ = J⁻¹ =
// L⁻ᵀ L⁻¹ (2d x 2d; an observed end is an identity block with h = 0, zeroed in Σ afterwards).  The residual r = x_out - A x_in - b
// has E[r] = r(c) + C δ and Cov(r) = C Σ C' with C = [I, -A]: every statistic is of the size of the noise, nothing is cancelled.
//
//   k_ev_var       (cx_evidence.hip) one thread per variable: the belief means and precisions (scratch W)
//   k_fs_belief    one thread per requested factor: its row (2d means | 2d x 2d covariance)
//   k_fs_stats     one 64-thread block per chunk of at most 64 factors of ONE group (a work list sorted by group, then factor
//                  index): each thread writes its factor's 1 + 2d + 3d² statistics and two flags to LDS, lane j adds up entry j of
//                  the 64 in thread order (compensated) and writes the chunk's row (sums | compensations)
//   k_fs_reduce    the rows of one group in runs of at most 64, in index order, level after level until one row per group remains
// No atomics: two calls on one state are bit-identical.
#include "cx_evidence_core.h"

namespace cx {
namespace fs {

using ev::Lay;
using ev::kLog2Pi;

constexpr int kW = 64;         // threads per block of the factor passes = factors per chunk = rows per reduction run

template <int D>
struct SLay {
    static constexpr int NS = 1 + 2 * D + 3 * D * D;     // n | Σ E[r] | Σ E[x_in] | Σ E[r r'] | Σ E[r x_in'] | Σ E[x_in x_in']
    static constexpr int NW = NS + 2;                     // + factors with an undefined input, factors whose belief is not pd
    static constexpr int NB = 2 * D + 4 * D * D;          // a belief row: means | covariance
};

// the joint belief of pair row p, centred: centre c (the belief means of the free ends, the data of the observed ones), offset dl
// (zero on observed ends) and covariance S (zero rows and columns on observed ends); also the factor's A and residual at the
// centre, rc = c_out - A c_in - b (in B).  Returns 0, 1 (an undefined input) or 2 (the belief is not positive definite).
template <int D>
__device__ __forceinline__ int pair_belief(int64_t p, const ev::PairTab &tab, const ev::Msgs &msg, ev::PairJoint<D> &B, double (&dl)[2 * D],
                                           double (&S)[2 * D][2 * D]) {
    constexpr int N = 2 * D;
    ev::pair_joint<D>(p, tab, msg, B);
    if (!B.ok) return 1;
    double logdet, quad;
    if (!ev::chol_quad<N>(B.J, B.h, logdet, quad)) return 2;
    ev::back_solve<N>(B.J, B.h, dl);
    ev::inv_lower<N>(B.J);
    ev::gram_lower<N>(B.J, S);      // Σ = L⁻ᵀ L⁻¹: its lower triangle, masked and mirrored below
#pragma unroll
    for (int i = 0; i < N; i++) {
        if (!(i < D ? B.fo : B.fi)) dl[i] = 0.0;
#pragma unroll
        for (int j = 0; j <= i; j++) {
            S[i][j] = (i < D ? B.fo : B.fi) && (j < D ? B.fo : B.fi) ? S[i][j] : 0.0;
            S[j][i] = S[i][j];
        }
    }
    return 0;
}

// ---- beliefs: one thread per requested pair row -----------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(kW) void k_fs_belief(int64_t n, const int32_t *__restrict__ rows, ev::PairTab tab, ev::Msgs msg, double *__restrict__ out) {
    constexpr int N = 2 * D;
    const int64_t i = (int64_t)blockIdx.x * kW + threadIdx.x;
    if (i >= n) return;
    const double nan = __builtin_nan("");
    ev::PairJoint<D> B;
    double dl[N], S[N][N];
    const int st = pair_belief<D>(rows[i], tab, msg, B, dl, S);
    double *o = out + i * SLay<D>::NB;
#pragma unroll
    for (int k = 0; k < N; k++) o[k] = st ? nan : B.c[k] + dl[k];
#pragma unroll
    for (int k = 0; k < N; k++)
#pragma unroll
        for (int j = 0; j < N; j++) o[N + k * N + j] = st ? nan : S[k][j];
}

// ---- statistics: one block per chunk of one group; row k of part = sums[NW] | compensations[NW] -----------------------------------
template <int D>
__global__ __launch_bounds__(kW) void k_fs_stats(const int32_t *__restrict__ cbeg, const int32_t *__restrict__ items, ev::PairTab tab, ev::Msgs msg,
                                                 double *__restrict__ part) {
    constexpr int N = 2 * D, NW = SLay<D>::NW, P = kW + 1;     // (P: entry j of the 64 threads spreads over the banks)
    __shared__ double sv[NW * P];
    const int t = threadIdx.x;
    const int64_t i = (int64_t)cbeg[blockIdx.x] + t;
    double *v = sv + t;                                        // entry k of this thread at v[k * P]
    if (i < cbeg[blockIdx.x + 1]) {
        ev::PairJoint<D> B;
        double dl[N], S[N][N];
        const int st = pair_belief<D>(items[i], tab, msg, B, dl, S);
        const double (&A)[D][D] = B.A;
        v[0] = 1.0;
        if (st) {
#pragma unroll
            for (int k = 1; k < NW; k++) v[k * P] = 0.0;
            v[(NW - 2) * P] = st == 1 ? 1.0 : 0.0;
            v[(NW - 1) * P] = st == 2 ? 1.0 : 0.0;
        } else {
            double er[D], ex[D], CS[D][N];          // E[r], E[x_in], C Σ
#pragma unroll
            for (int p = 0; p < D; p++) {
                double t0 = B.rc[p] + dl[p];
#pragma unroll
                for (int q = 0; q < D; q++) t0 -= A[p][q] * dl[D + q];
                er[p] = t0;
                ex[p] = B.c[D + p] + dl[D + p];
#pragma unroll
                for (int k = 0; k < N; k++) {
                    double u = S[p][k];
#pragma unroll
                    for (int q = 0; q < D; q++) u -= A[p][q] * S[D + q][k];
                    CS[p][k] = u;
                }
            }
            constexpr int o_r = 1, o_x = 1 + D, o_rr = 1 + 2 * D, o_rx = o_rr + D * D, o_xx = o_rx + D * D;
#pragma unroll
            for (int p = 0; p < D; p++) {
                v[(o_r + p) * P] = er[p];
                v[(o_x + p) * P] = ex[p];
#pragma unroll
                for (int s = 0; s < D; s++) {
                    double u = CS[p][s];
#pragma unroll
                    for (int q = 0; q < D; q++) u -= CS[p][D + q] * A[s][q];
                    v[(o_rr + p * D + s) * P] = u + er[p] * er[s];
                    v[(o_rx + p * D + s) * P] = CS[p][D + s] + er[p] * ex[s];
                    v[(o_xx + p * D + s) * P] = S[D + p][D + s] + ex[p] * ex[s];
                }
            }
            v[(NW - 2) * P] = 0.0;
            v[(NW - 1) * P] = 0.0;
        }
    } else {
#pragma unroll
        for (int k = 0; k < NW; k++) v[k * P] = 0.0;
    }
    __syncthreads();
    if (t < NW) {
        double s = 0.0, cc = 0.0;
        for (int k = 0; k < kW; k++) ev::neu(s, cc, sv[t * P + k]);
        double *o = part + (int64_t)blockIdx.x * 2 * NW;
        o[t] = s;
        o[NW + t] = cc;
    }
}

// ---- one reduction level: output row k = the rows seg[k] .. seg[k + 1] - 1 of `in`, in index order --------------------------------
__global__ __launch_bounds__(kW) void k_fs_reduce(const int32_t *__restrict__ seg, int nw, const double *__restrict__ in, double *__restrict__ out) {
    const int t = threadIdx.x;
    if (t >= nw) return;
    const int32_t r0 = seg[blockIdx.x], r1 = seg[blockIdx.x + 1];
    double s = 0.0, c = 0.0;
    for (int32_t r = r0; r < r1; r++) {
        const double *row = in + (int64_t)r * 2 * nw;
        ev::neu(s, c, row[t]);
        c += row[nw + t];
    }
    double *o = out + (int64_t)blockIdx.x * 2 * nw;
    o[t] = s;
    o[nw + t] = c;
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
struct Cache {
    // the grouping the lists were built for
    bool valid = false, explicit_ids = false;
    uint64_t epoch = ~0ull;
    int64_t n_groups = 0;
    std::vector<int64_t> ids, groups;
    // the lists: items (pair rows by group, then factor index), chunks, the reduction levels
    int64_t n_items = 0, n_chunks = 0;
    std::vector<int64_t> level_off, level_n;       // per level: offset into d_seg, output rows
    std::vector<int64_t> out_group;                // the group of every final row (ascending)
    DevBuf<int32_t> d_items, d_cbeg, d_seg;
    DevBuf<double> d_rows[2];
    double *h_rows = nullptr;                      // pinned: the final rows
    // beliefs (grown on demand)
    DevBuf<int32_t> d_brows;
    DevBuf<double> d_bout;
    Cache() = default;
    Cache(const Cache &) = delete;
    ~Cache() { if (h_rows) (void)hipHostFree(h_rows); }
};

void free_lists(Cache &L) {
    reset_all(L.d_items, L.d_cbeg, L.d_seg, L.d_rows[0], L.d_rows[1]);
    if (L.h_rows) (void)hipHostFree(L.h_rows);
    L.h_rows = nullptr;
    L.valid = false;
}

Cache &cache_of(cx_handle *h) {
    if (!h->learn) h->learn.reset(new Cache());
    return *h->learn;
}

// the group of every pair row (-1: not counted), checked; the caller's arrays (explicit) or the parameter sets (ids == null, dim > 1)
int32_t assign_groups(cx_handle *h, const ev::Cache &E, int64_t n, const int64_t *ids, const int64_t *groups, int64_t n_groups,
                      std::vector<int32_t> &grp) {
    using namespace cxh;
    const std::string who = "cx_factor_statistics";
    const int d = h->cfg.dim;
    grp.assign((size_t)E.n_pair, -1);
    if (!ids) {
        // one group per parameter set; a set that a factor of more than two variables also reads would get partial statistics
        std::vector<int64_t> kary_fac_of_set;
        for (int64_t r = 0; r < h->n_kary; r++)
            for (int e = 0; e < 8; e++) {
                if (h->kary_slot[8 * r + e] < 0) continue;
                const int32_t s = h->kary_pset[8 * r + e];
                if (s >= 0 && (size_t)s >= kary_fac_of_set.size()) kary_fac_of_set.resize((size_t)s + 1, -1);
                if (s >= 0 && kary_fac_of_set[(size_t)s] < 0) kary_fac_of_set[(size_t)s] = r;
            }
        for (int64_t p = 0; p < E.n_pair; p++) {
            const int32_t s = E.pair_ps[(size_t)p];
            if (s >= n_groups)
                return fail(h, CX_ERR_INVALID_ARGUMENT, who + ": factor " + std::to_string(h->fac_ids[(size_t)E.pair_fac[(size_t)p]]) + " uses parameter set " +
                            std::to_string(s) + ": n_groups must exceed every set in use");
            if ((size_t)s < kary_fac_of_set.size() && kary_fac_of_set[(size_t)s] >= 0)
                return fail(h, CX_ERR_UNSUPPORTED, who + ": parameter set " + std::to_string(s) + " is also read by a factor of more than two variables (its " +
                            "statistics would be incomplete)");
            grp[(size_t)p] = s;
        }
        (void)d;
        return CX_OK;
    }
    std::vector<int64_t> first((size_t)n_groups, -1);       // first pair row of every group
    for (int64_t i = 0; i < n; i++) {
        const int64_t f = find_factor(h, ids[i]);
        if (f < 0) return fail(h, CX_ERR_NOT_FOUND, who + ": no factor " + std::to_string(ids[i]));
        const int64_t g = groups[i];
        if (g < -1 || g >= n_groups) return fail(h, CX_ERR_INVALID_ARGUMENT, who + ": group " + std::to_string(g) + " of factor " + std::to_string(ids[i]) + " is not in -1 .. n_groups - 1");
        if (g < 0) continue;
        const int32_t p = E.row_of_fac[(size_t)f];
        if (p < 0) return fail(h, CX_ERR_UNSUPPORTED, who + ": factor " + std::to_string(ids[i]) + " is not a Gaussian factor of two variables");
        if (grp[(size_t)p] >= 0) return fail(h, CX_ERR_INVALID_ARGUMENT, who + ": factor " + std::to_string(ids[i]) + " is listed twice");
        grp[(size_t)p] = (int32_t)g;
        const int64_t q = first[(size_t)g];
        if (q < 0) { first[(size_t)g] = p; continue; }
        bool same;
        if (d > 1) same = E.pair_ps[(size_t)p] == E.pair_ps[(size_t)q];
        else {
            const int64_t fp = E.pair_fac[(size_t)p], fq = E.pair_fac[(size_t)q];
            const double *a = &h->fac_params[(size_t)fp * CX_NPARAM], *b = &h->fac_params[(size_t)fq * CX_NPARAM];
            const int32_t kp = h->fac_kind[(size_t)fp], kq = h->fac_kind[(size_t)fq];
            same = kp == kq && (kp != CX_FACTOR_GAUSS_LINEAR || (a[1] == b[1] && a[2] == b[2]));
        }
        if (!same)
            return fail(h, CX_ERR_INVALID_ARGUMENT, who + ": factors " + std::to_string(h->fac_ids[(size_t)E.pair_fac[(size_t)q]]) + " and " + std::to_string(ids[i]) +
                        " are in group " + std::to_string(g) + " but do not share their A (dim > 1: parameter set; dim 1: kind, a and b)");
    }
    return CX_OK;
}

// the work list, the chunks and the reduction levels of one grouping (O(n_pair) on the host, one upload)
int32_t build_lists(cx_handle *h, Cache &L, const std::vector<int32_t> &grp, int64_t n_groups, int nw) {
    using namespace cxh;
    std::vector<int64_t> cnt((size_t)n_groups + 1, 0);
    for (int32_t g : grp) if (g >= 0) cnt[(size_t)g + 1]++;
    for (int64_t g = 0; g < n_groups; g++) cnt[(size_t)g + 1] += cnt[(size_t)g];
    const int64_t n_items = cnt[(size_t)n_groups];
    std::vector<int32_t> items((size_t)n_items);
    {
        std::vector<int64_t> at(cnt.begin(), cnt.end() - 1);
        for (size_t p = 0; p < grp.size(); p++) if (grp[p] >= 0) items[(size_t)at[(size_t)grp[p]]++] = (int32_t)p;      // factor order within a group
    }
    std::vector<int32_t> cbeg, seg;
    std::vector<int64_t> row_group;
    for (int64_t g = 0; g < n_groups; g++)
        for (int64_t a = cnt[(size_t)g]; a < cnt[(size_t)g + 1]; a += kW) { cbeg.push_back((int32_t)a); row_group.push_back(g); }
    cbeg.push_back((int32_t)n_items);
    L.level_off.clear(); L.level_n.clear();
    int64_t max_rows = (int64_t)row_group.size();
    for (;;) {
        bool more = false;
        for (size_t r = 1; r < row_group.size() && !more; r++) more = row_group[r] == row_group[r - 1];
        if (!more) break;
        std::vector<int64_t> next;
        const int64_t off = (int64_t)seg.size();
        size_t r = 0;
        while (r < row_group.size()) {
            size_t e = r;
            while (e < row_group.size() && row_group[e] == row_group[r]) e++;
            for (size_t a = r; a < e; a += kW) { seg.push_back((int32_t)a); next.push_back(row_group[r]); }
            r = e;
        }
        seg.push_back((int32_t)row_group.size());
        L.level_off.push_back(off);
        L.level_n.push_back((int64_t)next.size());
        row_group.swap(next);
    }
    free_lists(L);
    int32_t rc;
    if ((rc = dev_upload(h, &L.d_items, items)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &L.d_cbeg, cbeg)) != CX_OK) return rc;
    if (!seg.empty() && (rc = dev_upload(h, &L.d_seg, seg)) != CX_OK) return rc;
    const int64_t rows = std::max<int64_t>(max_rows, 1) * 2 * nw;
    if ((rc = dev_alloc(h, &L.d_rows[0], rows)) != CX_OK) return rc;
    if ((rc = dev_alloc(h, &L.d_rows[1], rows)) != CX_OK) return rc;
    CX_HIP(h, hipHostMalloc((void **)&L.h_rows, (size_t)(std::max<int64_t>((int64_t)row_group.size(), 1) * 2 * nw) * sizeof(double), hipHostMallocDefault));
    CX_HIP(h, hipStreamSynchronize(h->stream));      // (the host vectors die here)
    L.n_items = n_items;
    L.n_chunks = (int64_t)cbeg.size() - 1;
    L.out_group = row_group;
    return CX_OK;
}

template <int D>
void launch_stats(cx_handle *h, const ev::Cache &E, const Cache &L, int &final_buf) {
    constexpr int NW = SLay<D>::NW;
    final_buf = 0;
    if (L.n_chunks == 0) return;
    hipLaunchKernelGGL(k_fs_stats<D>, dim3((unsigned)L.n_chunks), dim3(kW), 0, h->stream, L.d_cbeg, L.d_items, E.pair_tab(), ev::msgs_of(h, E), L.d_rows[0]);
    for (size_t l = 0; l < L.level_n.size(); l++) {
        hipLaunchKernelGGL(k_fs_reduce, dim3((unsigned)L.level_n[l]), dim3(kW), 0, h->stream, L.d_seg + L.level_off[l], NW, L.d_rows[final_buf],
                           L.d_rows[1 - final_buf]);
        final_buf = 1 - final_buf;
    }
}

template <int D>
void launch_beliefs(cx_handle *h, const ev::Cache &E, const Cache &L, int64_t n) {
    hipLaunchKernelGGL(k_fs_belief<D>, dim3((unsigned)((n + kW - 1) / kW)), dim3(kW), 0, h->stream, n, L.d_brows, E.pair_tab(), ev::msgs_of(h, E), L.d_bout);
}

int nw_of(int d) { return ev::with_dim(d, [](auto D) { return SLay<D()>::NW; }); }
int nb_of(int d) { return ev::with_dim(d, [](auto D) { return SLay<D()>::NB; }); }

}  // namespace fs

template <> void Deleter<fs::Cache>::operator()(fs::Cache *L) const { delete L; }

}  // namespace cx

using namespace cxh;

extern "C" int32_t cx_factor_beliefs(cx_handle *h, int64_t n, const int64_t *factor_ids, double *out) {
    try {
        cx::ev::Cache *Ep = nullptr;
        int32_t rc;
        const char *bad = n >= 0 && (n == 0 || (factor_ids && out)) ? nullptr : "null argument or negative count";
        if ((rc = cx::ev::prepare(h, "cx_factor_beliefs", bad, Ep)) != CX_OK) return rc;
        if (n == 0) return CX_OK;
        cx::ev::Cache &E = *Ep;
        cx::fs::Cache &L = cx::fs::cache_of(h);
        std::vector<int32_t> rows((size_t)n);
        for (int64_t i = 0; i < n; i++) {
            const int64_t f = find_factor(h, factor_ids[i]);
            if (f < 0) return fail(h, CX_ERR_NOT_FOUND, "cx_factor_beliefs: no factor " + std::to_string(factor_ids[i]));
            rows[(size_t)i] = E.row_of_fac[(size_t)f];
            if (rows[(size_t)i] < 0) return fail(h, CX_ERR_UNSUPPORTED, "cx_factor_beliefs: factor " + std::to_string(factor_ids[i]) + " is not a Gaussian factor of two variables");
        }
        const int d = h->cfg.dim, nb = cx::fs::nb_of(d);
        if ((rc = L.d_brows.ensure(h, n)) != CX_OK || (rc = L.d_bout.ensure(h, n * nb)) != CX_OK) return rc;
        CX_HIP(h, hipMemcpyAsync(L.d_brows, rows.data(), (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
        cx::ev::var_pass(h, E);
        cx::ev::with_dim(d, [&](auto D) { cx::fs::launch_beliefs<D()>(h, E, L, n); });
        CX_HIP(h, hipGetLastError());
        CX_HIP(h, hipMemcpyAsync(out, L.d_bout, (size_t)(n * nb) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        CX_HIP(h, hipStreamSynchronize(h->stream));
        return CX_OK;
    } catch (const std::bad_alloc &) { return fail(h, CX_ERR_OUT_OF_MEMORY, "cx_factor_beliefs: host allocation failed"); }
}

extern "C" int32_t cx_factor_statistics(cx_handle *h, int64_t n, const int64_t *factor_ids, const int64_t *groups, int64_t n_groups, double *out,
                                        int64_t *counts4) {
    try {
        cx::ev::Cache *Ep = nullptr;
        int32_t rc;
        const char *bad = !(out && counts4 && n_groups > 0) ? "null output or n_groups < 1"
                          : !(factor_ids ? (n >= 0 && (n == 0 || groups)) : !groups)
                              ? "factor_ids and groups go together (n >= 0), or both null for the parameter-set grouping"
                              : nullptr;
        if ((rc = cx::ev::prepare(h, "cx_factor_statistics", bad, Ep)) != CX_OK) return rc;
        const int d = h->cfg.dim;
        CX_REQUIRE(h, factor_ids || d > 1, CX_ERR_INVALID_ARGUMENT,
                   "cx_factor_statistics: dim 1 has per-factor parameters: name the factors and their groups (factor_ids, groups)");
        cx::ev::Cache &E = *Ep;
        cx::fs::Cache &L = cx::fs::cache_of(h);
        const int nw = cx::fs::nw_of(d), ns = nw - 2;
        // an explicit grouping is compared with the cached one (O(n) on the host); a new one is checked and its lists are rebuilt
        const bool same = L.valid && L.epoch == h->param_epoch && L.n_groups == n_groups && L.explicit_ids == (factor_ids != nullptr) &&
                          (!factor_ids || ((int64_t)L.ids.size() == n && std::equal(factor_ids, factor_ids + n, L.ids.begin()) &&
                                           std::equal(groups, groups + n, L.groups.begin())));
        if (!same) {
            L.valid = false;
            std::vector<int32_t> grp;
            if ((rc = cx::fs::assign_groups(h, E, n, factor_ids, groups, n_groups, grp)) != CX_OK) return rc;
            if ((rc = cx::fs::build_lists(h, L, grp, n_groups, nw)) != CX_OK) return rc;
            L.explicit_ids = factor_ids != nullptr;
            L.ids.assign(factor_ids, factor_ids ? factor_ids + n : factor_ids);
            L.groups.assign(groups, groups ? groups + n : groups);
            L.n_groups = n_groups;
            L.epoch = h->param_epoch;
            L.valid = true;
        }
        int fb = 0;
        cx::ev::var_pass(h, E);
        cx::ev::with_dim(d, [&](auto D) { cx::fs::launch_stats<D()>(h, E, L, fb); });
        CX_HIP(h, hipGetLastError());
        const int64_t nrows = L.n_chunks ? (int64_t)L.out_group.size() : 0;
        if (nrows) CX_HIP(h, hipMemcpyAsync(L.h_rows, L.d_rows[fb], (size_t)(nrows * 2 * nw) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        CX_HIP(h, hipStreamSynchronize(h->stream));
        std::fill(out, out + n_groups * ns, 0.0);
        for (int k = 0; k < 4; k++) counts4[k] = 0;
        for (int64_t r = 0; r < nrows; r++) {
            const double *row = L.h_rows + r * 2 * nw;
            double *o = out + L.out_group[(size_t)r] * ns;
            const int64_t n_undef = (int64_t)(row[nw - 2] + row[2 * nw - 2]), n_npd = (int64_t)(row[nw - 1] + row[2 * nw - 1]);
            counts4[0] += (int64_t)(row[0] + row[nw]);
            counts4[1] += 1;
            counts4[2] += n_undef;
            counts4[3] += n_npd;
            o[0] = row[0] + row[nw];
            for (int k = 1; k < ns; k++) o[k] = n_undef + n_npd > 0 ? kNaN : row[k] + row[nw + k];
        }
        return CX_OK;
    } catch (const std::bad_alloc &) { return fail(h, CX_ERR_OUT_OF_MEMORY, "cx_factor_statistics: host allocation failed"); }
}
