// cx_disturb_mfma.hip — cx_factor_disturbances_mfma and cx_factor_disturbance_rows_mfma: the smoothed disturbance of every two-variable
// x_out = A x_in + b + w, w ~ N(0, Q), factor at the matrix-core dims (cx_create dim 5 .. 64): E[w | data], Cov(w | data) and the two
// scalars t = E[w'Q⁻¹w | data], q = E[w]'Q⁻¹E[w], PER FACTOR.  DESIGN.md §4v.
//
// The arithmetic is cx_factor_statistics_mfma's (lm_factors, cx_learn_mfma_core.h: the residual r = x_out - A x_in - b IS w, formed as
// such, K = M⁻¹Λ_o A) in its third mode: a row is written where the statistics add it into a group's sum.  The kernel entry points are
// in this translation unit and not beside k_lm_factors: apart, those instances keep their registers (profiles/factor_disturbances_mfma.md).
//
// At most max_waves(KD) waves per launch, each with the workspace of its index and a contiguous run of the launch's rows; (t, status) and
// the scores go to whole-call arrays at the row's index, the payload through the bounded row buffer (mfr::stream_rows: one launch per
// chunk, nothing waits between chunks), mfr::k_status_part folds 256 rows into an ev::Part and ev::final_sum adds the parts in index
// order: no atomics, two calls on one state are bit-identical, and neither the total nor a row depends on how the rows are cut into
// chunks and waves, on `out` being asked for, or on what else is in the list.
#include "cx_learn_mfma_core.h"

namespace cx {
namespace lm {

template <int NT, int WAVES_PER_SIMD>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES_PER_SIMD, WAVES_PER_SIMD)))
void k_lm_disturb(const int nwave, const int row0, const int n, const int32_t *__restrict__ items, const int32_t *__restrict__ rec,
                  const int32_t *__restrict__ srcs, const double *__restrict__ ptab, const double *__restrict__ btab, const double *__restrict__ atab,
                  const double *__restrict__ f2v, const double *__restrict__ v2f, const int u, double *ws_all, double *rval, uint8_t *rflag,
                  double *scores, double *__restrict__ out) {
    RowsOut rw;
    rw.row0 = row0; rw.n = n; rw.rval = rval; rw.scores = scores; rw.rflag = rflag;
    lm_factors<NT, kDisturbances, false>(nwave, nullptr, nullptr, items, rec, srcs, ptab, btab, atab, f2v, v2f, nullptr, nullptr, u, ws_all, nullptr, nullptr, out, rw);
}
// the factors of a handle with factor offsets
template <int NT, int WAVES_PER_SIMD>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES_PER_SIMD, WAVES_PER_SIMD)))
void k_lm_disturb_off(const int nwave, const int row0, const int n, const int32_t *__restrict__ items, const int32_t *__restrict__ rec,
                      const int32_t *__restrict__ srcs, const double *__restrict__ ptab, const double *__restrict__ btab, const double *__restrict__ atab,
                      const double *__restrict__ f2v, const double *__restrict__ v2f, const double *__restrict__ goff, const double *__restrict__ boff,
                      const int u, double *ws_all, double *rval, uint8_t *rflag, double *scores, double *__restrict__ out) {
    RowsOut rw;
    rw.row0 = row0; rw.n = n; rw.rval = rval; rw.scores = scores; rw.rflag = rflag;
    lm_factors<NT, kDisturbances, true>(nwave, nullptr, nullptr, items, rec, srcs, ptab, btab, atab, f2v, v2f, goff, boff, u, ws_all, nullptr, nullptr, out, rw);
}

// rows [row0, row0 + n) of the request (d_rows: their payload, or null)
static void launch_rows(cx_handle *h, Cache &C, int64_t row0, int64_t n, double *d_rows) {
    if (!n) return;
    const int u = mfr::user_dim(h), nwave = (int)std::min<int64_t>(n, max_waves(h->cfg.dim));
    mfr::for_tiles(h->cfg.dim, [&](auto nt) {
        constexpr int NT = decltype(nt)::value, W = NT == 4 ? 1 : 2;      // (the statistics instances' waves per SIMD)
        if (h->has_offsets)      // cx_set_factor_offsets_mfma: the instances that read g and b
            hipLaunchKernelGGL((k_lm_disturb_off<NT, W>), dim3((unsigned)nwave), dim3(64), 0, h->stream, nwave, (int)row0, (int)n, C.d_ditems, C.d_rec, C.d_srcs,
                               h->d_ptab, h->d_ptab_bt, C.atab.d, h->d_mv_f2v, h->d_mv_v2f, (const double *)h->d_off_g, (const double *)h->d_off_b, u, C.d_ws,
                               C.d_drval, C.d_drflag, C.d_dscores, d_rows);
        else
            hipLaunchKernelGGL((k_lm_disturb<NT, W>), dim3((unsigned)nwave), dim3(64), 0, h->stream, nwave, (int)row0, (int)n, C.d_ditems, C.d_rec, C.d_srcs,
                               h->d_ptab, h->d_ptab_bt, C.atab.d, h->d_mv_f2v, h->d_mv_v2f, u, C.d_ws, C.d_drval, C.d_drflag, C.d_dscores, d_rows);
    });
}

// the factor indices of the rows, checked: the caller's, in the caller's order, or every covered factor in ascending factor id
static int32_t list_rows(cx_handle *h, const Cache &C, const std::string &who, int64_t n, const int64_t *ids, std::vector<int32_t> &fac) {
    using namespace cxh;
    fac.clear();
    if (!ids) {
        if (C.unsupported_fac >= 0) return mfr::refuse_factor(h, who, C.unsupported_fac);
        for (int64_t f = 0; f < h->nf; f++) if (C.kind[(size_t)f] >= 0) fac.push_back((int32_t)f);
        return CX_OK;
    }
    for (int64_t i = 0; i < n; i++) {
        const int64_t f = find_factor(h, ids[i]);
        if (f < 0) return fail(h, CX_ERR_NOT_FOUND, who + ": no factor " + std::to_string(ids[i]));
        if (C.kind[(size_t)f] < 0) return fail(h, CX_ERR_UNSUPPORTED, who + ": " + no_pair(ids[i]));
        fac.push_back((int32_t)f);
    }
    return CX_OK;
}

static const char *kSmallDims = "cx_factor_statistics sums these residual moments per group; the per-factor call exists at dim 5 .. 64 only";

}  // namespace lm
}  // namespace cx

using namespace cxh;

extern "C" int32_t cx_factor_disturbance_rows_mfma(cx_handle *h, int64_t cap, int64_t *factor_ids, int64_t *n_rows) {
    try {
        namespace lm = cx::lm;
        const std::string who = "cx_factor_disturbance_rows_mfma";
        lm::Cache *Cp = nullptr;
        int32_t rc;
        const char *bad = n_rows && cap >= 0 && (cap == 0 || factor_ids) ? nullptr : "null argument or negative capacity";
        if ((rc = lm::prepare(h, who, lm::kSmallDims, bad, Cp)) != CX_OK) return rc;
        std::vector<int32_t> fac;
        if ((rc = lm::list_rows(h, *Cp, who, 0, nullptr, fac)) != CX_OK) return rc;
        *n_rows = (int64_t)fac.size();
        for (int64_t i = 0; i < std::min<int64_t>(cap, *n_rows); i++) factor_ids[i] = h->fac_ids[(size_t)fac[(size_t)i]];
        return CX_OK;
    } catch (const std::bad_alloc &) { return fail(h, CX_ERR_OUT_OF_MEMORY, "cx_factor_disturbance_rows_mfma: host allocation failed"); }
}

extern "C" int32_t cx_factor_disturbances_mfma(cx_handle *h, int64_t n, const int64_t *factor_ids, double *out, double *scores, double *total,
                                               int64_t *counts4) {
    try {
        namespace lm = cx::lm;
        namespace mfr = cx::mfr;
        const std::string who = "cx_factor_disturbances_mfma";
        lm::Cache *Cp = nullptr;
        int32_t rc;
        const char *bad = !counts4 ? "counts4 is null" : factor_ids && n < 0 ? "negative count" : nullptr;
        if ((rc = lm::prepare(h, who, lm::kSmallDims, bad, Cp)) != CX_OK) return rc;
        lm::Cache &C = *Cp;      // (a new one when vinfo_epoch moved: its rows_key is not valid)
        if (!C.rows_key.matches(0, n, factor_ids)) {
            C.rows_key.valid = false;
            std::vector<int32_t> fac;
            if ((rc = lm::list_rows(h, C, who, n, factor_ids, fac)) != CX_OK) return rc;
            const int64_t m = (int64_t)fac.size();
            CX_REQUIRE(h, m < (int64_t)0x3fffff00, CX_ERR_UNSUPPORTED, who + ": more than 2^30 rows");
            C.n_drows = m;
            if (fac.empty()) fac.push_back(0);      // (never read: no wave is launched)
            if ((rc = dev_upload(h, &C.d_ditems, fac)) != CX_OK) return rc;
            if ((rc = C.d_drval.ensure(h, std::max<int64_t>(m, 1))) != CX_OK || (rc = C.d_drflag.ensure(h, std::max<int64_t>(m, 1))) != CX_OK ||
                (rc = C.d_dscores.ensure(h, std::max<int64_t>(2 * m, 1))) != CX_OK || (rc = C.d_dpart.ensure(h, (m + mfr::kTB - 1) / mfr::kTB + 1)) != CX_OK)
                return rc;
            CX_HIP(h, hipStreamSynchronize(h->stream));      // (the local host vector dies here)
            C.rows_key.remember(0, n, factor_ids);
        }
        const int u = mfr::user_dim(h);
        const int64_t nr = C.n_drows;
        if ((rc = C.d_ws.ensure(h, std::min<int64_t>(std::max<int64_t>(nr, 1), lm::max_waves(h->cfg.dim)) * lm::ws_doubles(h->cfg.dim))) != CX_OK) return rc;
        // the payload a chunk at a time through a bounded device buffer; the (value, status) and score arrays cover every row
        if (out) rc = mfr::stream_rows(h, nr, (int64_t)u + (int64_t)u * u, C.d_dout, out, [&](int64_t r0, int64_t m, double *d) { lm::launch_rows(h, C, r0, m, d); });
        else lm::launch_rows(h, C, 0, nr, nullptr);
        if (rc != CX_OK) return rc;
        CX_HIP(h, hipGetLastError());
        if (scores && nr) CX_HIP(h, hipMemcpyAsync(scores, C.d_dscores, (size_t)(2 * nr) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        double sum;
        if ((rc = C.dtotals.read_rows(h, nr, C.d_drval, C.d_drflag, C.d_dpart, counts4, &sum)) != CX_OK) return rc;      // (waits for the stream)
        if (total) *total = sum;
        return CX_OK;
    } catch (const std::bad_alloc &) { return fail(h, CX_ERR_OUT_OF_MEMORY, "cx_factor_disturbances_mfma: host allocation failed"); }
}
