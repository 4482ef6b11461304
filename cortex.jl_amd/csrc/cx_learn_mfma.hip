// cx_learn_mfma.hip — cx_factor_beliefs_mfma and cx_factor_statistics_mfma: the joint posterior of every two-variable
// x_out = A x_in + N(0, Q) factor and the EM statistics of cx_factor_statistics at the matrix-core dims (cx_create dim
// 5 .. 64, internal tiles of 16 / 32 / 64), from the stored factor→variable messages and the caller's data.  DESIGN.md §4n.
//
// ONE WAVE per factor, on the pieces of cx_log_evidence_mfma (cx_evidence_mfma_core.h): sums of message records, the blocked Cholesky
// with U in registers, block-column solves U^-T X.  What a factor needs besides is explicit inverses and a handful of KD x KD products;
// at 4 x 4 tiles they do not fit in registers beside U, so every intermediate matrix is PARKED in a workspace of the wave's own in device
// memory (six KD x KD matrices, row-major, plain vector loads and stores; a workgroup-scope fence between a pass that writes one and the
// pass that reads it — the wave is alone in its workgroup) and every product is X'Y read tile by tile from there: tts() contracts over
// tile rows, so the algebra below is arranged to need no other form.
//
// With (P, B, C) = (Q⁻¹, A'Q⁻¹, A'Q⁻¹A) the rule table towards IN, bt = B' = Q⁻¹A, and the leave-one-out messages m_{out→a} = (Λ_o, η_o),
// m_{in→a} = (Λ_i, η_i) summed directly from the other stored messages (opaque ones included):
//   1. OUT goes first:  M = Λ_o + P = U'U,  z = U^-T η_o,  W_M = U^-T (solve against the identity),  Yt = U^-T bt,
//                       M⁻¹ = W_M'W_M,  m0 = M⁻¹η_o = W_M'z,  Λ' = C - Yt'Yt,  η' = Yt'z          (x_out | x_in ~ N(m0 + G x_in, M⁻¹), G = M⁻¹bt)
//   2. IN:              S = Λ_i + Λ' = U_S'U_S,  W_S = U_S^-T,  Σ_ii = W_S'W_S,  μ_i = W_S'(U_S^-T (η_i + η'))
//   3. the pair (f, x_in) with f = m0 + J x_in + N(0, M⁻¹):   N = Σ_ii J' = Cov(x_in, f),   E[f] = m0 + J μ_i,   Cov(f) = M⁻¹ + J N
//        beliefs      f = x_out:           J' = B M⁻¹ = bt'M⁻¹
//        statistics   f = r = x_out - A x_in: J = G - A = -K with K = M⁻¹Λ_o A formed AS SUCH (J' = -(Λ_o A)'M⁻¹): a flat OUT leaf has
//                     Λ_o = 0, K = 0 and Cov(r) = M⁻¹ = Q to the rounding of one inverse; nothing of the size of A Σ_ii A' is cancelled
//   an observed OUT end (datum y):  m0 = y, M⁻¹ = 0, J = 0 (beliefs) or -A (statistics: r = y - A x_in), Λ' = C, η' = B y
//   an observed IN end (datum y):   μ_i = y, Σ_ii = 0; stage 1 as it is (E[x_out] = M⁻¹(η_o + bt y))
// Embedded dims: every matrix is block-diagonal (real block, identity block) and so is every product; rows and sums hold the real
// block only, d below is the user's.
// Factor offsets (cx_set_factor_offsets_mfma; OFF, entry points of their own): x_out = A x_in + b + N(0, Q) puts the linear terms g_out, g_in
//   (goff: by slot, [nslots][KD]) into the factor's potential — η_o + g_out enters stage 1, η_i + η' + g_in stage 2 (an observed OUT end:
//   η' = B y as before) — and the statistics' residual is r = x_out - A x_in - b: E[r] = m0 + J μ_i - b with the factor's own b (boff: by
//   slot, the same layout; it may differ within a group), Cov as it was.
// Undefined / not positive definite: cx_log_evidence_mfma's rules.  An input record (or datum) that is NaN: undefined; a failed pivot of
// either factorisation: not positive definite; with two free ends the inputs of the second stage are looked at themselves.
//
// k_lm_factors<NT, STATS>  a wave walks a contiguous run of PARTIALS (a partial: a contiguous run of factors of one group in the list
//                          sorted by group, then factor index) and adds each factor's 2d + 3d² moments, in order, to the partial's own
//                          row; beliefs: one factor per wave, its row written out
// k_lm_reduce              a group's partials added in index order
// No atomics; the cut into partials and waves depends on the grouping alone: two calls on one state are bit-identical (per handle).
// Sums are plain f64 in that fixed order (not compensated: a run is at most a few hundred noise-sized terms).
// Device workspace: at most W = max_waves(KD) wave workspaces of 6 KD² + 4 KD doubles (W = 1024 at KD = 64, 2048 below), and one row of
// 2d + 3d² doubles per partial, at most W + n_groups of them: it does not grow with the number of factors (KD = 64: 198,656 B + 99,328 B each,
// 305 MB plus n_groups rows at most; KD = 32: 154 MB; KD = 16: 39 MB).  cx_factor_beliefs_mfma goes through its list W factors at a time.
// lm_factors, its helpers and the Cache: cx_learn_mfma_core.h (shared with cx_disturb_mfma.hip, cx_factor_disturbances_mfma: its third mode).
#include "cx_learn_mfma_core.h"

namespace cx {
namespace lm {

template <int NT, bool STATS, int WAVES_PER_SIMD>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES_PER_SIMD, WAVES_PER_SIMD)))
void k_lm_factors(const int nwave, const int32_t *__restrict__ wbeg, const int32_t *__restrict__ pbeg, const int32_t *__restrict__ items,
                  const int32_t *__restrict__ rec, const int32_t *__restrict__ srcs, const double *__restrict__ ptab, const double *__restrict__ btab,
                  const double *__restrict__ atab, const double *__restrict__ f2v, const double *__restrict__ v2f, const int u, double *ws_all,
                  double *acc_all, int32_t *__restrict__ meta, double *__restrict__ out) {
    lm_factors<NT, STATS ? kStatistics : kBeliefs, false>(nwave, wbeg, pbeg, items, rec, srcs, ptab, btab, atab, f2v, v2f, nullptr, nullptr, u, ws_all, acc_all, meta, out);
}
// the factors of a handle with factor offsets
template <int NT, bool STATS, int WAVES_PER_SIMD>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES_PER_SIMD, WAVES_PER_SIMD)))
void k_lm_factors_off(const int nwave, const int32_t *__restrict__ wbeg, const int32_t *__restrict__ pbeg, const int32_t *__restrict__ items,
                      const int32_t *__restrict__ rec, const int32_t *__restrict__ srcs, const double *__restrict__ ptab, const double *__restrict__ btab,
                      const double *__restrict__ atab, const double *__restrict__ f2v, const double *__restrict__ v2f, const double *__restrict__ goff,
                      const double *__restrict__ boff, const int u, double *ws_all, double *acc_all, int32_t *__restrict__ meta, double *__restrict__ out) {
    lm_factors<NT, STATS ? kStatistics : kBeliefs, true>(nwave, wbeg, pbeg, items, rec, srcs, ptab, btab, atab, f2v, v2f, goff, boff, u, ws_all, acc_all, meta, out);
}

// row g of out = the rows gbeg[g] .. gbeg[g + 1] - 1 of acc, added in index order
__global__ __launch_bounds__(256) void k_lm_reduce(const int na, const int32_t *__restrict__ gbeg, const double *__restrict__ acc, double *__restrict__ out) {
    const int i = blockIdx.y * 256 + threadIdx.x, grp = blockIdx.x;
    if (i >= na) return;
    double s = 0.0;
    for (int p = gbeg[grp]; p < gbeg[grp + 1]; p++) s += acc[(int64_t)p * na + i];
    out[(int64_t)grp * na + i] = s;
}

// ---- host (the Cache: cx_learn_mfma_core.h) ----------------------------------------------------------------------------------------------------
static int32_t build(cx_handle *h, Cache &C, const std::string &who) {
    using namespace cxh;
    const int64_t nf = h->nf;
    mfr::Pairs P;
    mfr::pairs_of(h, P);
    std::vector<int32_t> rec((size_t)nf * 8, -1), srcs;
    C.kind.assign((size_t)nf, -1);
    C.set = P.set;
    C.unsupported_fac = P.unsupported_fac;
    for (int64_t f = 0; f < nf; f++) {
        if (h->fac_kind[f] == CX_FACTOR_OPAQUE) C.kind[f] = -2;
        if (P.so[f] < 0) continue;
        const bool oo = (h->vinfo[P.vo[f]] & kClamped) != 0, oi = (h->vinfo[P.vi[f]] & kClamped) != 0;
        const mfr::Run a = oo ? mfr::Run{} : mfr::other_slots(h, P.vo[f], P.so[f], srcs), b = oi ? mfr::Run{} : mfr::other_slots(h, P.vi[f], P.si[f], srcs);
        const int32_t r[8] = {(oo ? 1 : 0) | (oi ? 2 : 0), P.set[f], a.off, a.n, b.off, b.n, P.so[f], P.si[f]};
        std::copy(r, r + 8, &rec[(size_t)f * 8]);
        C.kind[f] = r[0];
    }
    CX_REQUIRE(h, nf < (int64_t)0x0fffffff && (int64_t)srcs.size() < (int64_t)0x7fffffff, CX_ERR_UNSUPPORTED, who + ": more than 2^28 factors");
    int32_t rc;
    if ((rc = dev_upload(h, &C.d_rec, rec)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &C.d_srcs, srcs)) != CX_OK) return rc;
    CX_HIP(h, hipStreamSynchronize(h->stream));      // (the local host vectors die here)
    C.built = true;
    C.vinfo_epoch = h->vinfo_epoch;
    C.group_key.valid = false;
    return CX_OK;
}

// [set][A | A'] at the internal dim (blockdiag(A, I) for an embedded one: cx_set_factor_matrices)
static void fill_atab(const cx_handle *h, std::vector<double> &at) {
    const size_t d = (size_t)h->cfg.dim, dd = d * d, ns = std::max<size_t>(h->psets.size(), 1);
    at.assign(ns * 2 * dd, cxh::kNaN);
    for (size_t s = 0; s < h->psets.size(); s++) {
        if (h->psets[s].empty()) continue;
        const double *A = h->psets[s].data();
        for (size_t r = 0; r < d; r++)
            for (size_t c = 0; c < d; c++) { at[s * 2 * dd + r * d + c] = A[r * d + c]; at[s * 2 * dd + dd + c * d + r] = A[r * d + c]; }
    }
}

// the refusals of a reader (cx_mfma_reader.h), the cache and its factor records
int32_t prepare(cx_handle *h, const std::string &who, const char *small_dims, const char *bad_args, Cache *&out) {
    using namespace cxh;
    int32_t rc;
    if ((rc = mfr::prepare(h, who, bad_args, {small_dims, "the variational and Beta-Bernoulli families have no Gaussian factor beliefs", "factors", true})) != CX_OK) return rc;
    if (h->learn_mfma && h->learn_mfma->vinfo_epoch != h->vinfo_epoch) h->learn_mfma.reset();      // other variables are observed
    if (!h->learn_mfma) h->learn_mfma.reset(new Cache());
    Cache &C = *h->learn_mfma;
    if (!C.built && (rc = build(h, C, who)) != CX_OK) { h->learn_mfma.reset(); return rc; }
    if ((rc = C.atab.refresh(h, [&](std::vector<double> &t) { fill_atab(h, t); })) != CX_OK) return rc;
    if ((rc = mv_ensure_chain_msgs(h)) != CX_OK) return rc;      // (every reader of d_mv_f2v calls this first)
    out = &C;
    return CX_OK;
}

std::string no_pair(int64_t id) { return "factor " + std::to_string(id) + " is no two-variable CX_FACTOR_GAUSS_LINEAR factor"; }

// the group of every factor index (-1: not counted), checked by cx_factor_statistics' rules
static int32_t assign_groups(cx_handle *h, const Cache &C, const std::string &who, int64_t n, const int64_t *ids, const int64_t *groups, int64_t n_groups,
                             std::vector<int32_t> &grp) {
    using namespace cxh;
    const int64_t nf = h->nf;
    grp.assign((size_t)nf, -1);
    if (!ids) {
        if (C.unsupported_fac >= 0) return mfr::refuse_factor(h, who, C.unsupported_fac);
        for (int64_t f = 0; f < nf; f++) {
            if (C.kind[f] < 0) continue;
            if (C.set[f] >= n_groups)
                return fail(h, CX_ERR_INVALID_ARGUMENT, who + ": factor " + std::to_string(h->fac_ids[f]) + " uses parameter set " + std::to_string(C.set[f]) +
                            ": n_groups must exceed every set in use");
            grp[f] = C.set[f];
        }
        return CX_OK;
    }
    std::vector<int64_t> first((size_t)n_groups, -1);
    for (int64_t i = 0; i < n; i++) {
        const int64_t f = find_factor(h, ids[i]);
        if (f < 0) return fail(h, CX_ERR_NOT_FOUND, who + ": no factor " + std::to_string(ids[i]));
        const int64_t g = groups[i];
        if (g < -1 || g >= n_groups) return fail(h, CX_ERR_INVALID_ARGUMENT, who + ": group " + std::to_string(g) + " of factor " + std::to_string(ids[i]) + " is not in -1 .. n_groups - 1");
        if (g < 0) continue;
        if (C.kind[f] < 0) return fail(h, CX_ERR_UNSUPPORTED, who + ": " + no_pair(ids[i]));
        if (grp[f] >= 0) return fail(h, CX_ERR_INVALID_ARGUMENT, who + ": factor " + std::to_string(ids[i]) + " is listed twice");
        grp[f] = (int32_t)g;
        const int64_t q = first[(size_t)g];
        if (q < 0) { first[(size_t)g] = f; continue; }
        if (C.set[f] != C.set[q])
            return fail(h, CX_ERR_INVALID_ARGUMENT, who + ": factors " + std::to_string(h->fac_ids[q]) + " and " + std::to_string(ids[i]) + " are in group " +
                        std::to_string(g) + " but do not share their A (one parameter set per group)");
    }
    return CX_OK;
}

// items by group, then factor index; a group's run cut into partials of at most ceil(items / max_waves) factors; the partials dealt to
// at most max_waves waves in contiguous runs
static int32_t build_lists(cx_handle *h, Cache &C, const std::vector<int32_t> &grp, int64_t n_groups, int na) {
    using namespace cxh;
    std::vector<int64_t> cnt((size_t)n_groups + 1, 0);
    for (int32_t g : grp) if (g >= 0) cnt[(size_t)g + 1]++;
    C.group_n.assign(cnt.begin() + 1, cnt.end());
    for (int64_t g = 0; g < n_groups; g++) cnt[(size_t)g + 1] += cnt[(size_t)g];
    const int64_t n_items = cnt[(size_t)n_groups];
    std::vector<int32_t> items((size_t)n_items), pbeg, wbeg, gbeg;
    {
        std::vector<int64_t> at(cnt.begin(), cnt.end() - 1);
        for (size_t f = 0; f < grp.size(); f++) if (grp[f] >= 0) items[(size_t)at[(size_t)grp[f]]++] = (int32_t)f;
    }
    const int64_t mw = max_waves(h->cfg.dim), len = std::max<int64_t>(1, (n_items + mw - 1) / mw);
    C.part_group.clear();
    for (int64_t g = 0; g < n_groups; g++) {
        gbeg.push_back((int32_t)pbeg.size());
        for (int64_t a = cnt[(size_t)g]; a < cnt[(size_t)g + 1]; a += len) { pbeg.push_back((int32_t)a); C.part_group.push_back((int32_t)g); }
    }
    gbeg.push_back((int32_t)pbeg.size());
    const int64_t np = (int64_t)pbeg.size(), nw = std::min<int64_t>(np, mw);
    pbeg.push_back((int32_t)n_items);
    for (int64_t w = 0; w <= nw; w++) wbeg.push_back((int32_t)(nw ? w * np / nw : 0));
    int32_t rc;
    if ((rc = dev_upload(h, &C.d_items, items)) != CX_OK || (rc = dev_upload(h, &C.d_pbeg, pbeg)) != CX_OK || (rc = dev_upload(h, &C.d_wbeg, wbeg)) != CX_OK ||
        (rc = dev_upload(h, &C.d_gbeg, gbeg)) != CX_OK)
        return rc;
    if ((rc = C.d_meta.ensure(h, 2 * np)) != CX_OK || (rc = C.d_acc.ensure(h, np * na)) != CX_OK || (rc = C.d_rows.ensure(h, n_groups * na)) != CX_OK) return rc;
    CX_HIP(h, hipStreamSynchronize(h->stream));      // (the host vectors die here)
    C.h_meta.assign((size_t)(2 * np), 0);
    C.h_rows.assign((size_t)(n_groups * na), 0.0);
    C.n_items = n_items; C.n_part = np; C.n_wave = nw;
    return CX_OK;
}

template <bool STATS>
static void launch(cx_handle *h, Cache &C, int nwave, const int32_t *wbeg, const int32_t *pbeg, const int32_t *items, double *out) {
    const int u = mfr::user_dim(h);
    mfr::for_tiles(h->cfg.dim, [&](auto nt) {
        constexpr int NT = decltype(nt)::value, W = NT == 4 ? 1 : 2;      // (4 x 4 tiles at two waves per SIMD: 7 to 11 registers spilled, so one)
        if (h->has_offsets)      // cx_set_factor_offsets_mfma: the instances that read g and b
            hipLaunchKernelGGL((k_lm_factors_off<NT, STATS, W>), dim3((unsigned)nwave), dim3(64), 0, h->stream, nwave, wbeg, pbeg, items, C.d_rec, C.d_srcs, h->d_ptab,
                               h->d_ptab_bt, C.atab.d, h->d_mv_f2v, h->d_mv_v2f, (const double *)h->d_off_g, (const double *)h->d_off_b, u, C.d_ws, C.d_acc, C.d_meta, out);
        else
        hipLaunchKernelGGL((k_lm_factors<NT, STATS, W>), dim3((unsigned)nwave), dim3(64), 0, h->stream, nwave, wbeg, pbeg, items, C.d_rec, C.d_srcs, h->d_ptab,
                           h->d_ptab_bt, C.atab.d, h->d_mv_f2v, h->d_mv_v2f, u, C.d_ws, C.d_acc, C.d_meta, out);
    });
}

}  // namespace lm

template <> void Deleter<lm::Cache>::operator()(lm::Cache *C) const { delete C; }

}  // namespace cx

using namespace cxh;

extern "C" int32_t cx_factor_beliefs_mfma(cx_handle *h, int64_t n, const int64_t *factor_ids, double *out) {
    try {
        namespace lm = cx::lm;
        const std::string who = "cx_factor_beliefs_mfma";
        lm::Cache *Cp = nullptr;
        int32_t rc;
        const char *bad = n >= 0 && (n == 0 || (factor_ids && out)) ? nullptr : "null argument or negative count";
        if ((rc = lm::prepare(h, who, "cx_factor_beliefs", bad, Cp)) != CX_OK) return rc;
        if (n == 0) return CX_OK;
        lm::Cache &C = *Cp;
        std::vector<int32_t> items((size_t)n);
        for (int64_t i = 0; i < n; i++) {
            const int64_t f = find_factor(h, factor_ids[i]);
            if (f < 0) return fail(h, CX_ERR_NOT_FOUND, who + ": no factor " + std::to_string(factor_ids[i]));
            if (C.kind[(size_t)f] < 0) return fail(h, CX_ERR_UNSUPPORTED, who + ": " + lm::no_pair(factor_ids[i]));
            items[(size_t)i] = (int32_t)f;
        }
        const int d = h->cfg.dim, u = cx::mfr::user_dim(h);
        const int64_t nb = 2 * u + 4 * (int64_t)u * u, chunk = std::min<int64_t>(n, lm::max_waves(d));
        if ((rc = C.d_bitems.ensure(h, chunk)) != CX_OK || (rc = C.d_bout.ensure(h, chunk * nb)) != CX_OK || (rc = C.d_ws.ensure(h, chunk * lm::ws_doubles(d))) != CX_OK) return rc;
        for (int64_t at = 0; at < n; at += chunk) {
            const int64_t m = std::min(chunk, n - at);
            CX_HIP(h, hipMemcpyAsync(C.d_bitems, items.data() + at, (size_t)m * 4, hipMemcpyHostToDevice, h->stream));
            lm::launch<false>(h, C, (int)m, nullptr, nullptr, C.d_bitems, C.d_bout);
            CX_HIP(h, hipGetLastError());
            CX_HIP(h, hipMemcpyAsync(out + at * nb, C.d_bout, (size_t)(m * nb) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            CX_HIP(h, hipStreamSynchronize(h->stream));
        }
        return CX_OK;
    } catch (const std::bad_alloc &) { return fail(h, CX_ERR_OUT_OF_MEMORY, "cx_factor_beliefs_mfma: host allocation failed"); }
}

extern "C" int32_t cx_factor_statistics_mfma(cx_handle *h, int64_t n, const int64_t *factor_ids, const int64_t *groups, int64_t n_groups, double *out,
                                             int64_t *counts4) {
    try {
        namespace lm = cx::lm;
        const std::string who = "cx_factor_statistics_mfma";
        lm::Cache *Cp = nullptr;
        int32_t rc;
        const char *bad = !(out && counts4 && n_groups > 0) ? "null output or n_groups < 1"
                          : !(factor_ids ? (n >= 0 && (n == 0 || groups)) : !groups)
                              ? "factor_ids and groups go together (n >= 0), or both null for the parameter-set grouping"
                              : nullptr;
        if ((rc = lm::prepare(h, who, "cx_factor_statistics", bad, Cp)) != CX_OK) return rc;
        lm::Cache &C = *Cp;
        const int d = h->cfg.dim, u = cx::mfr::user_dim(h), na = 2 * u + 3 * u * u, ns = 1 + na;
        if (!C.group_key.matches(n_groups, n, factor_ids, groups)) {
            C.group_key.valid = false;
            std::vector<int32_t> grp;
            if ((rc = lm::assign_groups(h, C, who, n, factor_ids, groups, n_groups, grp)) != CX_OK) return rc;
            if ((rc = lm::build_lists(h, C, grp, n_groups, na)) != CX_OK) return rc;
            C.group_key.remember(n_groups, n, factor_ids, groups);
        }
        std::fill(out, out + n_groups * ns, 0.0);
        for (int k = 0; k < 4; k++) counts4[k] = 0;
        if (C.n_part == 0) return CX_OK;
        if ((rc = C.d_ws.ensure(h, C.n_wave * lm::ws_doubles(d))) != CX_OK) return rc;
        lm::launch<true>(h, C, (int)C.n_wave, C.d_wbeg, C.d_pbeg, C.d_items, nullptr);
        hipLaunchKernelGGL(lm::k_lm_reduce, dim3((unsigned)n_groups, (unsigned)((na + 255) / 256)), dim3(256), 0, h->stream, na, C.d_gbeg, C.d_acc, C.d_rows);
        CX_HIP(h, hipGetLastError());
        CX_HIP(h, hipMemcpyAsync(C.h_rows.data(), C.d_rows, (size_t)(n_groups * na) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        CX_HIP(h, hipMemcpyAsync(C.h_meta.data(), C.d_meta, (size_t)(2 * C.n_part) * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        CX_HIP(h, hipStreamSynchronize(h->stream));
        std::vector<int64_t> g_bad((size_t)n_groups, 0);
        for (int64_t p = 0; p < C.n_part; p++) {
            counts4[2] += C.h_meta[(size_t)(2 * p)];
            counts4[3] += C.h_meta[(size_t)(2 * p + 1)];
            g_bad[(size_t)C.part_group[(size_t)p]] += C.h_meta[(size_t)(2 * p)] + C.h_meta[(size_t)(2 * p + 1)];
        }
        for (int64_t g = 0; g < n_groups; g++) {
            if (C.group_n[(size_t)g] == 0) continue;
            counts4[0] += C.group_n[(size_t)g];
            counts4[1] += 1;
            double *o = out + g * ns;
            o[0] = (double)C.group_n[(size_t)g];
            for (int k = 0; k < na; k++) o[1 + k] = g_bad[(size_t)g] > 0 ? kNaN : C.h_rows[(size_t)(g * na + k)];
        }
        return CX_OK;
    } catch (const std::bad_alloc &) { return fail(h, CX_ERR_OUT_OF_MEMORY, "cx_factor_statistics_mfma: host allocation failed"); }
}
