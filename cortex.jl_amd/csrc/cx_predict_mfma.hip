// cx_predict_mfma.hip — cx_predictive_mfma and cx_predictive_rows_mfma: cx_predictive at the matrix-core dims (cx_create dim
// 5 .. 64, internal tiles of 16 / 32 / 64): for every observation y that a two-variable rule factor y = A x + N(0, Q) generates from a
// non-observed x, the predictive distribution of that datum given other data, its log score and its squared standardised residual, from
// the stored factor→variable messages.  DESIGN.md §4o derives it; nothing here is a difference of messages:
//
//   cavity       Λc = Σ kept Λ, ηc = Σ kept η over x's stored messages the mode keeps (LOO: all but the row's own; CAUSAL: also not those
//                from rule factors on which x is the IN end), summed directly as cx_log_evidence_mfma sums its leave-one-out messages
//   Λc = U'U,    z = U^-T ηc,   Z = U^-T A'   (k_evm_terms' block-column solve with A' in place of B')
//   S = Q + Z'Z, ŷ = Z'z        (its Gram and vector passes with + for -)
//   e = y - ŷ,   S = Us'Us,  w = Us^-T e,  maha = Σ_{k < u} w_k²,  log_density = -½ (u log 2π + log det S + maha)
//
// One wave per row in the form of k_evm_terms (cx_evidence_mfma.hip): upper tiles in registers, the 16 x 16 diagonal tiles through
// diag_factor, z parked in LDS across the matrix solve.  A row is UNDEFINED when a stored message into x (kept or not) or the datum holds
// NaN, and otherwise IMPROPER when nothing is kept (flat by structure: no factorisation), when a pivot below u of Λc or S is not positive
// and finite, or when a pivot of Λc is at or below kFlat times the same diagonal entry of the sum of ALL stored messages into x: a
// message whose information is flat reaches the sum as the rounding of C - Yt'Yt, a number of either sign that must not pass for a
// cavity (cx_predict.hip: kFlatPivot).
//
// Embedded dims (a user dim u below the tile size KD): every matrix is block-diagonal, real block and padding block.  The padding block
// of a SUM OF MESSAGES may be zero (no rule table is added here, unlike cx_log_evidence_mfma's factor terms), and Z'Z runs over every
// row of Z: the identity is added to the padding diagonal of Λc before it is factored, which leaves the real block as it is.
//
// k_prm_rows writes (log_density, status) per row at the row's index and, when asked, the row's u + u² + 2 doubles; mfr::k_status_part folds 256
// rows into an ev::Part and ev::final_sum adds the parts in index order: no atomics, two calls on one state are bit-identical, and the
// total does not depend on how the payload is cut into chunks.
#include "cx_evidence_mfma_core.h"
#include "cx_mfma_reader.h"

namespace cx {
namespace prm {

using namespace w64;
using evm::add_sources, evm::any_nan_record, evm::factor_solve, evm::flat_pivot, evm::gram_pass, evm::pad_identity, evm::park_z, evm::solve_block_cols, evm::store_symmetric;

using mfr::Pairs;
constexpr int kScored = mfr::kRowOk, kUndefined = mfr::kRowUndefined, kImproper = mfr::kRowImproper;

// row record (8 int32): {parameter set, the slot of the datum (the OUT end's), kept offset, kept count, excluded offset, excluded count, 0, 0};
// kept and excluded are runs of message slots in `srcs`.  ttab: [set][A' | Q] at the internal dim.  One wave per row, rows [row0, row0 + n);
// out: null, or n rows of u + u² + 2 doubles (row row0 first).
template <int NT, int WAVES_PER_SIMD>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES_PER_SIMD, WAVES_PER_SIMD)))
void k_prm_rows(int row0, int n, const int32_t *__restrict__ rec, const int32_t *__restrict__ srcs, const double *__restrict__ ttab,
                const double *__restrict__ f2v, const double *__restrict__ v2f, const int u, const double k_flat, double *__restrict__ rval,
                uint8_t *__restrict__ rflag, double *__restrict__ out) {
    constexpr int KD = 16 * NT, KM = KD + KD * KD, NU = NT * (NT + 1) / 2;
    __shared__ double S[16 * kLdT];
    __shared__ double Vs[NT][16 * kLdT];
    __shared__ double ZS[KD];
    if ((int)blockIdx.x >= n) return;
    const int w = row0 + (int)blockIdx.x;
    const int lane = threadIdx.x, g = lane >> 4, c = lane & 15, mo = g * KD + c;
    const int32_t *t = rec + 8 * (int64_t)w;
    const int set = t[0], yslot = t[1], k_off = t[2], k_n = t[3], x_off = t[4], x_n = t[5];
    const double *tab = ttab + (int64_t)set * 2 * KD * KD;
    const int no = u + u * u + 2;
    double *o = out ? out + (int64_t)blockIdx.x * no : nullptr;
    const double nan = __builtin_nan("");

    // every store of the payload's matrix part: the same lane writes the same address whether it carries a value or NaN
    auto put_s = [&](int a, int b, int r, double v) {
        const int row = 16 * a + g + 4 * r, col = 16 * b + c;
        if (row < u && col < u) o[u + row * u + col] = v;
    };
    auto unscored = [&](int status) {
        if (o) {
#pragma unroll
            for (int j = 0; j < NT; j++)
                if (g == 0 && 16 * j + c < u) o[16 * j + c] = nan;
#pragma unroll
            for (int a = 0; a < NT; a++)
#pragma unroll
                for (int b = 0; b < NT; b++)
#pragma unroll
                    for (int r = 0; r < 4; r++) put_s(a, b, r, nan);
            if (lane == 0) { o[u + u * u] = nan; o[u + u * u + 1] = nan; }
        }
        if (lane == 0) { rval[w] = 0.0; rflag[w] = (uint8_t)status; }
    };

    // ---- the cavity's sums, the belief's diagonal, what is undefined --------------------------------------------------------------
    d4 M[NU];
    double wcv[NT];
#pragma unroll
    for (int i = 0; i < NU; i++) M[i] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < NT; j++) wcv[j] = 0.0;
    add_sources<NT>(M, wcv, f2v, srcs + k_off, k_n, mo, c);
    bool undef = __builtin_isnan(bcast(M[0][0], 0)) || __builtin_isnan(bcast(wcv[0], 0));      // (whole messages are NaN together)
    bool ynan = false;
#pragma unroll
    for (int j = 0; j < NT; j++) ynan = ynan || (16 * j + c < u && __builtin_isnan(v2f[(int64_t)yslot * KM + 16 * j + c]));      // (the datum is read again where it is used)
    pad_identity<NT>(M, g, c, u);
    undef = any_nan_record<NT>(undef || __ballot(ynan) != 0, f2v, srcs + x_off, x_n);
    if (undef) { unscored(kUndefined); return; }
    if (k_n == 0) { unscored(kImproper); return; }      // nothing is kept: flat by structure

    // ---- Λc = U'U, z = U^-T ηc; the flat-pivot rule off the tile diagonals of V = U^-1 ------------------------------------------------
    double zrv[NT][4], ld1, q1;
    bool pd1;
    factor_solve<NT>(M, wcv, zrv, S, Vs, g, c, u, ld1, q1, pd1);
    // against the diagonal of the sum of ALL stored messages into x (kept and excluded are adjacent runs of srcs)
    if (!pd1 || __ballot(flat_pivot<NT>(Vs, f2v, srcs + k_off, k_n + x_n, c, u, k_flat)) != 0) { unscored(kImproper); return; }
    park_z<NT>(ZS, zrv, g);

    // ---- Z = U^-T A', one block column at a time ------------------------------------------------------------------------------------
    d4 Y[NT][NT];
    solve_block_cols<NT, false>(Y, M, Vs, [&](int k) { return ((gcdp)tab)[mo + k]; }, g, c);
    // ---- S = Q + Z'Z (upper tiles), ŷ = Z'z, e = y - ŷ ----------------------------------------------------------------------------
    d4 Sm[NU];
    double ecv[NT];
    gram_pass<NT, 1>(Sm, Y, ZS, [&](int k) { return ((gcdp)tab)[KD * KD + mo + k]; }, [&](int a, double yh) {
        ecv[a] = v2f[(int64_t)yslot * KM + 16 * a + c] - yh;
        if (o && g == 0 && 16 * a + c < u) o[16 * a + c] = yh;
    }, g);
    // the payload's S before the factorisation takes the tiles
    if (o) {
#pragma unroll
        for (int a = 0; a < NT; a++)
#pragma unroll
            for (int b = a; b < NT; b++) store_symmetric(Sm[utn<NT>(a, b)], a, b, S, put_s, g, c);
    }
    // ---- the score -------------------------------------------------------------------------------------------------------------------
    // The lane's coordinates anew: with the two factorisations in one straight line hipcc keeps what the first derives from (g, c) — the
    // sixteen (k == c) selects of diag_factor among them, 32 registers — for the second, across the matrix solve, and spills at NT = 4
    int g2 = g, c2 = c;
    asm volatile("" : "+v"(g2), "+v"(c2));
    double wrv[NT][4], ld2, maha;
    bool pd2;
    factor_solve<NT>(Sm, ecv, wrv, S, Vs, g2, c2, u, ld2, maha, pd2);
    if (!pd2) { unscored(kImproper); return; }
    if (lane != 0) return;
    const double val = -0.5 * (u * ev::kLog2Pi + ld2 + maha);
    if (o) { o[u + u * u] = val; o[u + u * u + 1] = maha; }
    rval[w] = val;
    rflag[w] = (uint8_t)kScored;
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
// The rows follow the mode, the caller's ids, the graph and WHICH variables are observed (vinfo_epoch: cx_derived.h), the [A' | Q] table
// the rule parameters (param_epoch); messages and data are read by every call
struct Plan {
    mfr::RequestKey key;      // tag: the mode
    uint64_t vinfo_epoch = 0;
    int64_t n_rows = 0;
    DevBuf<int32_t> d_rec, d_srcs;
    mfr::ParamTable tab;
    DevBuf<double> d_rval, d_rows;
    DevBuf<uint8_t> d_rflag;
    DevBuf<ev::Part> d_part;
    mfr::Totals totals;
};

// a row: the OUT end observed, the IN end not
static bool is_row(const cx_handle *h, const Pairs &P, int64_t f) {
    return P.so[f] >= 0 && (h->vinfo[P.vo[f]] & kClamped) != 0 && (h->vinfo[P.vi[f]] & kClamped) == 0;
}

static const mfr::Words kWords = {"cx_predictive", "the variational and Beta-Bernoulli families have no Gaussian predictive", "rows"};
static const char *kNotARow = " is not a row: a two-variable CX_FACTOR_GAUSS_LINEAR factor whose CX_ROLE_OUT end is observed and whose CX_ROLE_IN end is not";

// the factor indices of the rows, checked: the caller's, in the caller's order, or every row in ascending factor id
static int32_t list_rows(cx_handle *h, const Pairs &P, const std::string &who, int64_t n, const int64_t *ids, std::vector<int64_t> &fac) {
    using namespace cxh;
    fac.clear();
    if (!ids) {
        for (int64_t f = 0; f < h->nf; f++) if (is_row(h, P, f)) fac.push_back(f);
        return CX_OK;
    }
    for (int64_t i = 0; i < n; i++) {
        const int64_t f = find_factor(h, ids[i]);
        if (f < 0) return fail(h, CX_ERR_NOT_FOUND, who + ": no factor " + std::to_string(ids[i]));
        if (!is_row(h, P, f)) return fail(h, CX_ERR_UNSUPPORTED, who + ": factor " + std::to_string(ids[i]) + kNotARow);
        fac.push_back(f);
    }
    return CX_OK;
}

static int32_t build_plan(cx_handle *h, const Pairs &P, Plan &L, int32_t mode, const std::vector<int64_t> &fac, const std::string &who) {
    using namespace cxh;
    const int64_t n = (int64_t)fac.size();
    // CX_PREDICT_CAUSAL: the slots on which a variable is the IN end of a rule factor (cx_predict.hip: build_plan)
    std::vector<uint8_t> in_slot((size_t)h->nslots, 0);
    if (mode == CX_PREDICT_CAUSAL)
        for (int64_t f = 0; f < h->nf; f++) if (P.si[f] >= 0) in_slot[(size_t)P.si[f]] = 1;
    std::vector<int32_t> rec((size_t)n * 8, 0), srcs;
    for (int64_t i = 0; i < n; i++) {
        const int64_t f = fac[(size_t)i];
        const int32_t x = P.vi[f], own = P.si[f];
        int32_t *r = &rec[(size_t)i * 8];
        r[0] = P.set[f]; r[1] = P.so[f];
        // x's slots: the kept run, then the excluded one
        const auto kept = [&](int32_t s) { return s != own && !in_slot[(size_t)s]; };
        const mfr::Run k = mfr::slots_where(h, x, srcs, kept), ex = mfr::slots_where(h, x, srcs, [&](int32_t s) { return !kept(s); });
        r[2] = k.off; r[3] = k.n; r[4] = ex.off; r[5] = ex.n;
        CX_REQUIRE(h, (int64_t)srcs.size() < (int64_t)0x7fffff00, CX_ERR_UNSUPPORTED, who + ": more than 2^31 inputs");
    }
    CX_REQUIRE(h, n < (int64_t)0x7fffff00, CX_ERR_UNSUPPORTED, who + ": more than 2^31 rows");
    L.n_rows = n;
    const int64_t nb = (n + mfr::kTB - 1) / mfr::kTB;
    if (srcs.empty()) srcs.push_back(0);      // (never read: no row names a slot)
    int32_t rc;
    if ((rc = dev_upload(h, &L.d_rec, rec)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &L.d_srcs, srcs)) != CX_OK) return rc;
    if ((rc = dev_alloc(h, &L.d_rval, std::max<int64_t>(n, 1))) != CX_OK) return rc;
    if ((rc = dev_alloc(h, &L.d_rflag, std::max<int64_t>(n, 1))) != CX_OK) return rc;
    if ((rc = dev_alloc(h, &L.d_part, std::max<int64_t>(nb, 1))) != CX_OK) return rc;
    CX_HIP(h, hipStreamSynchronize(h->stream));      // (the local host vectors die here)
    return CX_OK;
}

// [set][A' | Q] at the internal dim (blockdiag(A, I)', blockdiag(Q, I) for an embedded one: cx_set_factor_matrices)
static void fill_tab(const cx_handle *h, std::vector<double> &tb) {
    const size_t d = (size_t)h->cfg.dim, dd = d * d, ns = std::max<size_t>(h->psets.size(), 1);
    tb.assign(ns * 2 * dd, cxh::kNaN);
    for (size_t s = 0; s < h->psets.size(); s++) {
        if (h->psets[s].empty()) continue;
        const double *A = h->psets[s].data(), *Q = A + dd;
        for (size_t r = 0; r < d; r++)
            for (size_t c = 0; c < d; c++) {
                tb[s * 2 * dd + c * d + r] = A[r * d + c];
                tb[s * 2 * dd + dd + r * d + c] = 0.5 * (Q[r * d + c] + Q[c * d + r]);
            }
    }
}

// rows [row0, row0 + n) (d_rows: their payload, or null)
static void launch_rows(cx_handle *h, Plan &L, int64_t row0, int64_t n, double *d_rows) {
    if (!n) return;
    const int u = mfr::user_dim(h);
    const double k_flat = mfr::flat_pivot_factor(h);
    mfr::for_tiles(h->cfg.dim, [&](auto nt) {
        // waves per SIMD as the register counts allow; the launch bound makes hipcc keep to them without scratch
        constexpr int NT = decltype(nt)::value, W = NT == 1 ? 4 : NT == 2 ? 3 : 2;
        hipLaunchKernelGGL((k_prm_rows<NT, W>), dim3((unsigned)n), dim3(64), 0, h->stream, (int)row0, (int)n, L.d_rec, L.d_srcs, L.tab.d, h->d_mv_f2v,
                           h->d_mv_v2f, u, k_flat, L.d_rval, L.d_rflag, d_rows);
    });
}

}  // namespace prm

template <> void Deleter<prm::Plan>::operator()(prm::Plan *P) const { delete P; }

}  // namespace cx

using namespace cxh;

extern "C" int32_t cx_predictive_rows_mfma(cx_handle *h, int64_t cap, int64_t *factor_ids, int64_t *n_rows) {
    try {
        namespace prm = cx::prm;
        const std::string who = "cx_predictive_rows_mfma";
        cx::mfr::Pairs P;
        int32_t rc;
        const char *bad = n_rows && cap >= 0 && (cap == 0 || factor_ids) ? nullptr : "null argument or negative capacity";
        if ((rc = cx::mfr::prepare(h, who, bad, prm::kWords)) != CX_OK) return rc;
        if ((rc = cx::mfr::checked_pairs(h, who, P)) != CX_OK) return rc;
        std::vector<int64_t> fac;
        if ((rc = prm::list_rows(h, P, who, 0, nullptr, fac)) != CX_OK) return rc;
        *n_rows = (int64_t)fac.size();
        for (int64_t i = 0; i < std::min<int64_t>(cap, *n_rows); i++) factor_ids[i] = h->fac_ids[(size_t)fac[(size_t)i]];
        return CX_OK;
    } catch (const std::bad_alloc &) { return fail(h, CX_ERR_OUT_OF_MEMORY, "cx_predictive_rows_mfma: host allocation failed"); }
}

extern "C" int32_t cx_predictive_mfma(cx_handle *h, int32_t mode, int64_t n, const int64_t *factor_ids, double *out, double *total, int64_t *counts4) {
    try {
        namespace prm = cx::prm;
        namespace mfr = cx::mfr;
        const std::string who = "cx_predictive_mfma";
        int32_t rc;
        const char *bad = !counts4 ? "counts4 is null"
                          : mode != CX_PREDICT_LOO && mode != CX_PREDICT_CAUSAL ? "mode is CX_PREDICT_LOO or CX_PREDICT_CAUSAL"
                          : factor_ids && n < 0 ? "negative count" : nullptr;
        if ((rc = mfr::prepare(h, who, bad, prm::kWords)) != CX_OK) return rc;
        if (h->predict_mfma && h->predict_mfma->vinfo_epoch != h->vinfo_epoch) h->predict_mfma.reset();      // other variables are observed
        if (!h->predict_mfma) h->predict_mfma.reset(new prm::Plan());
        prm::Plan &L = *h->predict_mfma;
        if (!L.key.matches(mode, n, factor_ids)) {
            L.key.valid = false;
            mfr::Pairs P;
            if ((rc = mfr::checked_pairs(h, who, P)) != CX_OK) return rc;
            std::vector<int64_t> fac;
            if ((rc = prm::list_rows(h, P, who, n, factor_ids, fac)) != CX_OK) return rc;
            if ((rc = prm::build_plan(h, P, L, mode, fac, who)) != CX_OK) return rc;
            L.key.remember(mode, n, factor_ids);
            L.vinfo_epoch = h->vinfo_epoch;
        }
        if ((rc = L.tab.refresh(h, [&](std::vector<double> &t) { prm::fill_tab(h, t); })) != CX_OK) return rc;
        if ((rc = mv_ensure_chain_msgs(h)) != CX_OK) return rc;      // (every reader of d_mv_f2v calls this first)
        const int u = mfr::user_dim(h);
        const int64_t nr = L.n_rows;
        // the payload a chunk at a time through a bounded device buffer; the (value, status) arrays cover every row
        if (out) rc = mfr::stream_rows(h, nr, (int64_t)u + (int64_t)u * u + 2, L.d_rows, out, [&](int64_t r0, int64_t m, double *d) { prm::launch_rows(h, L, r0, m, d); });
        else prm::launch_rows(h, L, 0, nr, nullptr);
        if (rc != CX_OK) return rc;
        double sum;
        if ((rc = L.totals.read_rows(h, nr, L.d_rval, L.d_rflag, L.d_part, counts4, &sum)) != CX_OK) return rc;
        if (total) *total = sum;
        return CX_OK;
    } catch (const std::bad_alloc &) { return fail(h, CX_ERR_OUT_OF_MEMORY, "cx_predictive_mfma: host allocation failed"); }
}
