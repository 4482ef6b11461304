// cx_evidence_mfma.hip — cx_log_evidence_mfma: log p(data) of a Gaussian model at the matrix-core dims (cx_create dim 5 .. 64, internal
// tiles of 16 / 32 / 64) from the stored factor→variable messages and the caller's data.  DESIGN.md §4e defines the quantity,
//
//   log Z = Σ_o c_o + Σ_a log z_a + Σ_i (1 - d_i) log z_i,
//
// and §4m derives the terms at these dims.  Only pairwise x_out = A x_in + N(0, Q) factors and opaque messages exist here, so every
// term is one or two factorisations of a KD x KD matrix "table + sum of message records" by ONE WAVE, in the form of k_rule64w
// (cx_mv64w.hip): upper tiles in registers, the 16 x 16 diagonal tiles through diag_factor, U^-T η on the vector pipe.  With
// m_{i→a} the sum of variable i's OTHER stored messages (summed directly, as k_v2f64 does — never M_i - m_{a→i}):
//
//   variable (d_i != 1)       Λ = Σ all messages:                       log z_i = ½ η'Λ⁻¹η - ½ log det Λ + (d/2) log 2π
//   opaque message            Λ_o positive definite:                    c_o = ½ log det Λ_o - ½ η_o'Λ_o⁻¹η_o - (d/2) log 2π   (else 0)
//   factor, one end observed  S = Λ_{free→a} + C, h = η_{free→a} + B y: log z_a = -½ log det 2πQ - ½ y'P y + ½ h'S⁻¹h - ½ log det S + (d/2) log 2π
//                             ((P, B, C) the rule table TOWARDS the free end: its (C, B y) is the message k_point64 writes)
//   factor, both ends free    the OUT end goes first: M = Λ_{out→a} + Q⁻¹ is positive definite whenever its input is defined, a flat
//                             leaf included; that elimination IS the rule towards IN applied to m_{out→a}, (Λ', η') = (C - B M⁻¹ B',
//                             B M⁻¹ η_out), kept in registers; then S = Λ_{in→a} + Λ', h = η_{in→a} + η':
//                             log z_a = -½ log det 2πQ + [½ η_out'M⁻¹η_out - ½ log det M] + [½ h'S⁻¹h - ½ log det S] + d log 2π
//   factor, both observed     log N(y_out; A y_in, Q)
//
// Embedded dims (a user dim of 5 .. 15, 17 .. 31, 33 .. 63: every matrix block-diagonal, real block and identity block): a
// block-diagonal matrix has a block-diagonal Cholesky factor, so every log-determinant is Σ_{k < user dim} 2 log U_kk, every quadratic
// form the first `user dim` entries of U^-T η, and d above is the user's: the value is the real model's at any internal tile size.
//
// The terms are evaluated UNCENTRED (§4e centres dims 1 .. 4 on the belief means): ½ η'Λ⁻¹η of a term is of size (y/σ)² per component
// and cancels between terms, so about (y/σ)² 1e-16 of absolute error per term against ~ d/2 of value: 1e-9 relative is lost for data
// beyond ~ 3e3 √d standard deviations from the origin (an estimate from the sizes of the terms, not a measurement).
//
// k_evm_terms writes one (value, flags) per term at the term's index; k_evm_part folds 256 terms into an ev::Part and ev::final_sum
// (k_ev_final, cx_evidence.hip) adds the parts in index order: no atomics, two calls on one state are bit-identical.
// cx_log_evidence and cx_log_evidence_components keep refusing these dims (their tests pin that); routing them here is a later,
// separate decision.
//
// cx_log_evidence_components_mfma: the same k_evm_terms launch, then the terms summed per connected component of the
// graph by the segmented sum of cx_log_evidence_components (ev::reduce_components: k_ev_seg / k_ev_span of cx_evidence.hip, §4l) over
// d_tval / d_tflag in place of k_evm_part and k_ev_final.  The term list keeps its order; the plan (evm::build_components) only
// says which component every term belongs to.
#include "cx_components.h"
#include "cx_evidence_mfma_terms.h"

namespace cx {
namespace evm {

using namespace w64;

// one wave per term (evm_term, cx_evidence_mfma_terms.h: the records, the kinds and the arithmetic).  This is the entry point of a handle
// without factor offsets; k_evm_terms_off (cx_evidence_mfma_off.hip) is the one of a handle with them
template <int NT, int WAVES_PER_SIMD>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES_PER_SIMD, WAVES_PER_SIMD)))
void k_evm_terms(int nterm, const int32_t *__restrict__ rec, const int32_t *__restrict__ srcs, const double *__restrict__ ptab,
                 const double *__restrict__ btab, const double *__restrict__ ldq, const double *__restrict__ f2v,
                 const double *__restrict__ v2f, const int u, double *__restrict__ tval, uint8_t *__restrict__ tflag) {
    __shared__ double S[16 * kLdT];
    __shared__ double Vs[NT][16 * kLdT];
    __shared__ double ZS[16 * NT];
    evm_term<NT, false>(nterm, rec, srcs, ptab, btab, ldq, f2v, v2f, nullptr, nullptr, u, tval, tflag, S, Vs, ZS);
}

// 256 terms -> one ev::Part (fixed-order tree); ev::final_sum adds the parts in index order
__global__ __launch_bounds__(kTB) void k_evm_part(int nterm, const double *__restrict__ tval, const uint8_t *__restrict__ tflag, ev::Part *__restrict__ part) {
    const int i = blockIdx.x * kTB + threadIdx.x;
    const double s = i < nterm ? tval[i] : 0.0;
    const unsigned f = i < nterm ? tflag[i] : 0u;
    ev::block_part<kTB>(s, 0.0, (f & ev::kTermVar) ? 1u : 0u, (f & ev::kTermUndef) ? 1u : 0u, (f & ev::kTermNpd) ? 1u : 0u, 0u, part);
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
// The term lists follow the graph and WHICH variables are observed (vinfo_epoch: cx_derived.h), the log-det table the rule parameters
// (param_epoch); messages and data are read by every call
struct Cache {
    bool built = false;
    uint64_t vinfo_epoch = 0;
    int64_t n_term = 0, n_fac = 0, nb = 0, unsupported_fac = -1;
    DevBuf<int32_t> d_rec, d_srcs;
    mfr::ParamTable ldq;
    DevBuf<double> d_tval;
    DevBuf<uint8_t> d_tflag;
    DevBuf<ev::Part> d_part;
    mfr::Totals totals;
    // cx_log_evidence_components_mfma: the plan of the first component call, dropped with the cache.  term_var / term_fac: the variable
    // every term of d_rec is filed under and whether it is a factor's (kept from build() until the plan is made)
    bool comp_built = false;
    std::vector<int32_t> term_var;
    std::vector<uint8_t> term_fac;
    std::vector<int64_t> comp_fac_terms;      // [C] the factor terms of every component
    ev::CompPlan comp;
};

static int32_t build(cx_handle *h, Cache &C, const std::string &who) {
    using namespace cxh;
    using mfr::Run;
    mfr::Pairs P;
    mfr::pairs_of(h, P);
    // the terms in the order made, and the variable each is filed under: the list is sorted by it (stable), so that a variable's term,
    // the terms of its factors and those of its neighbours — which read the same message records — are next to each other
    std::vector<int32_t> made, key, srcs;
    auto term = [&](int32_t file_under, int kind, int tab, Run a, Run b, int y0, int y1) {
        const int32_t r[8] = {kind, tab, a.off, a.n, b.off, b.n, y0, y1};
        made.insert(made.end(), r, r + 8);
        key.push_back(file_under);
    };
    C.unsupported_fac = P.unsupported_fac;
    for (int64_t v = 0; v < h->nv; v++) {
        if (h->vinfo[v] & (kClamped | kGhost)) continue;
        int di = 0;
        for (int32_t e = h->var_off[v]; e < h->var_off[v + 1]; e++) {
            if (h->fac_kind[P.efac[e]] != CX_FACTOR_OPAQUE) { di++; continue; }
            srcs.push_back(slot_of_edge(h, e));
            term((int32_t)v, kOpaque, -1, {}, {(int32_t)srcs.size() - 1, 1}, 0, 0);
        }
        if (di == 1) continue;
        term((int32_t)v, kVar, -1, {}, mfr::other_slots(h, (int32_t)v, -1, srcs), di, 0);
    }
    C.n_fac = 0;
    for (int64_t f = 0; f < h->nf; f++) {
        if (P.so[f] < 0) continue;
        const int32_t so = P.so[f], si = P.si[f], vo = P.vo[f], vi = P.vi[f], set = P.set[f];
        const bool oo = (h->vinfo[vo] & kClamped) != 0, oi = (h->vinfo[vi] & kClamped) != 0;
        if (oo && oi) term(std::min(vo, vi), kFacBoth, 2 * set + 1, {}, {}, so, si);
        else if (oo) term(vi, kFacObs, 2 * set + 1, {}, mfr::other_slots(h, vi, si, srcs), so, si);      // towards IN
        else if (oi) term(vo, kFacObs, 2 * set, {}, mfr::other_slots(h, vo, so, srcs), si, so);          // towards OUT
        else {
            const Run a = mfr::other_slots(h, vo, so, srcs);
            term(std::min(vo, vi), kFacFree, 2 * set + 1, a, mfr::other_slots(h, vi, si, srcs), so, si);
        }
        C.n_fac++;
    }
    C.n_term = (int64_t)key.size();
    std::vector<int32_t> order((size_t)C.n_term), rec;
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return key[(size_t)a] < key[(size_t)b]; });
    rec.reserve(made.size());
    C.term_var.clear(); C.term_fac.clear();
    for (int32_t i : order) {
        rec.insert(rec.end(), made.begin() + 8 * (size_t)i, made.begin() + 8 * (size_t)i + 8);
        C.term_var.push_back(key[(size_t)i]);
        C.term_fac.push_back(made[8 * (size_t)i] >= kFacFree);
    }
    CX_REQUIRE(h, C.n_term < (int64_t)0x7fffffff && (int64_t)srcs.size() < (int64_t)0x7fffffff, CX_ERR_UNSUPPORTED, who + ": more than 2^31 terms");
    C.nb = (C.n_term + kTB - 1) / kTB;
    int32_t rc;
    if ((rc = dev_upload(h, &C.d_rec, rec)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &C.d_srcs, srcs)) != CX_OK) return rc;
    if ((rc = dev_alloc(h, &C.d_tval, C.n_term)) != CX_OK) return rc;
    if ((rc = dev_alloc(h, &C.d_tflag, C.n_term)) != CX_OK) return rc;
    if ((rc = dev_alloc(h, &C.d_part, C.nb)) != CX_OK) return rc;
    CX_HIP(h, hipStreamSynchronize(h->stream));      // (the local host vectors die here)
    C.built = true;
    C.vinfo_epoch = h->vinfo_epoch;
    return CX_OK;
}

// log det 2πQ of the real block of every parameter set (Q symmetric positive definite: cx_set_factor_matrices checks it)
static void fill_ldq(const cx_handle *h, std::vector<double> &ldq) {
    const int d = h->cfg.dim, u = mfr::user_dim(h);
    ldq.assign(std::max<size_t>(h->psets.size(), 1), cxh::kNaN);
    std::vector<double> L((size_t)u * u);
    for (size_t s = 0; s < h->psets.size(); s++) {
        if (h->psets[s].empty()) continue;
        const double *Q = h->psets[s].data() + (size_t)d * d;
        double ld = u * ev::kLog2Pi;
        for (int j = 0; j < u; j++) {
            double t = Q[(size_t)j * d + j];
            for (int k = 0; k < j; k++) t -= L[(size_t)j * u + k] * L[(size_t)j * u + k];
            L[(size_t)j * u + j] = std::sqrt(t); ld += std::log(t);
            for (int i = j + 1; i < u; i++) {
                double x = 0.5 * (Q[(size_t)i * d + j] + Q[(size_t)j * d + i]);
                for (int k = 0; k < j; k++) x -= L[(size_t)i * u + k] * L[(size_t)j * u + k];
                L[(size_t)i * u + j] = x / L[(size_t)j * u + j];
            }
        }
        ldq[s] = ld;
    }
}

// The plan of cx_log_evidence_components_mfma: the labels of the graph as cx_graph_create received it (comp::label), every term under
// the label of the variable it is filed under — an opaque term's variable, one end of a factor: the same component as the factor —
// and ev::plan_components' positions.  The term list itself stays as build() left it
static int32_t build_components(cx_handle *h, Cache &C, const std::string &who) {
    using namespace cxh;
    std::vector<int32_t> efac((size_t)h->ne), var_label, fac_label, term_label((size_t)C.n_term);
    for (int64_t e = 0; e < h->ne; e++) efac[(size_t)e] = (int32_t)find_factor(h, h->edge_fac_id[(size_t)e]);
    const int64_t n_comp = comp::label(h->nv, h->nf, h->ne, h->edge_var.data(), efac.data(), var_label, fac_label);
    C.comp_fac_terms.assign((size_t)n_comp, 0);
    for (int64_t t = 0; t < C.n_term; t++) {
        term_label[(size_t)t] = var_label[(size_t)C.term_var[(size_t)t]];
        C.comp_fac_terms[(size_t)term_label[(size_t)t]] += C.term_fac[(size_t)t];
    }
    int32_t rc;
    if ((rc = ev::plan_components(h, C.comp, n_comp, term_label, who)) != CX_OK) return rc;
    std::vector<int32_t>().swap(C.term_var);
    std::vector<uint8_t>().swap(C.term_fac);
    C.comp_built = true;
    return CX_OK;
}

// the handle's cache with its term lists and its log-det table, the messages in their slots: what both entries do after mfr::prepare
static int32_t ready(cx_handle *h, const std::string &who, Cache *&Cp) {
    using namespace cxh;
    int32_t rc;
    if (h->evidence_mfma && h->evidence_mfma->vinfo_epoch != h->vinfo_epoch) h->evidence_mfma.reset();      // other variables are observed
    if (!h->evidence_mfma) h->evidence_mfma.reset(new Cache());
    Cache &C = *h->evidence_mfma;
    if (!C.built && (rc = build(h, C, who)) != CX_OK) { h->evidence_mfma.reset(); return rc; }
    if (C.unsupported_fac >= 0) return mfr::refuse_factor(h, who, C.unsupported_fac);
    if ((rc = C.ldq.refresh(h, [&](std::vector<double> &t) { fill_ldq(h, t); })) != CX_OK) return rc;
    if ((rc = mv_ensure_chain_msgs(h)) != CX_OK) return rc;      // (every reader of d_mv_f2v calls this first)
    Cp = &C;
    return CX_OK;
}

// k_evm_terms: one (value, flags) per term into d_tval / d_tflag
static void launch_terms(cx_handle *h, Cache &C) {
    const int n = (int)C.n_term, u = mfr::user_dim(h);
    if (!n) return;
    if (h->has_offsets) { launch_terms_off(h, n, C.d_rec, C.d_srcs, C.ldq.d, C.d_tval, C.d_tflag); return; }      // cx_set_factor_offsets_mfma: the instances that read g and κ
    const unsigned grid = 8u * (unsigned)((n + 7) / 8);      // (k_evm_terms: an eighth of the terms per XCD)
    mfr::for_tiles(h->cfg.dim, [&](auto nt) {
        // waves per SIMD as the register counts allow; the launch bound makes hipcc keep to them without scratch.
        // 4 x 4 tiles: 256 registers, and only with one block of B' / one tile of C in flight in the two-free-ends pass
        constexpr int NT = decltype(nt)::value, W = NT == 1 ? 4 : NT == 2 ? 3 : 2;
        hipLaunchKernelGGL((k_evm_terms<NT, W>), dim3(grid), dim3(64), 0, h->stream, n, C.d_rec, C.d_srcs, h->d_ptab, h->d_ptab_bt, C.ldq.d, h->d_mv_f2v,
                           h->d_mv_v2f, u, C.d_tval, C.d_tflag);
    });
}

static void launch(cx_handle *h, Cache &C) {
    launch_terms(h, C);
    if (C.n_term) hipLaunchKernelGGL(k_evm_part, dim3((unsigned)C.nb), dim3(kTB), 0, h->stream, (int)C.n_term, C.d_tval, C.d_tflag, C.d_part);
}

}  // namespace evm

template <> void Deleter<evm::Cache>::operator()(evm::Cache *C) const { delete C; }

}  // namespace cx

using namespace cxh;

extern "C" int32_t cx_log_evidence_mfma(cx_handle *h, double *value, int64_t *counts4) {
    try {
        namespace evm = cx::evm;
        namespace mfr = cx::mfr;
        const std::string who = "cx_log_evidence_mfma";
        int32_t rc;
        if ((rc = mfr::prepare(h, who, value && counts4 ? nullptr : "null argument", {"cx_log_evidence", "no variational free energy, no Beta-Bernoulli evidence", "terms", true})) != CX_OK)
            return rc;
        evm::Cache *Cp = nullptr;
        if ((rc = evm::ready(h, who, Cp)) != CX_OK) return rc;
        evm::Cache &C = *Cp;
        evm::launch(h, C);
        if ((rc = C.totals.read(h, C.nb, C.d_part, C.n_fac, counts4, value)) != CX_OK) return rc;
        if (counts4[2] + counts4[3] > 0) *value = kNaN;
        return CX_OK;
    } catch (const std::bad_alloc &) { return fail(h, CX_ERR_OUT_OF_MEMORY, "cx_log_evidence_mfma: host allocation failed"); }
}

extern "C" int32_t cx_log_evidence_components_mfma(cx_handle *h, int64_t cap, double *values, int64_t *comp_counts4, int64_t *n_components, int64_t *counts4) {
    try {
        namespace evm = cx::evm;
        namespace mfr = cx::mfr;
        const std::string who = "cx_log_evidence_components_mfma";
        const char *bad = !n_components || !counts4 ? "null n_components or counts4" : cap < 0 ? "cap < 0" : cap > 0 && !values ? "cap > 0 with null values" : nullptr;
        int32_t rc;
        if ((rc = mfr::prepare(h, who, bad, {"cx_log_evidence_components", "no variational free energy, no Beta-Bernoulli evidence", "terms", true})) != CX_OK) return rc;
        evm::Cache *Cp = nullptr;
        if ((rc = evm::ready(h, who, Cp)) != CX_OK) return rc;
        evm::Cache &C = *Cp;
        if (!C.comp_built && (rc = evm::build_components(h, C, who)) != CX_OK) return rc;
        evm::launch_terms(h, C);
        cx::ev::reduce_components(h, C.comp, C.d_tval, C.d_tflag);
        return cx::ev::read_components(h, C.comp, who, C.n_fac, C.comp_fac_terms, cap, values, comp_counts4, n_components, counts4);
    } catch (const std::bad_alloc &) { return fail(h, CX_ERR_OUT_OF_MEMORY, "cx_log_evidence_components_mfma: host allocation failed"); }
}
