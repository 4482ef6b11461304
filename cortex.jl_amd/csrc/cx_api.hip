// cx_api.hip — host side of libcortex_hip.so: the C ABI of include/cortex_hip.h.
//
// Flattens the bipartite factor graph once (reference: the accessor loops of
// src/inference_engine.jl:228-247 and src/dependencies.jl:5-126 over
// ext/BipartiteFactorGraphsExt/BipartiteFactorGraphsExt.jl:22-48) into a CSR edge table sorted by
// (variable id, factor id), keeps Gaussian messages resident in HBM, and launches the kernels of
// cx_kernels.hip.  No exception leaves this file; every entry point returns a status.


#include "cx_host.h"
#include "cx_flatten.h"

using namespace cxh;

namespace cxh {

void dev_free_all(cx_handle *h) {
    // the raw exceptions (cx_internal.h), freed where they always were
    cx::chain64_free(h);
    cx::chain_onepass_free(h);
    for (void *p : {(void *)h->d_marg64_sums, (void *)h->d_marg64_tab, (void *)h->d_marg64_rec}) if (p) (void)hipFree(p);
    h->d_marg64_sums = h->d_marg64_tab = nullptr; h->d_marg64_rec = nullptr; h->marg64_cap = 0;
    cx::chain64_tree_free(h);
    // every graph, buffer, cache, flag and counter of the graph on the device, in DevState's order
    static_cast<cx::DevState &>(*h) = cx::DevState();
    h->device_bytes = 0; h->d_ref_list = nullptr; h->batch_epoch++;
}

}  // namespace cxh

extern "C" {

int32_t cx_version(void) { return CX_ABI_VERSION; }

const char *cx_last_error(const cx_handle *h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int64_t cx_payload_doubles(int32_t dim, int32_t form) {
    if (dim < 1) return -1;
    if (form == CX_FORM_POINT) return dim;
    if (form == CX_FORM_MOMENT || form == CX_FORM_NATURAL) return (int64_t)dim + (int64_t)dim * dim;
    if ((form == CX_FORM_MEAN_PRECISION || form == CX_FORM_GAMMA) && dim == 1) return 2;
    return -1;
}

const char *cx_kernel_name(int32_t k) {
    switch (k) {
    case CX_KERNEL_VAR_TO_FACTOR: return "k_sweep<var_to_factor>";
    case CX_KERNEL_FACTOR_TO_VAR: return "k_factor_to_var";
    case CX_KERNEL_FUSED: return "k_sweep<fused>";
    case CX_KERNEL_BATCH: return "k_batch";
    case CX_KERNEL_BIG_VAR: return "k_big_var_to_factor";
    case CX_KERNEL_HALO_BEGIN: return "k_halo_export";
    case CX_KERNEL_HALO_END: return "k_halo_import";
    }
    return "";
}

int32_t cx_create(const cx_config *config, cx_handle **out) {
    if (!out) return fail(nullptr, CX_ERR_INVALID_ARGUMENT, "cx_create: out is NULL");
    *out = nullptr;
    if (!config || config->struct_size != (int32_t)sizeof(cx_config))
        return fail(nullptr, CX_ERR_INVALID_ARGUMENT, "cx_create: config is NULL or struct_size mismatch");
    if (config->dim < 1 || config->dim > 64)
        return fail(nullptr, CX_ERR_UNSUPPORTED, "cx_create: this build implements dim 1 .. 64");
    // dim 5 .. 64 run on the matrix-core path in 1 x 1, 2 x 2 or 4 x 4 tiles of 16 (cx_const.h: is_mfma_dim): internal dim 16, 32 or 64,
    // the smallest that holds the user's (round 6; until then always 64: a d = 8 message moved 64 x its bytes).  A dim in between is
    // embedded: x -> (x, u) with u a unit random walk observed nowhere — every rule matrix, message and datum block-diagonal (real block,
    // identity block), so the real block of every result is exact and the identity block keeps every joint positive definite.  The
    // chain-scan and tree schedules run the same plans on kernels of their own for 1 x 1 and 2 x 2 tiles (cx_mv64chain.hip: k_compose_nt,
    // k_walk_nt).  CX_MFMA_DIM=64 forces 64 everywhere (A/B; a chain cut into time blocks: cx_chain_block_maps exchanges 64 x 64 potentials).
    cx_config padded;
    int user_dim = 0;
    if (config->dim > 4) {
        int internal = 64;
        const char *force = std::getenv("CX_MFMA_DIM");
        if (!(force && std::atoi(force) == 64)) internal = config->dim <= 16 ? 16 : config->dim <= 32 ? 32 : 64;
        user_dim = config->dim != internal ? config->dim : 0;
        padded = *config; padded.dim = internal; config = &padded;
    }
    const bool is_vmp = config->family == CX_FAMILY_VMP_MEAN_FIELD || config->family == CX_FAMILY_VMP_STRUCTURED;
    if (config->family != CX_FAMILY_GAUSSIAN && config->family != CX_FAMILY_NATURAL2 && !is_vmp)
        return fail(nullptr, CX_ERR_INVALID_ARGUMENT, "cx_create: unknown family");
    if (is_vmp && config->dim != 1)
        return fail(nullptr, CX_ERR_UNSUPPORTED, "cx_create: the variational families need dim == 1");
    if (config->family == CX_FAMILY_NATURAL2 && (config->dim != 1 || config->schedule == CX_SCHED_CHAIN_SCAN))
        return fail(nullptr, CX_ERR_UNSUPPORTED, "cx_create: CX_FAMILY_NATURAL2 needs dim == 1 and the flooding, fused, tree or reference schedule");
    // (round 6: the reference-order schedule for dim 64 too — and 5 .. 63 inside it: the stages through k_v2f64 / k_rule64w, cx_api_ref.hip)
    if (config->schedule == CX_SCHED_REFERENCE && is_vmp)
        return fail(nullptr, CX_ERR_UNSUPPORTED, "cx_create: CX_SCHED_REFERENCE replays the reference's execution order for the Gaussian and natural-pair families (the variational rules run under it as a wiring: cx_graph_wire)");
    if (config->dim > 1 && config->schedule != CX_SCHED_FUSED && config->schedule != CX_SCHED_CHAIN_SCAN && config->schedule != CX_SCHED_TREE && config->schedule != CX_SCHED_REFERENCE)
        return fail(nullptr, CX_ERR_UNSUPPORTED, "cx_create: dim > 1 runs the fused, the chain-scan, the tree and the reference-order schedule");
    if (config->schedule != CX_SCHED_FLOODING && config->schedule != CX_SCHED_FUSED && config->schedule != CX_SCHED_CHAIN_SCAN && config->schedule != CX_SCHED_TREE && config->schedule != CX_SCHED_REFERENCE)
        return fail(nullptr, CX_ERR_INVALID_ARGUMENT, "cx_create: unknown schedule");
    if (config->schedule == CX_SCHED_TREE && config->family == CX_FAMILY_VMP_MEAN_FIELD)
        return fail(nullptr, CX_ERR_UNSUPPORTED, "cx_create: the mean-field family has no inner sweep to schedule (flooding, fused or chain-scan are accepted and ignored; "
                                                 "the tree schedule is the structured family's, for state variables that form a forest)");
    if (config->reserved != 0 && config->reserved != 1)
        return fail(nullptr, CX_ERR_INVALID_ARGUMENT, "cx_create: cx_config.reserved must be 0 (ABI 2 - 3 called it sweeps_per_launch; the two-sweep launch, measured slower, was removed in ABI 4)");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, CX_ERR_NO_DEVICE, "cx_create: no HIP device visible (this library has no CPU fallback)");
    if (config->device < 0 || config->device >= ndev) return fail(nullptr, CX_ERR_INVALID_ARGUMENT, "cx_create: bad device ordinal");
    e = hipSetDevice(config->device);
    if (e != hipSuccess) return fail(nullptr, CX_ERR_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
    cx_handle *h = new (std::nothrow) cx_handle();
    if (!h) return fail(nullptr, CX_ERR_OUT_OF_MEMORY, "cx_create: host allocation failed");
    h->cfg = *config;
    h->user_dim = user_dim;
    h->nc = config->dim == 1 ? 2 : (cx::is_mfma_dim(config->dim) ? config->dim + config->dim * config->dim : config->dim + config->dim * (config->dim + 1) / 2);
    h->ncs = (config->dim >= 2 && config->dim <= 4) ? 2 * ((h->nc + 1) / 2) : h->nc;
    h->stream = nullptr;  // default stream until cx_set_stream
    *out = h;
    return CX_OK;
}

int32_t cx_destroy(cx_handle *h) {
    if (!h) return CX_OK;
    (void)hipSetDevice(h->cfg.device);
    (void)hipStreamSynchronize(h->stream);
    for (auto &r : h->recs) { (void)hipEventDestroy(r.start); (void)hipEventDestroy(r.stop); }
    cx::comm_destroy(h);
    cx::ipc_destroy(h);
    cx::vmp_free(h);
    dev_free_all(h);
    delete h;
    return CX_OK;
}

int32_t cx_sync(cx_handle *h) {
    CX_REQUIRE(h, h, CX_ERR_INVALID_ARGUMENT, "null handle");
    CX_HIP(h, hipStreamSynchronize(h->stream));
    return CX_OK;
}

int32_t cx_set_stream(cx_handle *h, void *hip_stream) {
    CX_REQUIRE(h, h, CX_ERR_INVALID_ARGUMENT, "null handle");
    CX_HIP(h, hipStreamSynchronize(h->stream));
    h->stream = (hipStream_t)hip_stream;
    return cx::vmp_set_stream(h);
}

// (re)upload the (P, B, C) rule tables of every registered parameter set (dim > 1)
static int32_t upload_ptab(cx_handle *h) {
    const int d = h->cfg.dim;
    const int64_t nsets = std::max<int64_t>((int64_t)h->psets.size(), h->max_pset + 1);
    if (nsets == 0) return CX_OK;
    const size_t per = (size_t)6 * d * d;
    std::vector<double> tab(per * nsets, std::numeric_limits<double>::quiet_NaN());
    for (int64_t i = 0; i < (int64_t)h->psets.size(); i++) {
        if (h->psets[i].empty()) continue;
        if (!cx::mv_rule_tables(d, h->psets[i].data(), h->psets[i].data() + d * d, &tab[per * i]))
            return fail(h, CX_ERR_INVALID_ARGUMENT, "cx_set_factor_matrices: Q of parameter set " + std::to_string(i) + " is not positive definite");
    }
    CX_HIP(h, hipStreamSynchronize(h->stream));
    // Captured sweeps hold the table pointers by value (cx_api_sweep.hip: tree_sweep; cx_api_ref.hip: run_entry): the tables are rewritten
    // IN PLACE while their size holds, and the graphs are dropped before a table that has to move goes (the next sweep captures again).
    if (h->d_ptab && h->ptab_sets < nsets) { captured_graphs_drop(h); h->d_ptab.reset(); }
    if (!h->d_ptab) { int32_t rc = dev_alloc(h, &h->d_ptab, (int64_t)(per * nsets)); if (rc != CX_OK) return rc; h->ptab_sets = nsets; }
    CX_HIP(h, hipMemcpy(h->d_ptab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
    if (cx::is_mfma_dim(d)) {   // the wave-per-message rule kernel reads B transposed (tile rows are its contraction index)
        const size_t dd = (size_t)d * d;
        std::vector<double> bt(2 * (size_t)nsets * dd);
        for (int64_t t = 0; t < 2 * nsets; t++) {
            const double *B = &tab[(size_t)t * 3 * dd + dd];
            for (int r = 0; r < d; r++) for (int c = 0; c < d; c++) bt[(size_t)t * dd + (size_t)r * d + c] = B[(size_t)c * d + r];
        }
        if (!h->d_zero_msg) {
            int32_t rc0 = dev_alloc(h, &h->d_zero_msg, (int64_t)(d + d * d));
            if (rc0 != CX_OK) return rc0;
            CX_HIP(h, hipMemset(h->d_zero_msg, 0, (size_t)(d + d * d) * 8));
        }
        if (h->d_ptab_bt && h->ptab_bt_sets < nsets) { captured_graphs_drop(h); h->d_ptab_bt.reset(); }
        if (!h->d_ptab_bt) {
            int32_t rc = dev_alloc(h, &h->d_ptab_bt, (int64_t)bt.size());
            if (rc != CX_OK) return rc;
            h->ptab_bt_sets = nsets;
        }
        CX_HIP(h, hipMemcpy(h->d_ptab_bt, bt.data(), bt.size() * 8, hipMemcpyHostToDevice));
    }
    return CX_OK;
}

int32_t cx_set_factor_matrices(cx_handle *h, int64_t parameter_set, const double *A, const double *Q) {
    CX_REQUIRE(h, h, CX_ERR_INVALID_ARGUMENT, "null handle");
    CX_REQUIRE(h, h->cfg.dim > 1, CX_ERR_STATE, "cx_set_factor_matrices: dim == 1 factors take scalar parameters");
    CX_REQUIRE(h, parameter_set >= 0 && parameter_set < (1 << 20) && A && Q, CX_ERR_INVALID_ARGUMENT, "cx_set_factor_matrices: bad argument");
    try {
        const int d = h->cfg.dim;
        std::vector<double> Ap, Qp;
        if (h->user_dim) {      // blockdiag(A, I), blockdiag(Q, I)
            const int u = h->user_dim;
            Ap.assign((size_t)d * d, 0.0); Qp.assign((size_t)d * d, 0.0);
            for (int r = 0; r < d; r++) { Ap[(size_t)r * d + r] = 1.0; Qp[(size_t)r * d + r] = 1.0; }
            for (int r = 0; r < u; r++) for (int c = 0; c < u; c++) { Ap[(size_t)r * d + c] = A[(size_t)r * u + c]; Qp[(size_t)r * d + c] = Q[(size_t)r * u + c]; }
            A = Ap.data(); Q = Qp.data();
        }
        if ((int64_t)h->psets.size() <= parameter_set) h->psets.resize(parameter_set + 1);
        auto &ps = h->psets[parameter_set];
        changed(*h, Change::RuleMatrices);      // (before the set is touched: a refused Q leaves it empty, which is a change too)
        ps.assign(A, A + d * d);
        ps.insert(ps.end(), Q, Q + d * d);
        std::vector<double> chk((size_t)6 * d * d);
        if (!cx::mv_rule_tables(d, A, Q, chk.data())) {
            ps.clear();
            return fail(h, CX_ERR_INVALID_ARGUMENT, "cx_set_factor_matrices: Q is not symmetric positive definite");
        }
        if (!h->has_graph) return CX_OK;
        if (h->cfg.schedule == CX_SCHED_CHAIN_SCAN) { int32_t rc0 = mv_ensure_chain_msgs(h); if (rc0 != CX_OK) return rc0; }   // under the old tables
        { const int32_t rc1 = upload_ptab(h); if (rc1 != CX_OK) return rc1; }
        if (h->has_offsets) {      // the offsets' linear terms, Q^-1 b and -A' Q^-1 b, follow the tables
            cx::mv_launch_offset_terms(h);
            CX_HIP(h, hipGetLastError());
        }
        return CX_OK;
    } catch (const std::bad_alloc &) { return fail(h, CX_ERR_OUT_OF_MEMORY, "cx_set_factor_matrices: host allocation failed"); }
}

// h->offsets (by factor) -> d_off_b (by slot, every slot: the arrays are small next to the messages) -> d_off_g (k_mv_offset_terms).
// dim 2 - 4: [d][nslots], component-major (a thread reads one component of many slots); the matrix-core dims: [nslots][d], one contiguous
// vector per slot (a wave reads one slot's), h->offsets in the user's dim and zeros in the padding of an embedded one (k_offset_terms64)
static int32_t upload_offsets(cx_handle *h) {
    const int d = h->cfg.dim, ud = h->user_dim ? h->user_dim : d;
    const bool mfma = cx::is_mfma_dim(d);
    const int64_t ns = h->nslots;
    std::vector<double> bs((size_t)d * ns, 0.0);
    for (int64_t f = 0; f < h->nf; f++)
        for (int k = 0; k < 2; k++) {
            const int32_t sl = h->off_fac_slots[2 * (size_t)f + k];
            if (sl < 0) continue;
            for (int i = 0; i < ud; i++) bs[mfma ? (size_t)sl * d + i : (size_t)i * ns + sl] = h->offsets[(size_t)f * ud + i];
        }
    CX_HIP(h, hipMemcpyAsync(h->d_off_b, bs.data(), bs.size() * 8, hipMemcpyHostToDevice, h->stream));
    cx::mv_launch_offset_terms(h);
    CX_HIP(h, hipGetLastError());
    CX_HIP(h, hipStreamSynchronize(h->stream));      // (bs dies here)
    return CX_OK;
}

// what cx_set_factor_offsets (dim 2 - 4) and cx_set_factor_offsets_mfma (dim 5 - 64) share, after each has checked the handle's dim:
// offsets is [n][the user's dim]
static int32_t set_factor_offsets(cx_handle *h, const std::string &who, int64_t n, const int64_t *factor_ids, const double *offsets) {
    CX_REQUIRE(h, h->has_graph, CX_ERR_STATE, who + ": no graph");
    CX_REQUIRE(h, h->cfg.schedule != CX_SCHED_REFERENCE, CX_ERR_UNSUPPORTED,
               who + ": not for CX_SCHED_REFERENCE handles or wirings (cx_graph_wire): the reference order has no d-dimensional offset to be pinned against");
    CX_REQUIRE(h, !h->chain_partition && !h->halo_state && h->send_slots.empty() && h->recv_slots.empty(), CX_ERR_UNSUPPORTED,
               who + ": not for a partitioned handle (halo lists, state halos or a chain's time block)");
    CX_REQUIRE(h, n >= 0 && (n == 0 || (factor_ids && offsets)), CX_ERR_INVALID_ARGUMENT, who + ": a negative count or a null array");
    CX_HIP(h, hipSetDevice(h->cfg.device));
    if (h->stream) {
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        CX_HIP(h, hipStreamIsCapturing(h->stream, &st));
        CX_REQUIRE(h, st == hipStreamCaptureStatusNone, CX_ERR_STATE, who + ": the handle's stream is being captured (the call is synchronous)");
    }
    try {
        const int d = h->user_dim ? h->user_dim : h->cfg.dim;      // (the caller's rows; the device arrays are cfg.dim wide)
        // everything is checked before anything changes
        std::vector<int64_t> fac((size_t)n);
        for (int64_t i = 0; i < n; i++) {
            const int64_t f = find_factor(h, factor_ids[i]);
            if (f < 0) return fail(h, CX_ERR_NOT_FOUND, who + ": no factor " + std::to_string(factor_ids[i]));
            if (h->fac_kind[(size_t)f] != CX_FACTOR_GAUSS_LINEAR)
                return fail(h, CX_ERR_UNSUPPORTED, who + ": factor " + std::to_string(factor_ids[i]) + " is not a two-variable CX_FACTOR_GAUSS_LINEAR factor");
            for (int k = 0; k < d; k++)
                if (!std::isfinite(offsets[i * d + k]))
                    return fail(h, CX_ERR_INVALID_ARGUMENT, who + ": the offset of factor " + std::to_string(factor_ids[i]) + " is not finite");
            fac[(size_t)i] = f;
        }
        if (h->cfg.schedule == CX_SCHED_CHAIN_SCAN) { const int32_t rc0 = mv_ensure_chain_msgs(h); if (rc0 != CX_OK) return rc0; }   // under the old offsets
        int32_t rc;
        if (!h->has_offsets) {
            // the factors' slots; per slot the rule table of the messages INTO it: what its partner sends (unmasked: an observed
            // receiver's slot has a term too, read when it is the sender's)
            h->off_fac_slots.assign((size_t)2 * h->nf, -1);
            for (int64_t e = 0; e < h->ne; e++) {
                const int64_t f = find_factor(h, h->edge_fac_id[e]);
                if (h->fac_kind[(size_t)f] != CX_FACTOR_GAUSS_LINEAR) continue;
                int32_t *fs = &h->off_fac_slots[2 * (size_t)f];
                fs[fs[0] < 0 ? 0 : 1] = cx::slot_of_edge(h, e);
            }
            std::vector<int32_t> rt((size_t)h->nslots, -1);
            for (int64_t f = 0; f < h->nf; f++) {
                const int32_t s0 = h->off_fac_slots[2 * (size_t)f], s1 = h->off_fac_slots[2 * (size_t)f + 1];
                if (s0 < 0 || s1 < 0 || h->partner[s0] != s1) { h->off_fac_slots[2 * (size_t)f] = h->off_fac_slots[2 * (size_t)f + 1] = -1; continue; }
                rt[s0] = h->spdir[s1]; rt[s1] = h->spdir[s0];
            }
            CX_HIP(h, hipStreamSynchronize(h->stream));
            captured_graphs_drop(h);      // a captured sweep names the kernels' instances without offsets
            if ((rc = dev_upload(h, &h->d_off_rt, rt)) != CX_OK) return rc;
            if ((rc = dev_alloc(h, &h->d_off_b, (int64_t)h->cfg.dim * h->nslots)) != CX_OK) return rc;
            if ((rc = dev_alloc(h, &h->d_off_g, (int64_t)h->cfg.dim * h->nslots)) != CX_OK) return rc;
            if (cx::is_mfma_dim(h->cfg.dim) && (rc = dev_alloc(h, &h->d_off_kappa, h->nslots)) != CX_OK) return rc;
            CX_HIP(h, hipStreamSynchronize(h->stream));      // (rt dies here)
            h->offsets.assign((size_t)h->nf * d, 0.0);
            h->has_offsets = true;
            // the matrix-core dims' chain plans (chain scan, heavy paths of the tree schedule) name the links' linear terms: built again, once
            if (cx::is_mfma_dim(h->cfg.dim)) { h->chains_dirty = true; h->tree_dirty = true; }      // (work site: the plans were built without the kOff space)
        }
        changed(*h, Change::RuleOffsets);
        for (int64_t i = 0; i < n; i++) std::copy(offsets + i * d, offsets + (i + 1) * d, h->offsets.begin() + fac[(size_t)i] * d);
        h->offsets_nonzero = std::any_of(h->offsets.begin(), h->offsets.end(), [](double v) { return v != 0.0; });
        return upload_offsets(h);
    } catch (const std::bad_alloc &) { return fail(h, CX_ERR_OUT_OF_MEMORY, who + ": host allocation failed"); }
}

int32_t cx_set_factor_offsets(cx_handle *h, int64_t n, const int64_t *factor_ids, const double *offsets) {
    const std::string who = "cx_set_factor_offsets";
    CX_REQUIRE(h, h, CX_ERR_INVALID_ARGUMENT, "null handle");
    CX_REQUIRE(h, h->cfg.family == CX_FAMILY_GAUSSIAN, CX_ERR_UNSUPPORTED, who + ": the Gaussian family only");
    CX_REQUIRE(h, h->cfg.dim != 1, CX_ERR_STATE, who + ": dim 1 factors carry b in their parameters (CX_FACTOR_GAUSS_LINEAR: params[2])");
    CX_REQUIRE(h, h->cfg.dim <= 4 && !h->user_dim, CX_ERR_UNSUPPORTED, who + ": dim 2, 3 and 4 (the matrix-core dims, 5 - 64: cx_set_factor_offsets_mfma)");
    return set_factor_offsets(h, who, n, factor_ids, offsets);
}

int32_t cx_set_factor_offsets_mfma(cx_handle *h, int64_t n, const int64_t *factor_ids, const double *offsets) {
    const std::string who = "cx_set_factor_offsets_mfma";
    CX_REQUIRE(h, h, CX_ERR_INVALID_ARGUMENT, "null handle");
    CX_REQUIRE(h, h->cfg.family == CX_FAMILY_GAUSSIAN, CX_ERR_UNSUPPORTED, who + ": the Gaussian family only");
    CX_REQUIRE(h, cx::is_mfma_dim(h->cfg.dim), CX_ERR_UNSUPPORTED, who + ": dim 5 - 64 (dim 2, 3 and 4: cx_set_factor_offsets; dim 1 factors carry b in their parameters)");
    return set_factor_offsets(h, who, n, factor_ids, offsets);
}


int32_t cx_graph_create(cx_handle *h, int64_t n_edges, const int64_t *edge_var, const int64_t *edge_fac,
                        const int32_t *edge_role, int64_t n_factors, const int64_t *factor_ids,
                        const int32_t *factor_kind, const double *factor_params) {
    CX_REQUIRE(h, h, CX_ERR_INVALID_ARGUMENT, "null handle");
    CX_REQUIRE(h, !h->has_graph, CX_ERR_STATE, "cx_graph_create: handle already has a graph");
    CX_REQUIRE(h, n_edges > 0 && edge_var && edge_fac, CX_ERR_INVALID_ARGUMENT, "cx_graph_create: empty edge list");
    CX_REQUIRE(h, n_edges < (int64_t)0x0fffffff, CX_ERR_UNSUPPORTED, "cx_graph_create: more than 2^28-1 edges per handle");
    if (is_vmp(h)) {
        CX_REQUIRE(h, n_factors > 0 && factor_ids && factor_kind, CX_ERR_INVALID_ARGUMENT, "cx_graph_create: factor table missing");
        int32_t rc = cx::vmp_graph_create(h, n_edges, edge_var, edge_fac, edge_role, n_factors, factor_ids, factor_kind);
        if (rc != CX_OK) cx::vmp_free(h);
        return rc;
    }
    CX_REQUIRE(h, n_factors > 0 && factor_ids && factor_kind && factor_params, CX_ERR_INVALID_ARGUMENT,
               "cx_graph_create: factor table missing");
    try {
        cx::flat::Out fo;
        std::string ferr;
        {
            const int32_t frc = cx::flat::flatten(h, n_edges, edge_var, edge_fac, edge_role, n_factors, factor_ids, factor_kind, factor_params, fo, ferr);
            if (frc != CX_OK) return fail(h, frc, ferr);
        }
        changed(*h, Change::GraphCreated);
        const int64_t ne = h->ne, nv = h->nv, slots = h->nslots, big_total = fo.big_total;
        const bool mv = fo.mv;
        std::vector<int32_t> &var_deg = fo.var_deg, &spdir = fo.spdir;
        std::vector<double> &q = fo.q, &a = fo.a, &b = fo.b, &sq = fo.sq, &sa = fo.sa, &sb = fo.sb;
        (void)ne;
        // ---- upload ------------------------------------------------------------------------------------------------
        CX_HIP(h, hipSetDevice(h->cfg.device));
        int32_t rc;
#define CX_TRY(x) do { rc = (x); if (rc != CX_OK) { dev_free_all(h); return rc; } } while (0)
        CX_TRY(dev_upload(h, &h->d_slice_off, h->slice_off));
        CX_TRY(dev_upload(h, &h->d_partner, h->partner));
        {   // the partners as 16-bit differences, where they all fit (grids, chains, banded graphs: the fused sweep then reads 2 bytes per slot)
            std::vector<int16_t> p16(h->partner.size());
            bool fits = !h->partner.empty();
            for (size_t sl = 0; sl < h->partner.size() && fits; sl++) {
                const int64_t pp = h->partner[sl], dl = pp - (int64_t)sl;
                if (pp < 0) p16[sl] = -32768;
                else if (dl < -32767 || dl > 32767) fits = false;
                else p16[sl] = (int16_t)dl;
            }
            if (fits) {
                CX_TRY(dev_upload(h, &h->d_partner16, p16));
                // ... and as wave-uniform runs (cx_partner_runs.h): built only with the differences — the packed sweep is their only reader
                std::vector<cx::pruns::Entry> runs;
                h->partner_run_fallback = cx::pruns::build(h->partner, h->slice_off, h->vinfo, h->nv, runs);
                h->partner_run_entries = (int64_t)runs.size();
                static_assert(sizeof(cx::pruns::Entry) == 16, "four words per entry");
                std::vector<int32_t> words(runs.size() * 4);
                if (!runs.empty()) std::memcpy(words.data(), runs.data(), words.size() * 4);
                CX_TRY(dev_upload(h, &h->d_partner_runs, words));
            }
        }
        CX_TRY(dev_upload(h, &h->d_vbase, h->vbase));
        CX_TRY(dev_upload(h, &h->d_var_deg, var_deg));
        CX_TRY(dev_upload(h, &h->d_vinfo, h->vinfo));
        CX_TRY(dev_upload(h, &h->d_big, h->big_vars));
        CX_TRY(dev_upload(h, &h->d_big_slots, h->big_slots));
        if (mv && !h->big_vars.empty()) {
            std::vector<int32_t> sv;
            sv.reserve(h->big_slots.size());
            for (int32_t v : h->big_vars) sv.insert(sv.end(), (size_t)var_deg[v], v);
            CX_TRY(dev_upload(h, &h->d_big_slot_var, sv));
        }
        CX_TRY(dev_alloc(h, &h->d_big_tmp, big_total));
        CX_TRY(dev_alloc(h, &h->d_scratch, 4096));
        if (mv) {
            const int64_t nc = h->nc, ncs = h->ncs;
            h->spdir = spdir;
            CX_TRY(dev_upload(h, &h->d_spdir, spdir));
            CX_TRY(dev_alloc(h, &h->d_mv_f2v, ncs * slots)); CX_TRY(dev_alloc(h, &h->d_mv_f2v_alt, ncs * slots));
            CX_TRY(dev_alloc(h, &h->d_mv_v2f, ncs * slots)); CX_TRY(dev_alloc(h, &h->d_mv_marg, cx::is_mfma_dim(h->cfg.dim) ? 1 : ncs * h->nslices * cx::kBlock));      // pair form by variable, whole 256-blocks
            CX_HIP(h, hipMemsetAsync(h->d_mv_f2v, 0xff, (size_t)(ncs * slots) * 8, h->stream));
            CX_HIP(h, hipMemsetAsync(h->d_mv_f2v_alt, 0xff, (size_t)(ncs * slots) * 8, h->stream));
            CX_HIP(h, hipMemsetAsync(h->d_mv_v2f, 0xff, (size_t)(ncs * slots) * 8, h->stream));
            if (!cx::is_mfma_dim(h->cfg.dim)) CX_HIP(h, hipMemsetAsync(h->d_mv_marg, 0xff, (size_t)(ncs * h->nslices * cx::kBlock) * 8, h->stream));
            CX_HIP(h, hipStreamSynchronize(h->stream));
            if (h->cfg.schedule == CX_SCHED_REFERENCE) CX_TRY(ref_build(h));      // dim 2 .. 4: the same wiring and shadow, the stages through k_batch_mv
            h->has_graph = true;
            return upload_ptab(h);
        }
        CX_TRY(dev_upload(h, &h->d_q, q));
        if (h->any_linear) {
            CX_TRY(dev_upload(h, &h->d_a, a)); CX_TRY(dev_upload(h, &h->d_b, b));
            CX_TRY(dev_upload(h, &h->d_sq, sq)); CX_TRY(dev_upload(h, &h->d_sa, sa)); CX_TRY(dev_upload(h, &h->d_sb, sb));
        }
        CX_TRY(dev_alloc(h, &h->d_f2v, slots)); CX_TRY(dev_alloc(h, &h->d_v2f, slots)); CX_TRY(dev_alloc(h, &h->d_marg, nv));
        // every message starts as UndefValue(): all-ones bytes are a NaN in both halves of each double2
        CX_HIP(h, hipMemsetAsync(h->d_f2v, 0xff, (size_t)slots * sizeof(double2), h->stream));
        CX_HIP(h, hipMemsetAsync(h->d_v2f, 0xff, (size_t)slots * sizeof(double2), h->stream));
        CX_HIP(h, hipMemsetAsync(h->d_marg, 0xff, (size_t)nv * sizeof(double2), h->stream));
        if (h->cfg.schedule == CX_SCHED_FUSED) {
            CX_TRY(dev_alloc(h, &h->d_f2v_alt, slots));
            CX_HIP(h, hipMemsetAsync(h->d_f2v_alt, 0xff, (size_t)slots * sizeof(double2), h->stream));
            // a grid of additive Gaussian factors: the plan of the paired sweep (cx_lattice_plan.h; cx_api_sweep.hip: cx_sweep runs it)
            if (h->cfg.family == CX_FAMILY_GAUSSIAN && !h->any_linear && h->n_kary == 0 && h->big_vars.empty()) {
                const cx::lattice::Plan pl = cx::lattice::build(h->partner, h->slice_off, h->vinfo, h->nv, q.data());
                h->pair_refused = pl.reason;
                if (pl.ok && h->pair_abort.alloc() && h->d_pair_flag.alloc(h, 1) == CX_OK) { h->pair_H = pl.H; h->pair_W = pl.W; h->pair_block_cols = pl.block_cols; }
            } else h->pair_refused = "not a fused scalar handle of additive Gaussian factors";
        }
#undef CX_TRY
#define CX_TRY2(x) do { int32_t rc2_ = (x); if (rc2_ != CX_OK) { dev_free_all(h); return rc2_; } } while (0)
        CX_HIP(h, hipStreamSynchronize(h->stream));
        if (h->n_kary) { if (h->slot_kary.empty()) h->slot_kary.assign(slots, -1); CX_TRY2(cx::kary_upload(h)); }
        if (h->cfg.schedule == CX_SCHED_REFERENCE) CX_TRY2(ref_build(h));      // the default resolver's wiring + the shadow of the readiness state
        h->has_graph = true;
        return CX_OK;
    } catch (const std::bad_alloc &) {
        return fail(h, CX_ERR_OUT_OF_MEMORY, "cx_graph_create: host allocation failed");
    } catch (const std::exception &ex) {
        return fail(h, CX_ERR_INVALID_ARGUMENT, std::string("cx_graph_create: ") + ex.what());
    }
}

int32_t cx_graph_stats(const cx_handle *h, cx_stats *out) {
    if (!h || !out) return CX_ERR_INVALID_ARGUMENT;
    out->n_variables = h->nv; out->n_factors = h->nf; out->n_edges = h->ne;
    out->n_messages_per_sweep = h->n_messages_per_sweep;
    out->n_slices = h->nslices; out->n_big_variables = (int64_t)h->big_vars.size(); out->n_slots = h->nslots;
    out->device_bytes = h->device_bytes; out->sweeps_done = h->sweeps_done;
    return CX_OK;
}

// tiles of the two-sweep launches (built on the first cx_sweep(n >= 2) of a fused scalar handle)

int32_t cx_edge_index(const cx_handle *hc, int64_t n, const int64_t *variable_ids, const int64_t *factor_ids, int64_t *out_edge) {
    cx_handle *h = const_cast<cx_handle *>(hc);
    CX_REQUIRE(h, h && h->has_graph, CX_ERR_STATE, "cx_edge_index: no graph");
    CX_REQUIRE(h, n >= 0 && (n == 0 || (variable_ids && factor_ids && out_edge)), CX_ERR_INVALID_ARGUMENT, "cx_edge_index: null argument");
    for (int64_t i = 0; i < n; i++) {
        out_edge[i] = find_edge(h, variable_ids[i], factor_ids[i]);
        if (out_edge[i] < 0)
            return fail(h, CX_ERR_NOT_FOUND, "no connection between variable " + std::to_string(variable_ids[i]) + " and factor " + std::to_string(factor_ids[i]));
    }
    return CX_OK;
}


}  // extern "C"
