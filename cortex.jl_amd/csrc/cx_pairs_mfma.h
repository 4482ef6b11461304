// cx_pairs_mfma.h — the host pieces that the readers of the stored messages at the matrix-core dims share (cx_predict_mfma.hip,
// cx_causal_mfma.hip): what the graph says about its two-variable rule factors, and the refusals of a call.
#pragma once
#include <string>
#include <utility>
#include <vector>

#include "cx_host.h"

namespace cx {
namespace prm {

// what the graph says about the two-variable rule factors: by factor index the slots and variables of (out, in) and the parameter set
struct Pairs {
    std::vector<int32_t> so, si, vo, vi, set;      // so < 0: no two-variable CX_FACTOR_GAUSS_LINEAR factor
    int64_t unsupported_fac = -1;
};

inline void pairs_of(const cx_handle *h, Pairs &P) {
    using namespace cxh;
    const int64_t ne = h->ne, nf = h->nf;
    std::vector<int32_t> fe1((size_t)nf, -1), fe2((size_t)nf, -1), nfe((size_t)nf, 0);
    for (int64_t e = 0; e < ne; e++) {
        const int64_t f = find_factor(h, h->edge_fac_id[e]);
        if (fe1[f] < 0) fe1[f] = (int32_t)e; else if (fe2[f] < 0) fe2[f] = (int32_t)e;
        nfe[f]++;
    }
    P.so.assign((size_t)nf, -1); P.si.assign((size_t)nf, -1); P.vo.assign((size_t)nf, -1); P.vi.assign((size_t)nf, -1); P.set.assign((size_t)nf, -1);
    P.unsupported_fac = -1;
    for (int64_t f = 0; f < nf; f++) {
        if (h->fac_kind[f] == CX_FACTOR_OPAQUE) continue;
        if (h->fac_kind[f] != CX_FACTOR_GAUSS_LINEAR || nfe[f] != 2) { if (P.unsupported_fac < 0) P.unsupported_fac = h->fac_ids[f]; continue; }
        const int32_t s1 = slot_of_edge(h, fe1[f]), s2 = slot_of_edge(h, fe2[f]);
        int32_t so = s1, si = s2, vo = h->edge_var[fe1[f]], vi = h->edge_var[fe2[f]];
        if ((h->spdir[s1] & 1) == 0) { std::swap(so, si); std::swap(vo, vi); }      // spdir[in slot] = 2 set (the message it sends goes forward)
        P.so[f] = so; P.si[f] = si; P.vo[f] = vo; P.vi[f] = vi; P.set[f] = h->spdir[si] >> 1;
    }
}

// the refusals of cx_log_evidence_mfma under this call's name; `small`: the call for dims 1 .. 4, `what`: what the other families lack
inline int32_t prepare(cx_handle *h, const std::string &who, const char *bad_args, const char *small = "cx_predictive", const char *what = "predictive") {
    using namespace cxh;
    CX_REQUIRE(h, !h || h->cfg.family == CX_FAMILY_GAUSSIAN, CX_ERR_UNSUPPORTED, who + ": the Gaussian family only (the variational and Beta-Bernoulli families have no Gaussian " + what + ")");
    CX_REQUIRE(h, h && h->has_graph, CX_ERR_STATE, who + ": no graph");
    CX_REQUIRE(h, !bad_args, CX_ERR_INVALID_ARGUMENT, who + ": " + (bad_args ? bad_args : ""));
    CX_REQUIRE(h, cx::is_mfma_dim(h->cfg.dim), CX_ERR_UNSUPPORTED, who + ": the matrix-core dims, 5 .. 64 (dim 1, 2, 3 and 4: " + small + ")");
    CX_REQUIRE(h, !h->chain_partition && !h->halo_state && h->send_slots.empty() && h->recv_slots.empty(), CX_ERR_UNSUPPORTED,
               who + ": not for a partitioned handle (halo lists, state halos or a chain's time block: its rows would need owners)");
    CX_HIP(h, hipSetDevice(h->cfg.device));
    if (h->stream) {
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        CX_HIP(h, hipStreamIsCapturing(h->stream, &st));
        CX_REQUIRE(h, st == hipStreamCaptureStatusNone, CX_ERR_STATE, who + ": the handle's stream is being captured (the call is synchronous)");
    }
    // (mv_check_psets' conditions under this call's name; behind them the tables are on the device: the check below is a guard)
    CX_REQUIRE(h, (int64_t)h->psets.size() > h->max_pset, CX_ERR_STATE, who + ": a factor names a parameter set that was never set (cx_set_factor_matrices)");
    for (int64_t i = 0; i <= h->max_pset; i++)
        CX_REQUIRE(h, !h->psets[i].empty(), CX_ERR_STATE, who + ": parameter set " + std::to_string(i) + " was never set (cx_set_factor_matrices)");
    CX_REQUIRE(h, h->d_ptab && h->d_ptab_bt && h->d_mv_f2v && h->d_mv_v2f, CX_ERR_STATE, who + ": the rule tables are not on the device (cx_set_factor_matrices)");
    return CX_OK;
}

// the pairs of the graph (O(connections) on the host: for a new request only), refused when a factor of another kind exists
inline int32_t checked_pairs(cx_handle *h, const std::string &who, Pairs &P) {
    using namespace cxh;
    pairs_of(h, P);
    if (P.unsupported_fac >= 0)
        return fail(h, CX_ERR_UNSUPPORTED, who + ": factor " + std::to_string(P.unsupported_fac) + " is no two-variable CX_FACTOR_GAUSS_LINEAR factor and no opaque message");
    return CX_OK;
}

}  // namespace prm
}  // namespace cx
