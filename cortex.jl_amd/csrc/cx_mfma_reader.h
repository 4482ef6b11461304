// cx_mfma_reader.h — the host kit of the readers of the stored messages at the matrix-core dims: cx_evidence_mfma.hip, cx_learn_mfma.hip,
// cx_disturb_mfma.hip, cx_predict_mfma.hip, cx_causal_mfma.hip and cx_sample_mfma.hip.  What the graph says about its two-variable rule factors, the refusals of a call, the key
// of the last request, a parameter table that follows param_epoch, the payload through a bounded device buffer, the totals of a call and
// the choice of the tile count.  The wave side: cx_evidence_mfma_core.h.
#pragma once
#include <algorithm>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "cx_evidence_core.h"
#include "cx_host.h"

namespace cx {
namespace mfr {

// the user's dim: below the internal one (cfg.dim, a multiple of the tile) for an embedded model
inline int user_dim(const cx_handle *h) { return h->user_dim ? h->user_dim : h->cfg.dim; }
// The flat-pivot factor (evm::flat_pivot): a message that carries no information arrives as the rounding of u-term sums (DESIGN.md
// §4o: the measured remainders)
inline double flat_pivot_factor(const cx_handle *h) { return 64.0 * user_dim(h) * 2.220446049250313e-16; }

// f(tile count as a compile-time constant) for the handle's internal dim of 16, 32 or 64
template <class F>
inline void for_tiles(int dim, F f) {
    if (dim == 16) f(std::integral_constant<int, 1>{});
    else if (dim == 32) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 4>{});
}

// ---- the graph ------------------------------------------------------------------------------------------------------------------------
// what the graph says about the two-variable rule factors: by factor index the slots and variables of (out, in) and the parameter set;
// by connection the factor index
struct Pairs {
    std::vector<int32_t> so, si, vo, vi, set;      // so < 0: no two-variable CX_FACTOR_GAUSS_LINEAR factor
    std::vector<int32_t> efac;
    int64_t unsupported_fac = -1;                  // the first factor that is neither such a factor nor an opaque message
};

inline void pairs_of(const cx_handle *h, Pairs &P) {
    using namespace cxh;
    const int64_t ne = h->ne, nf = h->nf;
    std::vector<int32_t> fe1((size_t)nf, -1), fe2((size_t)nf, -1), nfe((size_t)nf, 0);
    P.efac.resize((size_t)ne);
    for (int64_t e = 0; e < ne; e++) {
        const int64_t f = find_factor(h, h->edge_fac_id[e]);
        P.efac[e] = (int32_t)f;
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

inline int32_t refuse_factor(cx_handle *h, const std::string &who, int64_t id) {
    return cxh::fail(h, CX_ERR_UNSUPPORTED, who + ": factor " + std::to_string(id) + " is no two-variable CX_FACTOR_GAUSS_LINEAR factor and no opaque message");
}
// the pairs of the graph (O(connections) on the host: for a new request only), refused when a factor of another kind exists
inline int32_t checked_pairs(cx_handle *h, const std::string &who, Pairs &P) {
    pairs_of(h, P);
    return P.unsupported_fac >= 0 ? refuse_factor(h, who, P.unsupported_fac) : CX_OK;
}

// a run of message slots (or sources) in a list
struct Run { int32_t off = 0, n = 0; };
// appends the message slots of variable v that `keep` takes, in ascending neighbour order (k_v2f64's)
template <class Keep>
inline Run slots_where(const cx_handle *h, int32_t v, std::vector<int32_t> &srcs, Keep keep) {
    Run r;
    r.off = (int32_t)srcs.size();
    for (int32_t e = h->var_off[v]; e < h->var_off[v + 1]; e++) {
        const int32_t s = slot_of_edge(h, e);
        if (keep(s)) srcs.push_back(s);
    }
    r.n = (int32_t)srcs.size() - r.off;
    return r;
}
// the slots of variable v but `skip` (-1: all of them)
inline Run other_slots(const cx_handle *h, int32_t v, int32_t skip, std::vector<int32_t> &srcs) {
    return slots_where(h, v, srcs, [skip](int32_t s) { return s != skip; });
}

// ---- the refusals of a call ---------------------------------------------------------------------------------------------------------------
// the words of a caller: the call for dims 1 .. 4, what the other families lack, what a partitioned handle would need owners for
// takes_offsets: the call reads the factor offsets of cx_set_factor_offsets_mfma; the others refuse while one is non-zero
struct Words { const char *small, *lack, *owners; bool takes_offsets = false; };

inline int32_t prepare(cx_handle *h, const std::string &who, const char *bad_args, const Words &w) {
    using namespace cxh;
    CX_REQUIRE(h, !h || h->cfg.family == CX_FAMILY_GAUSSIAN, CX_ERR_UNSUPPORTED, who + ": the Gaussian family only (" + w.lack + ")");
    CX_REQUIRE(h, h && h->has_graph, CX_ERR_STATE, who + ": no graph");
    CX_REQUIRE(h, !bad_args, CX_ERR_INVALID_ARGUMENT, who + ": " + (bad_args ? bad_args : ""));
    CX_REQUIRE(h, cx::is_mfma_dim(h->cfg.dim), CX_ERR_UNSUPPORTED, who + ": the matrix-core dims, 5 .. 64 (dim 1, 2, 3 and 4: " + w.small + ")");
    // (a user wiring, cx_graph_wire, cannot exist here: it is refused at these dims)
    CX_REQUIRE(h, !h->chain_partition && !h->halo_state && h->send_slots.empty() && h->recv_slots.empty(), CX_ERR_UNSUPPORTED,
               who + ": not for a partitioned handle (halo lists, state halos or a chain's time block: its " + w.owners + " would need owners)");
    // factor offsets at these dims: a reader that does not take them refuses while one is non-zero (dim 2 - 4's rule for its uncovered
    // readers) — none computes as if b were 0
    CX_REQUIRE(h, w.takes_offsets || !h->offsets_nonzero, CX_ERR_UNSUPPORTED, who + ": the handle has non-zero factor offsets (cx_set_factor_offsets_mfma), which this call does not implement");
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

// ---- what is kept between calls -------------------------------------------------------------------------------------------------------
// The last request: a tag (mode, lag or not, number of groups), the caller's ids or none, and with them a second array (groups).  What a
// new vinfo_epoch does to a plan is its owner's business: the key only says whether the caller asks what they asked last time.
struct RequestKey {
    bool valid = false, explicit_ids = false;
    int64_t tag = 0;
    std::vector<int64_t> ids, second;
    bool matches(int64_t t, int64_t n, const int64_t *i, const int64_t *s = nullptr) const {
        return valid && tag == t && explicit_ids == (i != nullptr) &&
               (!i || ((int64_t)ids.size() == n && std::equal(i, i + n, ids.begin()) && (!s || std::equal(s, s + n, second.begin()))));
    }
    void remember(int64_t t, int64_t n, const int64_t *i, const int64_t *s = nullptr) {
        tag = t;
        explicit_ids = i != nullptr;
        ids.assign(i, i ? i + n : i);
        second.assign(s, s ? s + n : s);
        valid = true;
    }
};

// A table made from the parameter sets, on the device, made again when the rule parameters change (param_epoch).  fill(t): the table
// into the host vector t
struct ParamTable {
    DevBuf<double> d;
    uint64_t epoch = ~0ull;
    template <class Fill>
    int32_t refresh(cx_handle *h, Fill fill) {
        if (epoch == h->param_epoch && d) return CX_OK;
        std::vector<double> t;
        fill(t);
        int32_t rc;
        if ((rc = d.ensure(h, (int64_t)t.size())) != CX_OK) return rc;
        CX_HIP(h, hipMemcpyAsync(d, t.data(), t.size() * 8, hipMemcpyHostToDevice, h->stream));
        CX_HIP(h, hipStreamSynchronize(h->stream));
        epoch = h->param_epoch;
        return CX_OK;
    }
};

// ---- a call's results ---------------------------------------------------------------------------------------------------------------------
constexpr int64_t kRowBufBytes = (int64_t)32 << 20;      // the device row buffer: a payload goes to the host a chunk at a time

// n_rows rows of per_row doubles to `out` through `buf`; launch(row0, n, d_rows) computes rows [row0, row0 + n) into d_rows.  Nothing waits
// here: the copies are in stream order, the caller synchronises (read_totals)
template <class Launch>
inline int32_t stream_rows(cx_handle *h, int64_t n_rows, int64_t per_row, DevBuf<double> &buf, double *out, Launch launch) {
    if (!n_rows) return CX_OK;
    const int64_t chunk = std::min<int64_t>(n_rows, std::max<int64_t>(1, kRowBufBytes / (per_row * 8)));
    int32_t rc;
    if ((rc = buf.ensure(h, chunk * per_row)) != CX_OK) return rc;
    for (int64_t r0 = 0; r0 < n_rows; r0 += chunk) {
        const int64_t m = std::min(chunk, n_rows - r0);
        launch(r0, m, buf.get());
        CX_HIP(h, hipGetLastError());
        CX_HIP(h, hipMemcpyAsync(out + r0 * per_row, buf, (size_t)(m * per_row) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    return CX_OK;
}

// the status of a row, and 256 (value, status) -> one ev::Part (fixed-order tree); rval null: statuses alone
constexpr int kRowOk = 0, kRowUndefined = 1, kRowImproper = 2;
constexpr int kTB = 256;
template <int TB>
__global__ __launch_bounds__(TB) void k_status_part(int n, const double *__restrict__ rval, const uint8_t *__restrict__ rflag, ev::Part *__restrict__ part) {
    const int i = blockIdx.x * TB + threadIdx.x;
    const double s = (rval && i < n) ? rval[i] : 0.0;
    const int f = i < n ? (int)rflag[i] : -1;
    ev::block_part<TB>(s, 0.0, f == kRowOk, f == kRowUndefined, f == kRowImproper, 0u, part);
}

// The tail of a call: ev::final_sum adds the nb parts in index order, the value and the counters come to the host, the stream is waited
// for.  counts4 = {n0, the three counters}; the value is returned in *total
struct Totals {
    DevBuf<double> d_out;
    std::vector<double> h_out;
    int32_t read(cx_handle *h, int64_t nb, const ev::Part *part, int64_t n0, int64_t *counts4, double *total) {
        int32_t rc;
        if (!d_out && (rc = cxh::dev_alloc(h, &d_out, 1 + ev::kNCnt)) != CX_OK) return rc;
        h_out.assign(1 + ev::kNCnt, 0.0);
        ev::final_sum(h, nb, part, d_out);
        CX_HIP(h, hipGetLastError());
        CX_HIP(h, hipMemcpyAsync(h_out.data(), d_out, (1 + ev::kNCnt) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        CX_HIP(h, hipStreamSynchronize(h->stream));
        uint64_t cnt[ev::kNCnt];
        std::memcpy(cnt, h_out.data() + 1, sizeof(cnt));
        counts4[0] = n0;
        for (int k = 1; k < 4; k++) counts4[k] = (int64_t)cnt[k - 1];
        *total = h_out[0];
        return CX_OK;
    }
    // the same of row statuses (and values, or null); a template, so that only its callers hold the kernel
    template <int TB = kTB>
    int32_t read_rows(cx_handle *h, int64_t n, const double *rval, const uint8_t *rflag, ev::Part *part, int64_t *counts4, double *total) {
        const int64_t nb = (n + TB - 1) / TB;
        if (n) hipLaunchKernelGGL(k_status_part<TB>, dim3((unsigned)nb), dim3(TB), 0, h->stream, (int)n, rval, rflag, part);
        return read(h, nb, part, n, counts4, total);
    }
};

}  // namespace mfr
}  // namespace cx
