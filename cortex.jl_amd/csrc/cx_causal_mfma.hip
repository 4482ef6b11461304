// cx_causal_mfma.hip — cx_causal_marginals_mfma: cx_causal_marginals at the matrix-core dims (cx_create dim 5 .. 64,
// internal tiles of 16 / 32 / 64): the predicted, filtered and fixed-lag-smoothed marginal of every non-observed variable from the
// stored factor→variable messages.  DESIGN.md §4p; the classes of the messages into a non-observed variable i are cx_predictive_mfma's:
//   U  an opaque message, or a rule factor on which i is the CX_ROLE_OUT end
//   O  a rule factor on which i is the CX_ROLE_IN end and whose OUT end is observed
//   T  a rule factor on which i is the CX_ROLE_IN end and whose OUT end is not observed
//   predicted = Σ U,   filtered = Σ U + Σ O,   fixed lag L = Σ U + Σ O + Σ_T β^(L)
//   β_a^(0) = flat;  β_a^(s) = the factor's rule towards i applied to  Σ O_j + Σ_{a' ∈ T_j} β_{a'}^(s-1),  j the OUT end of a
// Sums of the messages that are kept, never the belief minus what is left out.
//
//   k_cmm_presum  one wave per variable j with more than three sources: their sum into a scratch record (the rule takes three)
//   k_cmm_back    launched L times, one wave per T entry, double-buffered over β: rule64w_apply (cx_mv64w_core.h) on the sending
//                 slot's tables, its sources plain record pointers — O slots in the stored messages, T entries in β^(s-1).  An entry
//                 whose nearest datum downstream is more than s transitions away (the host plan's distance) stores exact zeros: the
//                 rule would leave the rounding of C - Yt'Yt, a "precision" of either sign.  Where the rule returns false (a NaN
//                 input, M not positive definite) it has stored nothing: the record becomes NaN, and a row that sums it is undefined
//   k_cmm_rows    one wave per row in the form of k_prm_rows (cx_predict_mfma.hip) without its second factorisation: the kept records
//                 summed in ascending neighbour order, Λ = U'U, z = U^-T η, Z = U^-T (lower block triangle), cov = Z'Z, mean = Z'z;
//                 an observed row is its datum and zeros.  Statuses as there: UNDEFINED when a stored message into i (kept or not)
//                 or a summed β holds NaN, otherwise IMPROPER when nothing is kept, a pivot below u is not positive and finite, or a
//                 pivot is at or below kFlat times the same diagonal entry of the sum of ALL stored messages into i
//   the row statuses are folded 256 to one ev::Part (cx_mfma_reader.h); ev::final_sum adds the parts in index order: no atomics
#include <algorithm>
#include <climits>

#include "cx_evidence_mfma_core.h"
#include "cx_mfma_reader.h"

namespace cx {
namespace cmm {

using namespace w64;
using evm::add_records, evm::any_nan_record, evm::factor_solve, evm::flat_pivot, evm::pad_identity, evm::park_z, evm::solve_identity_cols, evm::store_symmetric;

constexpr int kFinite = mfr::kRowOk, kUndefined = mfr::kRowUndefined, kImproper = mfr::kRowImproper;
constexpr int32_t kNone = -1;                         // a source: e >= 0 the stored message of slot e, e <= -2 the β of T entry -2 - e
constexpr int32_t kNever = INT_MAX;                   // a T entry that no datum reaches

__device__ __forceinline__ const double *record_of(int e, const double *f2v, const double *beta, const double *zero, int km) {
    if (e >= 0) return f2v + (int64_t)e * km;
    return (e == kNone || !beta) ? zero : beta + (int64_t)(-2 - e) * km;      // (beta null: β^(0), flat)
}

// pre[w] = the sum of the sources srcs[rec[2 w] .. + rec[2 w + 1]), in that order
template <int NT>
__global__ __launch_bounds__(64) void k_cmm_presum(int n, const int32_t *__restrict__ rec, const int32_t *__restrict__ srcs, const double *__restrict__ f2v,
                                                   const double *__restrict__ beta, const double *__restrict__ zero, double *__restrict__ pre) {
    constexpr int KD = 16 * NT, KM = KD + KD * KD;
    const int w = blockIdx.x;
    if (w >= n) return;
    const int off = rec[2 * w], m = rec[2 * w + 1];
    double *dst = pre + (int64_t)w * KM;
    for (int k = threadIdx.x; k < KM; k += 64) {
        double s = 0.0;
        for (int i = 0; i < m; i++) s += record_of(srcs[off + i], f2v, beta, zero, KM)[k];
        dst[k] = s;
    }
}

// T entry t (8 int32): {rule-table index of the sending slot, distance to the nearest datum downstream, three sources, index into pre
// (-1: the three sources are all there are), 0, 0}.  ptab, btab: as k_rule64w reads them.  next[t] = β_t^(step)
template <int NT, int WAVES_PER_SIMD>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES_PER_SIMD, WAVES_PER_SIMD)))
void k_cmm_back(int nt, int step, const int32_t *__restrict__ trec, const double *__restrict__ ptab, const double *__restrict__ btab,
                const double *__restrict__ zero, const double *__restrict__ f2v, const double *__restrict__ pre, const double *__restrict__ prev,
                double *__restrict__ next) {
    constexpr int KD = 16 * NT, KM = KD + KD * KD;
    __shared__ double S[16 * kLdT];
    __shared__ double Vs[NT][16 * kLdT];
    __shared__ double ZS[KD];
    const int t = blockIdx.x;
    if (t >= nt) return;
    const int lane = threadIdx.x, g = lane >> 4, c = lane & 15;
    const int32_t *r = trec + 8 * (int64_t)t;
    const int tabi = r[0], dist = r[1], e0 = r[2], e1 = r[3], e2 = r[4], pi = r[5];
    double *dst = next + (int64_t)t * KM;
    if (step < dist) {      // no datum within reach: flat, exactly
        for (int k = lane; k < KM; k += 64) dst[k] = 0.0;
        return;
    }
    const double *tab = ptab + (int64_t)tabi * 3 * KD * KD;
    const double *bt = btab + (int64_t)tabi * KD * KD;
    const double *src0 = pi >= 0 ? pre + (int64_t)pi * KM : record_of(e0, f2v, prev, zero, KM);
    const double *src1 = pi >= 0 ? zero : record_of(e1, f2v, prev, zero, KM);
    const bool has2 = pi < 0 && e2 != kNone;
    const double *src2 = has2 ? record_of(e2, f2v, prev, zero, KM) : zero;
    // z waits in LDS across the matrix solve.  4 x 4 tiles: the same body on buffer descriptors with its operand loads in chunks
    // (rule64b_apply, the form of the chain walks) — on plain pointers hipcc spills the lane's number, 8 bytes of scratch per lane, at
    // two waves per SIMD, whatever stands around the call
    bool ok;
    if constexpr (NT == 4)
        ok = rule64b_apply<false, true>((gcdp)tab, (gcdp)bt, (gcdp)(tab + 2 * KD * KD), nullptr, nullptr, (gcdp)src0, (gcdp)src1, (gcdp)src2, has2, (gdp)dst, S, Vs,
                                        lane, g, c, ZS);
    else
        ok = rule64w_apply<false, true, NT>((gcdp)tab, (gcdp)bt, (gcdp)(tab + 2 * KD * KD), nullptr, nullptr, (gcdp)src0, (gcdp)src1, (gcdp)src2, has2, (gdp)dst, S,
                                            Vs, lane, g, c, ZS);
    if (!ok) {
        // (the lane's number anew: the rule leaves no register free at two and four waves per SIMD, and one held across it is spilled)
        const int l2 = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        const double nan = __builtin_nan("");
        for (int k = l2; k < KM; k += 64) dst[k] = nan;
    }
}

// row record (8 int32): {1 observed / 0 not, the slot of the datum (-1: an observed variable without a connection), kept offset, kept
// count, all offset, all count, 0, 0}; kept: a run of sources in `srcs`, all: the run of every message slot into the variable.  One
// wave per row, rows [row0, row0 + n); out: n rows of u + u² doubles (row row0 first)
template <int NT, int WAVES_PER_SIMD>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES_PER_SIMD, WAVES_PER_SIMD)))
void k_cmm_rows(int row0, int n, const int32_t *__restrict__ rec, const int32_t *__restrict__ srcs, const double *__restrict__ f2v,
                const double *__restrict__ v2f, const double *__restrict__ beta, const double *__restrict__ zero, const int u, const double k_flat,
                uint8_t *__restrict__ rflag, double *__restrict__ out) {
    constexpr int KD = 16 * NT, KM = KD + KD * KD, NU = NT * (NT + 1) / 2;
    __shared__ double S[16 * kLdT];
    __shared__ double Vs[NT][16 * kLdT];
    __shared__ double ZS[KD];
    if ((int)blockIdx.x >= n) return;
    const int w = row0 + (int)blockIdx.x;
    const int lane = threadIdx.x, g = lane >> 4, c = lane & 15, mo = g * KD + c;
    const int32_t *t = rec + 8 * (int64_t)w;
    const int observed = t[0], yslot = t[1], k_off = t[2], k_n = t[3], a_off = t[4], a_n = t[5];
    double *o = out + (int64_t)blockIdx.x * (u + u * u);
    const double nan = __builtin_nan("");

    // every store of the covariance: the same lane writes the same address whether it carries a value, zero or NaN
    auto put_s = [&](int a, int b, int r, double v) {
        const int row = 16 * a + g + 4 * r, col = 16 * b + c;
        if (row < u && col < u) o[u + row * u + col] = v;
    };
    auto put_m = [&](int j, double v) {
        if (g == 0 && 16 * j + c < u) o[16 * j + c] = v;
    };
    auto fill = [&](double v) {
#pragma unroll
        for (int a = 0; a < NT; a++)
#pragma unroll
            for (int b = 0; b < NT; b++)
#pragma unroll
                for (int r = 0; r < 4; r++) put_s(a, b, r, v);
    };
    auto unscored = [&](int status) {
#pragma unroll
        for (int j = 0; j < NT; j++) put_m(j, nan);
        fill(nan);
        if (lane == 0) rflag[w] = (uint8_t)status;
    };

    if (observed) {      // its datum and a zero covariance
        if (yslot < 0) { unscored(kUndefined); return; }
#pragma unroll
        for (int j = 0; j < NT; j++) put_m(j, v2f[(int64_t)yslot * KM + 16 * j + c]);
        fill(0.0);
        if (lane == 0) rflag[w] = (uint8_t)kFinite;
        return;
    }

    // ---- the sum of the kept records in ascending neighbour order; what is undefined ------------------------------------------------
    d4 M[NU];
    double wcv[NT];
#pragma unroll
    for (int i = 0; i < NU; i++) M[i] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < NT; j++) wcv[j] = 0.0;
    add_records<NT>(M, wcv, k_n, [&](int s) { return record_of(srcs[k_off + s], f2v, beta, zero, KM); }, mo, c);
    bool undef = __builtin_isnan(bcast(M[0][0], 0)) || __builtin_isnan(bcast(wcv[0], 0));      // (whole messages are NaN together)
    pad_identity<NT>(M, g, c, u);
    undef = any_nan_record<NT>(undef, f2v, srcs + a_off, a_n);
    if (undef) { unscored(kUndefined); return; }
    if (k_n == 0) { unscored(kImproper); return; }      // nothing is kept: flat by structure

    // ---- Λ = U'U, z = U^-T η; the flat-pivot rule off the tile diagonals of V = U^-1 (k_prm_rows) -----------------------------------
    double zrv[NT][4], ld, q;
    bool pd;
    factor_solve<NT>(M, wcv, zrv, S, Vs, g, c, u, ld, q, pd);
    if (!pd || __ballot(flat_pivot<NT>(Vs, f2v, srcs + a_off, a_n, c, u, k_flat)) != 0) { unscored(kImproper); return; }
    park_z<NT>(ZS, zrv, g);

    // ---- Z = U^-T: the identity through the forward substitution; Z is lower block triangular, tiles (j, b), j >= b ------------------------
    d4 Y[NT][NT];
    solve_identity_cols<NT>(Y, M, Vs, g, c);
    // ---- cov = Z'Z, mean = Z'z: the upper tiles as they are, the lower ones turned through LDS, a diagonal tile the mean of its two
    //      triangles, so that the covariance is symmetric to the last bit ---------------------------------------------------------------
#pragma unroll
    for (int a = 0; a < NT; a++) {
#pragma unroll
        for (int b = a; b < NT; b++) {
            d4 D = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int j = b; j < NT; j++) D = tts(Y[a][j], Y[b][j], D);      // (Z'Z over the block triangle: its own loop, not gram_pass)
            store_symmetric(D, a, b, S, put_s, g, c);
        }
        double p = 0.0;
#pragma unroll
        for (int j = a; j < NT; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) p += Y[a][j][r] * ZS[16 * j + g + 4 * r];
        put_m(a, sum_groups(p));
    }
    if (lane == 0) rflag[w] = (uint8_t)kFinite;
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
// The rows follow the mode, whether there is a lag, the caller's ids, the graph and WHICH variables are observed (vinfo_epoch:
// cx_derived.h); the T entries the graph and the observed flags.  Rule tables, messages and data are read by every call
struct Plan {
    mfr::RequestKey key;      // tag: 2 mode + (a lag or none)
    uint64_t vinfo_epoch = 0;
    int64_t n_rows = 0, n_t = 0, n_pre = 0;
    DevBuf<int32_t> d_rec, d_srcs, d_trec, d_prec, d_psrcs;
    DevBuf<double> d_beta[2], d_pre, d_rows;
    DevBuf<uint8_t> d_rflag;
    DevBuf<ev::Part> d_part;
    mfr::Totals totals;
};

// the variable indices of the rows: the caller's, in the caller's order, or every variable in ascending id
static int32_t list_rows(cx_handle *h, const std::string &who, int64_t n, const int64_t *ids, std::vector<int32_t> &var) {
    using namespace cxh;
    var.clear();
    if (!ids) {
        for (int64_t v = 0; v < h->nv; v++) var.push_back((int32_t)v);
        return CX_OK;
    }
    for (int64_t i = 0; i < n; i++) {
        const int64_t v = find_var(h, ids[i]);
        if (v < 0) return fail(h, CX_ERR_NOT_FOUND, who + ": no variable " + std::to_string(ids[i]));
        var.push_back((int32_t)v);
    }
    return CX_OK;
}

static int32_t build_plan(cx_handle *h, const mfr::Pairs &P, Plan &L, int32_t mode, bool lagged, const std::vector<int32_t> &var, const std::string &who) {
    using namespace cxh;
    constexpr uint8_t kU = 0, kO = 1, kT = 2;
    const int64_t n = (int64_t)var.size(), km = (int64_t)h->cfg.dim * (h->cfg.dim + 1);
    auto obs = [&](int32_t v) { return (h->vinfo[(size_t)v] & kClamped) != 0; };
    // the class of every slot into a non-observed variable; the T entries in the order of the variable they gather from (the OUT end)
    std::vector<uint8_t> cls((size_t)std::max<int64_t>(h->nslots, 1), kU);
    struct Entry { int32_t si, so, vo, vi; };
    std::vector<Entry> ent;
    for (int64_t f = 0; f < h->nf; f++) {
        if (P.so[f] < 0 || obs(P.vi[f])) continue;
        cls[(size_t)P.si[f]] = obs(P.vo[f]) ? kO : kT;
        if (lagged && !obs(P.vo[f])) ent.push_back({P.si[f], P.so[f], P.vo[f], P.vi[f]});
    }
    std::stable_sort(ent.begin(), ent.end(), [](const Entry &a, const Entry &b) { return a.vo < b.vo; });
    const int64_t nt = (int64_t)ent.size();
    CX_REQUIRE(h, nt < (int64_t)0x7fffff00, CX_ERR_UNSUPPORTED, who + ": more than 2^31 transitions");
    std::vector<int32_t> tidx((size_t)std::max<int64_t>(h->nslots, 1), -1);
    for (int64_t t = 0; t < nt; t++) tidx[(size_t)ent[(size_t)t].si] = (int32_t)t;
    // the sources of the rule towards i through an entry whose OUT end is j: j's O slots and T entries, in ascending neighbour order
    auto sources_of = [&](int32_t j, std::vector<int32_t> &out) {
        out.clear();
        for (int32_t e = h->var_off[j]; e < h->var_off[j + 1]; e++) {
            const int32_t s = slot_of_edge(h, e);
            if (cls[(size_t)s] == kO) out.push_back(s);
            else if (cls[(size_t)s] == kT) out.push_back(-2 - tidx[(size_t)s]);
        }
    };
    // the distance of an entry to the nearest datum downstream: 1 when its OUT end has a datum of its own, otherwise one more than the
    // least distance of the OUT end's entries (breadth first from the data, against the direction of the transitions)
    std::vector<int32_t> dist((size_t)nt, kNever), first_of((size_t)h->nv + 1, 0), queue;
    for (int64_t t = 0; t < nt; t++) first_of[(size_t)ent[(size_t)t].vo + 1]++;
    for (int64_t v = 0; v < h->nv; v++) first_of[(size_t)v + 1] += first_of[(size_t)v];      // entries [first_of[j], first_of[j + 1]) have OUT end j
    std::vector<int32_t> trec((size_t)nt * 8, 0), prec, psrcs, src;
    for (int64_t t = 0; t < nt; t++) {
        const int32_t j = ent[(size_t)t].vo;
        int32_t *r = &trec[(size_t)t * 8];
        r[0] = h->spdir[(size_t)ent[(size_t)t].so];
        r[2] = r[3] = r[4] = kNone; r[5] = -1;
        if (t > first_of[(size_t)j]) {      // (a second entry out of the same variable: the same sources)
            const int32_t *r0 = &trec[(size_t)first_of[(size_t)j] * 8];
            for (int k = 2; k < 6; k++) r[k] = r0[k];
            if (dist[(size_t)first_of[(size_t)j]] == 1) { dist[(size_t)t] = 1; queue.push_back((int32_t)t); }
            continue;
        }
        sources_of(j, src);
        if (src.size() <= 3) for (size_t k = 0; k < src.size(); k++) r[2 + k] = src[k];
        else {
            r[5] = (int32_t)(prec.size() / 2);
            prec.push_back((int32_t)psrcs.size()); prec.push_back((int32_t)src.size());
            psrcs.insert(psrcs.end(), src.begin(), src.end());
            CX_REQUIRE(h, (int64_t)psrcs.size() < (int64_t)0x7fffff00, CX_ERR_UNSUPPORTED, who + ": more than 2^31 inputs");
        }
        if (std::any_of(src.begin(), src.end(), [](int32_t e) { return e >= 0; })) { dist[(size_t)t] = 1; queue.push_back((int32_t)t); }
    }
    for (size_t q = 0; q < queue.size(); q++) {
        const int32_t a1 = queue[q], i1 = ent[(size_t)a1].vi;
        for (int32_t a = first_of[(size_t)i1]; a < first_of[(size_t)i1 + 1]; a++)
            if (dist[(size_t)a] == kNever) { dist[(size_t)a] = dist[(size_t)a1] + 1; queue.push_back(a); }
    }
    for (int64_t t = 0; t < nt; t++) trec[(size_t)t * 8 + 1] = dist[(size_t)t];
    // the rows
    std::vector<int32_t> rec((size_t)n * 8, 0), srcs;
    for (int64_t i = 0; i < n; i++) {
        const int32_t x = var[(size_t)i];
        int32_t *r = &rec[(size_t)i * 8];
        if (obs(x)) {
            r[0] = 1;
            r[1] = h->var_off[x] < h->var_off[x + 1] ? slot_of_edge(h, h->var_off[x]) : -1;
            continue;
        }
        r[2] = (int32_t)srcs.size();
        for (int32_t e = h->var_off[x]; e < h->var_off[x + 1]; e++) {
            const int32_t s = slot_of_edge(h, e);
            const uint8_t c = cls[(size_t)s];
            if (c == kU || (c == kO && mode == CX_CAUSAL_FILTERED)) srcs.push_back(s);
            else if (c == kT && lagged) srcs.push_back(-2 - tidx[(size_t)s]);
        }
        r[3] = (int32_t)srcs.size() - r[2];
        const mfr::Run all = mfr::other_slots(h, x, -1, srcs);
        r[4] = all.off; r[5] = all.n;
        CX_REQUIRE(h, (int64_t)srcs.size() < (int64_t)0x7fffff00, CX_ERR_UNSUPPORTED, who + ": more than 2^31 inputs");
    }
    CX_REQUIRE(h, n < (int64_t)0x7fffff00, CX_ERR_UNSUPPORTED, who + ": more than 2^31 rows");
    L.n_rows = n;
    L.n_t = nt;
    L.n_pre = (int64_t)prec.size() / 2;
    if (srcs.empty()) srcs.push_back(0);      // (never read: no row names a source)
    int32_t rc;
    if ((rc = dev_upload(h, &L.d_rec, rec)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &L.d_srcs, srcs)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &L.d_trec, trec)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &L.d_prec, prec)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &L.d_psrcs, psrcs)) != CX_OK) return rc;
    if ((rc = L.d_pre.ensure(h, L.n_pre * km)) != CX_OK) return rc;
    if ((rc = dev_alloc(h, &L.d_rflag, std::max<int64_t>(n, 1))) != CX_OK) return rc;
    if ((rc = dev_alloc(h, &L.d_part, std::max<int64_t>((n + mfr::kTB - 1) / mfr::kTB, 1))) != CX_OK) return rc;
    CX_HIP(h, hipStreamSynchronize(h->stream));      // (the local host vectors die here)
    return CX_OK;
}

// the L launches of the backward pass; returns the buffer that holds β^(lag) (null: lag 0, or no T entry)
static const double *launch_back(cx_handle *h, Plan &L, int32_t lag) {
    const double *beta = nullptr;
    if (!L.n_t) return beta;
    const double *f2v = h->d_mv_f2v, *zero = h->d_zero_msg;
    for (int32_t s = 1; s <= lag; s++) {
        double *next = L.d_beta[(s - 1) & 1];
        mfr::for_tiles(h->cfg.dim, [&](auto tiles) {
            // waves per SIMD: k_rule64w's, whose body this is (the register counts)
            constexpr int NT = decltype(tiles)::value, W = NT == 4 ? 2 : 4;
            if (L.n_pre)
                hipLaunchKernelGGL((k_cmm_presum<NT>), dim3((unsigned)L.n_pre), dim3(64), 0, h->stream, (int)L.n_pre, L.d_prec, L.d_psrcs, f2v, beta, zero, L.d_pre);
            hipLaunchKernelGGL((k_cmm_back<NT, W>), dim3((unsigned)L.n_t), dim3(64), 0, h->stream, (int)L.n_t, (int)s, L.d_trec, h->d_ptab, h->d_ptab_bt, zero,
                               f2v, L.d_pre, beta, next);
        });
        beta = next;
    }
    return beta;
}

// rows [row0, row0 + n) into d_rows
static void launch_rows(cx_handle *h, Plan &L, int64_t row0, int64_t n, const double *beta, double *d_rows) {
    if (!n) return;
    const int u = mfr::user_dim(h);
    const double k_flat = mfr::flat_pivot_factor(h);
    mfr::for_tiles(h->cfg.dim, [&](auto nt) {
        // waves per SIMD as the register counts allow; the launch bound makes hipcc keep to them without scratch
        constexpr int NT = decltype(nt)::value, W = NT == 1 ? 4 : NT == 2 ? 3 : 2;
        hipLaunchKernelGGL((k_cmm_rows<NT, W>), dim3((unsigned)n), dim3(64), 0, h->stream, (int)row0, (int)n, L.d_rec, L.d_srcs, h->d_mv_f2v, h->d_mv_v2f,
                           beta, h->d_zero_msg, u, k_flat, L.d_rflag, d_rows);
    });
}

}  // namespace cmm

template <> void Deleter<cmm::Plan>::operator()(cmm::Plan *P) const { delete P; }

}  // namespace cx

using namespace cxh;

extern "C" int32_t cx_causal_marginals_mfma(cx_handle *h, int32_t mode, int32_t lag, int64_t n, const int64_t *variable_ids, double *out, int64_t *counts4) {
    try {
        namespace cmm = cx::cmm;
        namespace mfr = cx::mfr;
        const std::string who = "cx_causal_marginals_mfma";
        int32_t rc;
        const char *bad = !out || !counts4 ? "null argument"
                          : mode != CX_CAUSAL_PREDICTED && mode != CX_CAUSAL_FILTERED ? "mode is CX_CAUSAL_PREDICTED or CX_CAUSAL_FILTERED"
                          : lag < 0 ? "negative lag"
                          : lag > 0 && mode == CX_CAUSAL_PREDICTED ? "a lag goes with CX_CAUSAL_FILTERED"
                          : variable_ids && n < 0 ? "negative count" : nullptr;
        if ((rc = mfr::prepare(h, who, bad, {"cx_causal_marginals", "the variational and Beta-Bernoulli families have no Gaussian marginals of this kind", "rows"})) != CX_OK)
            return rc;
        if ((rc = mv_ensure_chain_msgs(h)) != CX_OK) return rc;      // (every reader of d_mv_f2v calls this first)
        if (!h->causal_mfma) h->causal_mfma.reset(new cmm::Plan());
        cmm::Plan &L = *h->causal_mfma;
        // other variables are observed: the lists are built again, the β and row buffers stay (a user who clamps a state between two
        // calls does not pay for gigabytes freed and allocated anew)
        if (L.vinfo_epoch != h->vinfo_epoch) L.key.valid = false;
        const int64_t tag = 2 * (int64_t)mode + (lag > 0);
        if (!L.key.matches(tag, n, variable_ids)) {
            L.key.valid = false;
            mfr::Pairs P;
            // (a guard: cx_graph_create lets nothing but two-variable CX_FACTOR_GAUSS_LINEAR factors and opaque ones into a handle of
            // these dims, so no graph built through the API reaches this refusal)
            if ((rc = mfr::checked_pairs(h, who, P)) != CX_OK) return rc;
            std::vector<int32_t> var;
            if ((rc = cmm::list_rows(h, who, n, variable_ids, var)) != CX_OK) return rc;
            if ((rc = cmm::build_plan(h, P, L, mode, lag > 0, var, who)) != CX_OK) return rc;
            L.key.remember(tag, n, variable_ids);
            L.vinfo_epoch = h->vinfo_epoch;
        }
        const int u = mfr::user_dim(h);
        const int64_t km = (int64_t)h->cfg.dim * (h->cfg.dim + 1);
        // β: allocated by the first call with a lag, one buffer for lag 1 and two beyond
        if (lag > 0 && L.n_t)
            for (int k = 0; k < std::min<int32_t>(lag, 2); k++) if ((rc = L.d_beta[k].ensure(h, L.n_t * km)) != CX_OK) return rc;
        const double *beta = cmm::launch_back(h, L, lag);
        CX_HIP(h, hipGetLastError());
        // the payload a chunk at a time through a bounded device buffer; the status array covers every row
        if ((rc = mfr::stream_rows(h, L.n_rows, (int64_t)u + (int64_t)u * u, L.d_rows, out,
                                   [&](int64_t r0, int64_t m, double *d) { cmm::launch_rows(h, L, r0, m, beta, d); })) != CX_OK)
            return rc;
        double none;
        return L.totals.read_rows(h, L.n_rows, nullptr, L.d_rflag, L.d_part, counts4, &none);
    } catch (const std::bad_alloc &) { return fail(h, CX_ERR_OUT_OF_MEMORY, "cx_causal_marginals_mfma: host allocation failed"); }
}
