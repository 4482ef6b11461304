// cx_sweep_deep.hip — K = 3 or 4 fused sweeps per launch on a 4-neighbour grid: the pipeline of cx_sweep_pair.hip with K levels instead of two
// (the geometry: cx_lattice_deep.h).
//
// A wave owns 64 - 2 (K - 1) columns, with K - 1 halo lanes on each side, and streams down rows r0 - (K - 1) .. r1 + (K - 1) - 1 of its segment.
// In the iteration of row i, level 1 works on row i as loaded, level j on row i - (j - 1), and level K stores row i - (K - 1) into the OTHER
// buffer at the partner slots.  Level j of a row takes the unary message, the left / right inputs that level j - 1 of the same row pushed one
// lane sideways (a wave shuffle; kept for one iteration), the up input that level j - 1 of the row above sent down (kept for two) and the
// down input that level j - 1 of the row below sends up in this very iteration.  What a row needs at every level — the unary message, the q
// of its right and its lower factor, its first slot — is carried in registers from the one time it is loaded (K + 1 rows of them; loading
// them again at level K was not tried: with them K = 4 still fits three waves per SIMD).  No LDS, no barrier, no atomics, no wait on another
// workgroup; every global access is a unit-stride run of 16 B per lane.
//
// Bit-identity with K plain sweeps.  Every level is the pair kernel's: the same leave_one_out over the fixed order unary, left, right, up,
// down with +0 for an absent direction, the same factor_rule<kRuleAdditive>(., q, 1.0, 0.0), q of a factor read at one of its two slots.
// The argument in the header of cx_sweep_pair.hip therefore holds level by level, at the cells valid at that level (cx_lattice_deep.h);
// the others hold garbage, which reaches no valid cell, is not tested for an undefined message and is not stored.
//
// Undefined messages: as in the pair kernel.  Every level tests the variable→factor messages of its valid cells and raises the same word.

#include "cx_scalar_core.h"
#include "cx_lattice_deep.h"

namespace cx {

namespace {

// (the small helpers of cx_sweep_pair.hip, repeated: that file and cx_kernels.hip stay as they are — build.py: KERNEL_SOURCES)
typedef double dd2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double2 deep_load_stream(const double2 *p) {
    const dd2v v = __builtin_nontemporal_load((const dd2v *)p);
    return make_double2(v.x, v.y);
}
__device__ __forceinline__ int deep_slab(int b, int nb) {
    const int xcd = b & 7, q = nb >> 3, r = nb & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
}
__device__ __forceinline__ double2 dsel2(bool c, double2 a, double2 b) { return make_double2(c ? a.x : b.x, c ? a.y : b.y); }
__device__ __forceinline__ double2 dshfl_up2(double2 a) { return make_double2(__shfl_up(a.x, 1, 64), __shfl_up(a.y, 1, 64)); }
__device__ __forceinline__ double2 dshfl_down2(double2 a) { return make_double2(__shfl_down(a.x, 1, 64), __shfl_down(a.y, 1, 64)); }

// k_sweep's leave-one-out sums over five inputs: out[k] = (in[0] + .. + in[k-1]) + (in[4] + .. + in[k+1])
__device__ __forceinline__ void deep_leave_one_out(const double2 (&in)[5], double2 (&out)[5]) {
    double2 acc = zero2();
#pragma unroll
    for (int k = 0; k < 5; k++) { out[k] = acc; acc = add2(acc, in[k]); }
    acc = zero2();
#pragma unroll
    for (int k = 4; k >= 0; k--) { out[k] = add2(out[k], acc); acc = add2(acc, in[k]); }
}

struct DeepRow {          // one grid row as loaded: the five ranks, the q of the right and the lower factor, the lane's first slot
    double2 x[5];
    double qR, qD;
    int base;
};
struct DeepOut {          // what a level of one row sends to the next level: to the row itself (sideways), to the row above, to the row below
    double2 L, R, up, down;
};
struct DeepPending {      // the inputs of a level that wait for their row's turn: left / right (one iteration), up (two: carry, then U)
    double2 L, R, U, carry;
};

// the variable→factor messages o of one row at a level below K, through the factors: left / right by the sender's right factor and the
// receiver's own (one q per factor), up through the factor above (q came with the row above), down through the row's lower factor
__device__ __forceinline__ DeepOut deep_emit(const double2 (&o)[5], bool hasL, bool hasR, double qR, double qU, double qD) {
    DeepOut e;
    const double2 to_right = factor_rule<kRuleAdditive>(o[2], qR, 1.0, 0.0);
    const double2 from_left = dshfl_up2(to_right);
    const double2 from_right = factor_rule<kRuleAdditive>(dshfl_down2(o[1]), qR, 1.0, 0.0);
    e.L = dsel2(hasL, from_left, zero2());
    e.R = dsel2(hasR, from_right, zero2());
    e.up = factor_rule<kRuleAdditive>(o[3], qU, 1.0, 0.0);
    e.down = factor_rule<kRuleAdditive>(o[4], qD, 1.0, 0.0);
    return e;
}

__device__ __forceinline__ bool deep_undefined(const double2 (&o)[5], bool hasL, bool hasR, bool hasU, bool hasD) {
    return (hasL && __builtin_isnan(o[1].y)) || (hasR && __builtin_isnan(o[2].y)) || (hasU && __builtin_isnan(o[3].y)) || (hasD && __builtin_isnan(o[4].y));
}

}  // namespace

// grid = block_cols * nseg workgroups; wave w of workgroup (bc, seg) owns strip 4 bc + w, rows [seg R, seg R + R)
template <int K>
__global__ __launch_bounds__(kBlock) void k_sweep_deep(int H, int W, int R, int nseg, const int32_t *__restrict__ slice_off, const double *__restrict__ q,
                                                       const double2 *__restrict__ f2v_in, double2 *__restrict__ f2v_out, unsigned *__restrict__ abort_word) {
    namespace dp = lattice::deep;
    const int s = deep_slab(blockIdx.x, gridDim.x);
    const int bc = s / nseg, seg = s - bc * nseg;       // consecutive segments of one column of workgroups share an XCD (their halo rows meet in its L2)
    const int strip = bc * lattice::kStripsPerBlock + (threadIdx.x >> 6);
    if (strip * dp::strip_cols(K) >= W) return;         // (wave-uniform: the last workgroup column may hold fewer than four strips)
    const int lane = threadIdx.x & 63;
    const int c = dp::lane_col(strip, lane, K);
    const bool colv = c >= 0 && c < W;
    const bool hasL = colv && c > 0, hasR = colv && c < W - 1;
    const bool own = dp::lane_owned(lane, c, W, K) && colv;
    const bool two = hasL && hasR;                      // left AND right: up / down sit one rank higher
    const int r0 = seg * R, r1 = min(r0 + R, H);
    bool bad = false;

    // rows outside the grid and lanes outside the row load nothing: zeros, q = 1 (their results are never used).  The lane's first slot of
    // a row comes from slice_off one row earlier than the row's messages are asked for: no dependent load in front of them
    auto load_base = [&](int r) { return (r >= 0 && r < H && colv) ? lattice::slot_base(slice_off, r * W + c) : 0; };
    auto load_row = [&](int r, int base) {
        DeepRow in;
#pragma unroll
        for (int k = 0; k < 5; k++) in.x[k] = zero2();
        in.qR = 1.0; in.qD = 1.0; in.base = base;
        if (r >= 0 && r < H && colv) {
            const int deg = lattice::degree(r, c, H, W);
#pragma unroll
            for (int k = 0; k < 5; k++)
                if (k < deg) in.x[k] = deep_load_stream(&f2v_in[in.base + k * kBlock]);
            if (hasR) in.qR = q[in.base + lattice::rank_right(c) * kBlock];
            if (r < H - 1) in.qD = q[in.base + lattice::rank_down(r, c, W) * kBlock];
        }
        return in;
    };

    // by age a: row i - a of the iteration of row i.  Age 0 is the row at level 1; level j works on age j - 1; level K stores into the rows
    // of ages K - 2 (below), K - 1 (sideways) and K (above)
    double2 P[K];
    double qR[K], qD[K + 1];
    int base[K + 1];
#pragma unroll
    for (int a = 0; a < K; a++) { P[a] = zero2(); qR[a] = 1.0; }
#pragma unroll
    for (int a = 0; a <= K; a++) { qD[a] = 1.0; base[a] = 0; }
    DeepPending pend[K + 1];          // (indexed by level: 2 .. K)
#pragma unroll
    for (int j = 0; j <= K; j++) { pend[j].L = zero2(); pend[j].R = zero2(); pend[j].U = zero2(); pend[j].carry = zero2(); }

    const int i0 = r0 - (K - 1), i1 = r1 + (K - 1) - 1;      // rows loaded: level K reaches row r1 - 1 in the iteration of row i1
    DeepRow cur = load_row(i0, load_base(i0));
    int base_next = load_base(i0 + 1);
    for (int i = i0; i <= i1; i++) {
        DeepRow nxt = cur;
        if (i < i1) nxt = load_row(i + 1, base_next);        // (uniform) the next row's loads are in flight while this one is worked on
        if (i + 1 < i1) base_next = load_base(i + 2);
        P[0] = cur.x[0]; qR[0] = cur.qR; qD[0] = cur.qD; base[0] = cur.base;
        DeepOut e;
        e.L = zero2(); e.R = zero2(); e.up = zero2(); e.down = zero2();
        if (i >= 0 && i < H) {                               // (uniform) level 1 of row i
            const bool hasU = i > 0, hasD = i < H - 1;
            double2 in[5], o[5];
            const double2 xu = two ? cur.x[3] : cur.x[2];
            const double2 xd = hasU ? (two ? cur.x[4] : cur.x[3]) : xu;
            in[0] = cur.x[0];
            in[1] = dsel2(hasL, cur.x[1], zero2());
            in[2] = dsel2(hasR, hasL ? cur.x[2] : cur.x[1], zero2());
            in[3] = dsel2(hasU && colv, xu, zero2());
            in[4] = dsel2(hasD && colv, xd, zero2());
            deep_leave_one_out(in, o);
            bad = bad || deep_undefined(o, hasL, hasR, colv && hasU, colv && hasD);
            e = deep_emit(o, hasL, hasR, cur.qR, qD[1], cur.qD);
        }
#pragma unroll
        for (int j = 2; j <= K; j++) {
            const int m = i - (j - 1);                       // level j's row: its inputs are complete now
            DeepOut f;
            f.L = zero2(); f.R = zero2(); f.up = zero2(); f.down = zero2();
            int baseL = 0, baseR = 0;
            double qL = 1.0;
            if (j == K) {                                    // (by every lane: the stores below are the owned lanes' alone)
                baseL = __shfl_up(base[K - 1], 1, 64); baseR = __shfl_down(base[K - 1], 1, 64);
                qL = __shfl_up(qR[K - 1], 1, 64);
            }
            if (dp::row_valid_at_level(m, r0, r1, H, K, j)) {      // (uniform)
                const bool mU = m > 0, mD = m < H - 1;
                double2 in[5], o[5];
                in[0] = P[j - 1]; in[1] = pend[j].L; in[2] = pend[j].R;
                in[3] = dsel2(mU, pend[j].U, zero2());
                in[4] = dsel2(mD, e.up, zero2());
                deep_leave_one_out(in, o);
                if (dp::lane_valid_at_level(lane, c, W, j)) bad = bad || deep_undefined(o, hasL, hasR, mU, mD);
                if (j < K) f = deep_emit(o, hasL, hasR, qR[j - 1], qD[j], qD[j - 1]);
                else if (own) {                              // level K of an owned row (row_valid_at_level at j = K: r0 <= m < r1): stored
                    if (hasL) f2v_out[baseL + lattice::rank_right(c - 1) * kBlock] = factor_rule<kRuleAdditive>(o[1], qL, 1.0, 0.0);
                    if (hasR) f2v_out[baseR + lattice::rank_left() * kBlock] = factor_rule<kRuleAdditive>(o[2], qR[K - 1], 1.0, 0.0);
                    if (mU) f2v_out[base[K] + lattice::rank_down(m - 1, c, W) * kBlock] = factor_rule<kRuleAdditive>(o[3], qD[K], 1.0, 0.0);
                    if (mD) f2v_out[base[K - 2] + lattice::rank_up(c, W) * kBlock] = factor_rule<kRuleAdditive>(o[4], qD[K - 1], 1.0, 0.0);
                }
            }
            // what level j - 1 produced in this iteration waits for its row's turn at level j
            pend[j].L = e.L; pend[j].R = e.R; pend[j].U = pend[j].carry; pend[j].carry = e.down;
            e = f;
        }
#pragma unroll
        for (int a = K; a >= 1; a--) {
            if (a < K) { P[a] = P[a - 1]; qR[a] = qR[a - 1]; }
            qD[a] = qD[a - 1]; base[a] = base[a - 1];
        }
        cur = nxt;
    }
    if (bad) *abort_word = 1u;      // (an ordinary per-lane store)
}

template <int K>
static int64_t deep_capacity(const cx_handle *h) {
    int per_cu = 0, dev = h->cfg.device;
    hipDeviceProp_t prop;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_sweep_deep<K>, kBlock, 0) != hipSuccess || per_cu <= 0) { (void)hipGetLastError(); per_cu = 2; }
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) { (void)hipGetLastError(); return (int64_t)per_cu * 256; }
    return (int64_t)per_cu * prop.multiProcessorCount;
}

// workgroups of k_sweep_deep<depth> the device holds at once
int64_t deep_capacity_blocks(const cx_handle *h, int depth) { return depth == 3 ? deep_capacity<3>(h) : deep_capacity<4>(h); }

void launch_sweep_deep(cx_handle *h, int depth, const double2 *f2v_in, double2 *f2v_out) {
    const int R = h->deep_rows[depth], nseg = (h->pair_H + R - 1) / R;
    const dim3 grid((unsigned)(lattice::deep::block_cols(h->pair_W, depth) * nseg));
    if (depth == 3)
        hipLaunchKernelGGL(k_sweep_deep<3>, grid, dim3(kBlock), 0, h->stream, h->pair_H, h->pair_W, R, nseg, h->d_slice_off, h->d_q, f2v_in, f2v_out, h->pair_abort.dev);
    else
        hipLaunchKernelGGL(k_sweep_deep<4>, grid, dim3(kBlock), 0, h->stream, h->pair_H, h->pair_W, R, nseg, h->d_slice_off, h->d_q, f2v_in, f2v_out, h->pair_abort.dev);
}

}  // namespace cx
