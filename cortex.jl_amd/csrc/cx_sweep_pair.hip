// cx_sweep_pair.hip — two fused sweeps per launch on a 4-neighbour grid (the plan: cx_lattice_plan.h).
//
// A plain fused sweep (cx_kernels.hip: k_sweep) reads every factor→variable message once and writes every one once; two of them write
// 128 MB on the 10 M-edge grid that the second reads straight back.  Here the intermediate sweep never leaves the registers: a wave owns
// 62 columns (lanes 1 .. 62; lanes 0 and 63 are halo columns) and streams down the rows of its segment.  For each row it loads the five
// ranks of the level-t messages, forms the variable→factor messages with k_sweep's own leave-one-out sums, and pushes them through the
// factor rule into the level-t+1 inputs of the rows above, below (same lane) and of the row itself (one lane left / right, by a wave
// shuffle).  A row whose four inputs are complete is processed at level t+1 and its messages are stored into the OTHER buffer at the
// partner slots, which the plan proved to be arithmetic.  Every global access is a unit-stride run of 16 B per lane along the id order.
// No LDS, no barrier, no atomics, no wait on another workgroup.
//
// Bit-identity with two plain sweeps.  k_sweep sums a variable's messages in rank order with zeros above the degree; here the five
// inputs sit in the fixed order unary, left, right, up, down with a zero for an absent direction.  The running sums start from +0 and a
// sum in round-to-nearest is never -0 unless both terms are, so an added +0 changes no bit, in the middle of the order as little as at its
// end: the present terms meet in the same order with the same partial sums.  The rule is factor_rule<kRuleAdditive> with the same q.
//
// Undefined messages.  A plain sweep does not store an undefined (NaN) variable→factor message's result, so the slot keeps an older value;
// a pair cannot reproduce that.  The host runs pairs only when every live slot of the input is defined (k_pair_check); if a launch still
// meets a NaN variable→factor message at either level (inf - inf in a diverging model) it raises a word in mapped host memory, which
// the next checked HIP call of the host turns into an error (cx_host.h: pair_abort_take).

#include "cx_scalar_core.h"
#include "cx_lattice_plan.h"

namespace cx {

namespace {

// (as in cx_kernels.hip, whose code a committed counter profile is tied to — build.py: KERNEL_SOURCES — and therefore stays as it is)
typedef double pd2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double2 pair_load_stream(const double2 *p) {
    const pd2v v = __builtin_nontemporal_load((const pd2v *)p);
    return make_double2(v.x, v.y);
}
__device__ __forceinline__ void pair_store(double2 *p, double2 v, int nt) {
    if (nt) { pd2v t; t.x = v.x; t.y = v.y; __builtin_nontemporal_store(t, (pd2v *)p); }
    else *p = v;
}
// workgroups are dealt round-robin over the 8 XCDs: XCD x takes the x-th contiguous run of the launch's linear order (cx_kernels.hip: xcd_slab)
__device__ __forceinline__ int pair_slab(int b, int nb) {
    const int xcd = b & 7, q = nb >> 3, r = nb & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
}

__device__ __forceinline__ double2 sel2(bool c, double2 a, double2 b) { return make_double2(c ? a.x : b.x, c ? a.y : b.y); }
__device__ __forceinline__ double2 shfl_up2(double2 a) { return make_double2(__shfl_up(a.x, 1, 64), __shfl_up(a.y, 1, 64)); }
__device__ __forceinline__ double2 shfl_down2(double2 a) { return make_double2(__shfl_down(a.x, 1, 64), __shfl_down(a.y, 1, 64)); }

// k_sweep's leave-one-out sums over five inputs: out[k] = (in[0] + .. + in[k-1]) + (in[4] + .. + in[k+1])
__device__ __forceinline__ void leave_one_out(const double2 (&in)[5], double2 (&out)[5]) {
    double2 acc = zero2();
#pragma unroll
    for (int k = 0; k < 5; k++) { out[k] = acc; acc = add2(acc, in[k]); }
    acc = zero2();
#pragma unroll
    for (int k = 4; k >= 0; k--) { out[k] = add2(out[k], acc); acc = add2(acc, in[k]); }
}

struct RowIn {            // one grid row as loaded: the five ranks, the q of the right and the lower factor, the lane's first slot
    double2 x[5];
    double qR, qD;
    int base;
};

}  // namespace

// grid = block_cols * nseg workgroups; wave w of workgroup (bc, seg) owns strip 4 bc + w, rows [seg R, seg R + R)
__global__ __launch_bounds__(kBlock) void k_sweep_pair(int H, int W, int R, int nseg, const int32_t *__restrict__ slice_off,
                                                       const double *__restrict__ q, const double2 *__restrict__ f2v_in,
                                                       double2 *__restrict__ f2v_out, unsigned *__restrict__ abort_word, int nt_out) {
    const int s = pair_slab(blockIdx.x, gridDim.x);
    const int bc = s / nseg, seg = s - bc * nseg;       // consecutive segments of one column of workgroups share an XCD (their halo rows meet in its L2)
    const int strip = bc * lattice::kStripsPerBlock + (threadIdx.x >> 6);
    if (strip * lattice::kStripCols >= W) return;       // (wave-uniform: the last workgroup column may hold fewer than four strips)
    const int lane = threadIdx.x & 63;
    const int c = lattice::lane_col(strip, lane);
    const bool colv = c >= 0 && c < W;
    const bool hasL = colv && c > 0, hasR = colv && c < W - 1;
    const bool own = lattice::lane_owned(lane, c, W) && colv;
    const bool two = hasL && hasR;                      // left AND right: up / down sit one rank higher
    const int r0 = seg * R, r1 = min(r0 + R, H);
    bool bad = false;

    // rows outside the grid and lanes outside the row load nothing: zeros, q = 1 (their results are never used).  The lane's first slot of
    // a row comes from slice_off one row earlier than the row's messages are asked for: no dependent load in front of them
    auto load_base = [&](int r) { return (r >= 0 && r < H && colv) ? lattice::slot_base(slice_off, r * W + c) : 0; };
    auto load_row = [&](int r, int base) {
        RowIn in;
#pragma unroll
        for (int k = 0; k < 5; k++) in.x[k] = zero2();
        in.qR = 1.0; in.qD = 1.0; in.base = base;
        if (r >= 0 && r < H && colv) {
            const int deg = lattice::degree(r, c, H, W);
#pragma unroll
            for (int k = 0; k < 5; k++)
                if (k < deg) in.x[k] = pair_load_stream(&f2v_in[in.base + k * kBlock]);
            if (hasR) in.qR = q[in.base + lattice::rank_right(c) * kBlock];
            if (r < H - 1) in.qD = q[in.base + lattice::rank_down(r, c, W) * kBlock];
        }
        return in;
    };

    // the pending row (r - 1 while row r is at level t): its level-t+1 inputs so far, its q, its slots and those of the row above it
    double2 pP = zero2(), pL = zero2(), pR = zero2(), pU = zero2();
    double pqL = 1.0, pqR = 1.0, pqU = 1.0, pqD = 1.0;
    int pbase = 0, ppbase = 0;
    double2 carryU = zero2();         // rule(row r - 1's message down): the level-t+1 input "up" of row r

    RowIn cur = load_row(r0 - 1, load_base(r0 - 1));
    int base_next = load_base(r0);
    for (int r = r0 - 1; r <= r1; r++) {
        RowIn nxt = cur;
        if (r < r1) nxt = load_row(r + 1, base_next);    // (uniform) the next row's loads are in flight while this one is worked on
        if (r + 1 < r1) base_next = load_base(r + 2);
        const bool rowv = r >= 0 && r < H, hasU = r > 0, hasD = r < H - 1;
        double2 nP = zero2(), nL = zero2(), nR = zero2(), up_msg = zero2(), down_msg = zero2();
        double nqL = 1.0;
        if (rowv) {                                      // (uniform) level t of row r
            double2 in[5], o[5];
            const double2 xu = two ? cur.x[3] : cur.x[2];
            const double2 xd = hasU ? (two ? cur.x[4] : cur.x[3]) : xu;
            in[0] = cur.x[0];
            in[1] = sel2(hasL, cur.x[1], zero2());
            in[2] = sel2(hasR, hasL ? cur.x[2] : cur.x[1], zero2());
            in[3] = sel2(hasU && colv, xu, zero2());
            in[4] = sel2(hasD && colv, xd, zero2());
            leave_one_out(in, o);
            bad = bad || (hasL && __builtin_isnan(o[1].y)) || (hasR && __builtin_isnan(o[2].y)) || (colv && hasU && __builtin_isnan(o[3].y)) ||
                  (colv && hasD && __builtin_isnan(o[4].y));
            // left / right: the sender's lane applies the rule of its right factor, the receiver's that of ITS right factor (one q per factor)
            const double2 to_right = factor_rule<kRuleAdditive>(o[2], cur.qR, 1.0, 0.0);
            const double2 from_left = shfl_up2(to_right);
            const double2 from_right = factor_rule<kRuleAdditive>(shfl_down2(o[1]), cur.qR, 1.0, 0.0);
            nqL = __shfl_up(cur.qR, 1, 64);
            nP = cur.x[0];
            nL = sel2(hasL, from_left, zero2());
            nR = sel2(hasR, from_right, zero2());
            up_msg = factor_rule<kRuleAdditive>(o[3], pqD, 1.0, 0.0);          // through the factor above: its q came with row r - 1
            down_msg = factor_rule<kRuleAdditive>(o[4], cur.qD, 1.0, 0.0);
        }
        const int m = r - 1;                             // the pending row: complete now
        const int baseL = __shfl_up(pbase, 1, 64), baseR = __shfl_down(pbase, 1, 64);
        if (m >= r0 && m < r1) {                         // (uniform) an owned row: level t + 1, stored
            const bool mU = m > 0, mD = m < H - 1;
            double2 in[5], o[5];
            in[0] = pP; in[1] = pL; in[2] = pR;
            in[3] = sel2(mU, pU, zero2());
            in[4] = sel2(mD && rowv, up_msg, zero2());
            leave_one_out(in, o);
            if (own) {
                bad = bad || (hasL && __builtin_isnan(o[1].y)) || (hasR && __builtin_isnan(o[2].y)) || (mU && __builtin_isnan(o[3].y)) || (mD && __builtin_isnan(o[4].y));
                if (hasL) pair_store(&f2v_out[baseL + lattice::rank_right(c - 1) * kBlock], factor_rule<kRuleAdditive>(o[1], pqL, 1.0, 0.0), nt_out);
                if (hasR) pair_store(&f2v_out[baseR + lattice::rank_left() * kBlock], factor_rule<kRuleAdditive>(o[2], pqR, 1.0, 0.0), nt_out);
                if (mU) pair_store(&f2v_out[ppbase + lattice::rank_down(m - 1, c, W) * kBlock], factor_rule<kRuleAdditive>(o[3], pqU, 1.0, 0.0), nt_out);
                if (mD) pair_store(&f2v_out[cur.base + lattice::rank_up(c, W) * kBlock], factor_rule<kRuleAdditive>(o[4], pqD, 1.0, 0.0), nt_out);
            }
        }
        // row r becomes the pending row
        ppbase = pbase; pbase = cur.base;
        pqU = pqD; pqL = nqL; pqR = cur.qR; pqD = cur.qD;
        pP = nP; pL = nL; pR = nR; pU = carryU;
        carryU = down_msg;
        cur = nxt;
    }
    if (bad) *abort_word = 1u;      // (an ordinary per-lane store)
}

// every live slot of `in` defined, and the unary messages (which no sweep writes) the same in both buffers: what a pair relies on
__global__ __launch_bounds__(kBlock) void k_pair_check(int nv, const int32_t *__restrict__ slice_off, const uint8_t *__restrict__ vinfo,
                                                       const double2 *__restrict__ in, const double2 *__restrict__ alt, unsigned *__restrict__ flag) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    const int base = lattice::slot_base(slice_off, v), deg = vinfo[v] & kDegMask;
    bool bad = false;
    for (int k = 0; k < deg; k++) bad = bad || __builtin_isnan(in[base + k * kBlock].y);
    const double2 a = in[base], b = alt[base];
    bad = bad || __double_as_longlong(a.x) != __double_as_longlong(b.x) || __double_as_longlong(a.y) != __double_as_longlong(b.y);
    if (bad) *flag = 1u;
}

// workgroups of k_sweep_pair the device holds at once
int64_t pair_capacity_blocks(const cx_handle *h) {
    int per_cu = 0, dev = h->cfg.device;
    hipDeviceProp_t prop;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_sweep_pair, kBlock, 0) != hipSuccess || per_cu <= 0) { (void)hipGetLastError(); per_cu = 2; }
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) { (void)hipGetLastError(); return (int64_t)per_cu * 256; }
    return (int64_t)per_cu * prop.multiProcessorCount;
}

void launch_sweep_pair(cx_handle *h, const double2 *f2v_in, double2 *f2v_out) {
    const int R = h->pair_rows, nseg = (h->pair_H + R - 1) / R;
    // stores: plain by default, as in the plain sweep on a graph larger than the L2s (CX_PAIR_NT=1: nontemporal, A/B)
    static const int nt = [] { const char *e = std::getenv("CX_PAIR_NT"); return e && e[0] == '1' ? 1 : 0; }();
    hipLaunchKernelGGL(k_sweep_pair, dim3((unsigned)(h->pair_block_cols * nseg)), dim3(kBlock), 0, h->stream, h->pair_H, h->pair_W, R, nseg,
                       h->d_slice_off, h->d_q, f2v_in, f2v_out, h->pair_abort.dev, nt);
}

void launch_pair_check(cx_handle *h, const double2 *f2v, const double2 *alt, unsigned *d_flag) {
    hipLaunchKernelGGL(k_pair_check, dim3((unsigned)((h->nv + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream, (int)h->nv, h->d_slice_off, h->d_vinfo,
                       f2v, alt, d_flag);
}

}  // namespace cx
