// cx_sweep_deep.hip — K = 3 .. 6 fused sweeps per launch on a 4-neighbour grid: the pipeline of cx_sweep_pair.hip with K levels instead of two
// (the geometry: cx_lattice_deep.h).
//
// A wave owns 64 - 2 (K - 1) columns, with K - 1 halo lanes on each side, and streams down rows r0 - (K - 1) .. r1 + (K - 1) - 1 of its segment.
// In the iteration of row i, level 1 works on row i as loaded, level j on row i - (j - 1), and level K stores row i - (K - 1) into the OTHER
// buffer at the partner slots.  Level j of a row takes the unary message, the left / right inputs that level j - 1 of the same row pushed one
// lane sideways (a whole-wave shift; kept for one iteration), the up input that level j - 1 of the row above sent down (kept for two) and the
// down input that level j - 1 of the row below sends up in this very iteration.  What a row needs at every level — the unary message, the q
// of its right and its lower factor, its first slot — is carried in registers from the one time it is loaded (K + 1 rows of them; loading
// them again at level K was not tried: with them K = 4 still fits three waves per SIMD, K = 5 and 6 two: profiles/deep_sweep_56.md).  No LDS, no barrier, no atomics, no wait on another
// workgroup; every global access is a unit-stride run of 16 B per lane.
//
// The loop and its loads (profiles/deep_sweep_issue.md).  The loads of row i + 1 are issued at the top of the iteration of row i and are first
// needed at the top of the next one: between them lie all K levels of arithmetic, and no instruction there waits for a load.  That takes
// two things.  The slice_off word of row i + 2 is loaded behind the loads of row i + 1 and kept as loaded; the row's first slot is formed
// from it one iteration later, in front of that iteration's loads.  And the loop starts one row early, on a row of zeros, so that the first
// row is loaded where every other row is and the loop is entered with nothing in flight.  One s_waitcnt vmcnt(0) per iteration remains, where
// the loaded row is taken over; it also waits for level K's four stores of the iteration, which the in-order counter cannot tell apart.
// (Issued in every iteration outside every branch, as buffer stores with an offset beyond the buffer where nothing is to be stored, they
// make that wait a vmcnt(4) and stay in flight over it; on the card that was not faster, three waves per SIMD cover the wait already:
// profiles/deep_sweep_stores.md.)
//
// Depth and waves per SIMD (profiles/deep_sweep_56.md).  K = 3 and 4 fit three waves per SIMD, K = 5 and 6 two; the rows per segment are
// chosen so that the launch is resident at once (choose_rows_packed), 12 at K = 4 and 19 at K = 5 on the flagship grid.  A deeper launch
// moves fewer bytes per sweep for the same arithmetic per stored cell; the vector unit is busy 0.74 - 0.80 of the launch (0.66 - 0.71 while
// every rule held a branch: profiles/deep_sweep_div.md).
//
// Three instances per depth, chosen per wave (wave-uniformly; cx_lattice_deep.h: wave_class).  INTERIOR: a wave all of whose columns and rows
// have four neighbours in the grid (strip_interior, segment_interior) runs the loop with every edge test folded to true.  COLUMN-EDGE: a
// wave of an interior segment whose strip holds the grid's first or last column (both, on a grid narrower than a strip): every row it
// touches at any level lies in 1 .. H - 2, so every row test is folded to true, and what depends on the lane — whether its column lies in
// the grid and has a left and a right neighbour, the ranks of its loads, of qR / qD and of the four stores — is the same for every row and
// is formed once in front of the loop; its loads are issued without a branch like the interior loop's, each direction from its own rank.
// GENERAL: every other wave, the top and bottom segments.  757 / 721 / 929 instructions per row at K = 4, 921 / 874 / 1,114 at K = 5, with
// 16 and 20 v_rcp_f64 (profiles/deep_sweep_div.md; with a division in each branch of the rule 950 / 914 / 1,164 and 1,170 / 1,120 / 1,404
// stood in the listing, of which a wave without point masses skipped some 50 per level: profiles/deep_sweep_edges.md, deep_sweep_56.md).
// The arithmetic, its order, the rule at a point mass and the test for an undefined message are the same in all three.
//
// Waves to workgroups (cx_lattice_deep.h: packed_wave).  Four adjacent strips of one segment make a workgroup.  Where the last workgroup
// column has s < 4 strips, a workgroup takes floor(4 / s) consecutive segments of it instead, so that no wave slot of a resident workgroup
// stays empty: on the flagship grid at K = 4 (25 strips) that is a ninth of the slots, and it lets the launch be resident at 12 rows per
// segment instead of 13 (choose_rows_packed; profiles/deep_sweep_stores.md).  Which wave runs which (strip, segment) changes no stored bit.
//
// Bit-identity with K plain sweeps.  Every level is the pair kernel's: the same leave_one_out over the fixed order unary, left, right, up,
// down with +0 for an absent direction, the bits of factor_rule<kRuleAdditive>(., q, 1.0, 0.0), q of a factor read at one of its two slots.
// The argument in the header of cx_sweep_pair.hip therefore holds level by level, at the cells valid at that level (cx_lattice_deep.h);
// the others hold garbage, which reaches no valid cell, is not tested for an undefined message and is not stored.
// The rule is written here with ONE division (deep_rule).  factor_rule has two branches, 1 / q at a point mass (m.y == +inf) and
// 1 / (1 + q m.y) otherwise, an IEEE division in each (v_rcp_f64 and about ten f64 instructions).  The compiler kept the point-mass branch
// as a block behind s_and_saveexec / s_cbranch_execz: a wave without point masses skipped its body but paid 40 mask-and-branch pairs per
// row at K = 5, and the block boundaries kept the four division chains of a level from being interleaved; without them the launch takes
// 0.895 of its busy cycles at K = 5 for as many executed instructions (profiles/deep_sweep_div.md).  With s = 1 / den the branches differ only in den and in one factor of o.y: at a point mass
// den = q, o.y = s, o.x = m.x s, which is factor_rule's 1 / q and m.x (1 / q); otherwise den, o.y = m.y s and o.x = m.x s are factor_rule's
// own expressions, and 1 + q m.y is contracted into one fused multiply-add or not as it is there (the same source expression, the same
// compiler; the bit-for-bit tests against plain sweeps would show a difference).  NaN and -inf compare unequal to +inf and take the
// ordinary branch, as they do there.  deep_rule selects the operands instead of the results (den = a + q t with (a, t) = (-0, 1) at a point
// mass, (1, m.y) otherwise; q 1 + -0 is q for every q, -0 included), which costs three instructions per rule where selecting den and o.y
// costs four.  tests/test_deep_rule_host.py holds both forms for the host: the same bits on 1e6 random and special inputs;
// tests/test_gpu_sweep_deep_rule.py reaches the point-mass branch on the card.  profiles/deep_sweep_div.md.
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
// the value of the lane below (up) or above (down), as whole-wave DPP shifts of one dword each (v_mov_b32_dpp wave_shr:1 / wave_shl:1: no LDS
// instruction, no wait).  Lane 0 of a shift up and lane 63 of a shift down receive 0, not their own value as with __shfl_up / __shfl_down:
// those two lanes are valid at level 1 only and never owned (cx_lattice_deep.h), and what is shifted in feeds levels >= 2 and the stores, so
// nothing tested or stored depends on it
__device__ __forceinline__ int ishift_up(int x) { return __builtin_amdgcn_update_dpp(0, x, 0x138 /* wave_shr:1 */, 0xf, 0xf, false); }
__device__ __forceinline__ int ishift_down(int x) { return __builtin_amdgcn_update_dpp(0, x, 0x130 /* wave_shl:1 */, 0xf, 0xf, false); }
__device__ __forceinline__ double dshift_up(double x) { return __hiloint2double(ishift_up(__double2hiint(x)), ishift_up(__double2loint(x))); }
__device__ __forceinline__ double dshift_down(double x) { return __hiloint2double(ishift_down(__double2hiint(x)), ishift_down(__double2loint(x))); }
__device__ __forceinline__ double2 dshfl_up2(double2 a) { return make_double2(dshift_up(a.x), dshift_up(a.y)); }
__device__ __forceinline__ double2 dshfl_down2(double2 a) { return make_double2(dshift_down(a.x), dshift_down(a.y)); }

// k_sweep's leave-one-out sums over five inputs: out[k] = (in[0] + .. + in[k-1]) + (in[4] + .. + in[k+1])
__device__ __forceinline__ void deep_leave_one_out(const double2 (&in)[5], double2 (&out)[5]) {
    double2 acc = zero2();
#pragma unroll
    for (int k = 0; k < 5; k++) { out[k] = acc; acc = add2(acc, in[k]); }
    acc = zero2();
#pragma unroll
    for (int k = 4; k >= 0; k--) { out[k] = add2(out[k], acc); acc = add2(acc, in[k]); }
}

// factor_rule<kRuleAdditive>(m, q, 1.0, 0.0) with one division and no branch, the same bits (the header: bit-identity).  The rule has two
// branches, 1 / q at a point mass (m.y == +inf) and 1 / (1 + q m.y) otherwise, which the compiler kept as branches on the exec mask.  Here
// the branches differ in t, which is 1 at a point mass and m.y otherwise, and in the addend a, -0 or 1: the denominator a + q t is q
// exactly at a point mass (q 1 is q, and q + -0 is q, a q of -0 included) and the rule's own expression otherwise, contracted or not as
// the rule's is; o.y = t s is s exactly resp. m.y s.  +inf and 1.0 have the same low word, so t is m.y with one select on its high word
__device__ __forceinline__ double2 deep_rule(double2 m, double q) {
    const bool pm = m.y == __builtin_inf();
    const double t = __hiloint2double(pm ? 0x3ff00000 : __double2hiint(m.y), __double2loint(m.y));
    const double s = 1.0 / ((pm ? -0.0 : 1.0) + q * t);
    return make_double2(m.x * s, t * s);
}

struct DeepRow {          // one grid row as loaded: the five ranks (a column-edge wave: by direction), the q of the right and the lower factor, the lane's first slot
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
    const double2 to_right = deep_rule(o[2], qR);
    const double2 from_left = dshfl_up2(to_right);
    const double2 from_right = deep_rule(dshfl_down2(o[1]), qR);
    e.L = dsel2(hasL, from_left, zero2());
    e.R = dsel2(hasR, from_right, zero2());
    e.up = deep_rule(o[3], qU);
    e.down = deep_rule(o[4], qD);
    return e;
}

__device__ __forceinline__ bool deep_undefined(const double2 (&o)[5], bool hasL, bool hasR, bool hasU, bool hasD) {
    return (hasL && __builtin_isnan(o[1].y)) || (hasR && __builtin_isnan(o[2].y)) || (hasU && __builtin_isnan(o[3].y)) || (hasD && __builtin_isnan(o[4].y));
}

}  // namespace

// one wave: strip `strip`, rows [r0, r1).  ROWS (cx_lattice_deep.h: segment_interior) and COLS (strip_interior), both wave-uniform: every
// row touched, resp. every lane's column, lies inside the grid with both neighbours in that direction, so the edge tests of that direction
// below are the constant true and the selects on them compile to nothing.  With both every cell has degree 5 and the ranks are constants.
// With ROWS alone (a column-edge wave) nothing that is tested depends on the row: colv, hasL, hasR and the rank offsets of the loads and
// the stores are per-lane constants of the whole loop, formed once in front of it.  The rule's point mass (deep_rule: selected
// operands, no branch) and the test for an undefined message stay in every instance.
template <int K, bool ROWS, bool COLS>
__device__ __forceinline__ void deep_wave(int strip, int r0, int r1, int H, int W, const int32_t *__restrict__ slice_off, const double *__restrict__ q,
                                          const double2 *__restrict__ f2v_in, double2 *__restrict__ f2v_out, unsigned *__restrict__ abort_word) {
    namespace dp = lattice::deep;
    const int lane = threadIdx.x & 63;
    const int c = dp::lane_col(strip, lane, K);
    const bool colv = COLS || (c >= 0 && c < W);
    const bool hasL = COLS || (colv && c > 0), hasR = COLS || (colv && c < W - 1);
    const bool own = dp::lane_owned(lane, c, W, K) && colv;
    const bool two = hasL && hasR;                      // left AND right: up / down sit one rank higher
    // the ranks that do not depend on the row (ROWS: none does), as slot offsets: the right, the upper and the lower factor of the lane's
    // column, and the right factor of the column to its left (level K's store to the left)
    const int offR = (COLS ? 2 : lattice::rank_right(c)) * kBlock, offU = (COLS ? 3 : lattice::rank_up(c, W)) * kBlock;
    const int offRofL = (COLS ? 2 : lattice::rank_right(c - 1)) * kBlock;
    // A column-edge wave (EDGE) loads every row at every lane without a branch, as the interior instance does, each direction from its own
    // rank: x[1 .. 4] = left, right, up, down.  A direction the lane's column has not is loaded from rank 0 and replaced by +0 at level 1; a
    // lane outside the row reads variable 0 (a corner of the grid: ranks 0 .. 2), and nothing tested or stored depends on what it holds
    constexpr bool EDGE = ROWS && !COLS;
    const int ldL = hasL ? lattice::rank_left() * kBlock : 0, ldR = hasR ? offR : 0, ldU = colv ? offU : 0, ldD = colv ? offU + kBlock : 0;
    bool bad = false;

    // rows outside the grid and lanes outside the row load nothing: zeros, q = 1 (their results are never used).  The lane's first slot of a
    // row is slice_off[v >> 8] + (v & 255).  The slice_off word of row i + 2 is asked for in the iteration of row i, behind the loads of row
    // i + 1, and is kept as loaded; the sum is formed at the top of the next iteration, in front of that iteration's loads.  So no instruction
    // between the loads of a row and the end of the arithmetic of the row before needs a loaded value (profiles/deep_sweep_issue.md: the
    // loop's loads and waits)
    auto in_grid = [&](int r) { return (ROWS || (r >= 0 && r < H)) && colv; };
    auto load_raw = [&](int r) { return EDGE ? slice_off[(colv ? r * W + c : 0) >> kSliceShift] : in_grid(r) ? slice_off[(r * W + c) >> kSliceShift] : 0; };
    auto finish_base = [&](int r, int raw) { return EDGE ? raw + ((colv ? r * W + c : 0) & (kBlock - 1)) : in_grid(r) ? raw + ((r * W + c) & (kBlock - 1)) : 0; };
    auto zero_row = [](int base) {
        DeepRow in;
#pragma unroll
        for (int k = 0; k < 5; k++) in.x[k] = zero2();
        in.qR = 1.0; in.qD = 1.0; in.base = base;
        return in;
    };
    auto load_row = [&](int r, int base) {
        DeepRow in = zero_row(base);
        if (EDGE) {
            in.x[0] = deep_load_stream(&f2v_in[in.base]);
            in.x[1] = deep_load_stream(&f2v_in[in.base + ldL]); in.x[2] = deep_load_stream(&f2v_in[in.base + ldR]);
            in.x[3] = deep_load_stream(&f2v_in[in.base + ldU]); in.x[4] = deep_load_stream(&f2v_in[in.base + ldD]);
            in.qR = q[in.base + ldR]; in.qD = q[in.base + ldD];
        } else if (in_grid(r)) {
            const int deg = COLS ? 5 : lattice::degree(r, c, H, W);
#pragma unroll
            for (int k = 0; k < 5; k++)
                if (k < deg) in.x[k] = deep_load_stream(&f2v_in[in.base + k * kBlock]);
            if (hasR) in.qR = q[in.base + offR];
            if (ROWS || r < H - 1) in.qD = q[in.base + (ROWS ? offU + kBlock : lattice::rank_down(r, c, W) * kBlock)];
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
    // The loop starts one row early, on a row of zeros at which no level works, so that the first row's loads are issued where every other
    // row's are and the loop is entered with no load in flight: the compiler places its waits from what may be outstanding on any path into
    // the loop, and a row loaded in front of the loop cost a wait behind the loads of every iteration.  The empty asm is a use of the word
    // that the load cannot be moved behind
    DeepRow nxt = zero_row(0);
    int raw_next = load_raw(i0);
    asm volatile("" : "+v"(raw_next));
    // Priority that falls with progress: a wave starts at priority 3 and steps down one level at a quarter, a half and three quarters of
    // its row loop.  A SIMD serves its oldest wave first, so its waves end one after the other and the youngest runs on alone; with the
    // wave that is behind served first they end closer together (profiles/deep_sweep_56.md: 1 - 2 % at K = 4, nothing at K = 5 and 6)
    const int quarter = (i1 - i0 + 2) >> 2;
    const int p1 = i0 - 1 + quarter, p2 = p1 + quarter, p3 = p2 + quarter;
    __builtin_amdgcn_s_setprio(3);
    for (int i = i0 - 1; i <= i1; i++) {
        if (i == p1) __builtin_amdgcn_s_setprio(2);          // (uniform)
        else if (i == p2) __builtin_amdgcn_s_setprio(1);
        else if (i == p3) __builtin_amdgcn_s_setprio(0);
        const DeepRow cur = nxt;                             // the one wait for loads of the iteration: in front of the next row's loads
        const int base_next = finish_base(i + 1, raw_next);  // (the word came in behind row i's loads, one iteration ago)
        if (i < i1) nxt = load_row(i + 1, base_next);        // (uniform) in flight until the top of the next iteration: nothing below waits for a load
        if (i + 1 < i1) raw_next = load_raw(i + 2);
        P[0] = cur.x[0]; qR[0] = cur.qR; qD[0] = cur.qD; base[0] = cur.base;
        DeepOut e;
        e.L = zero2(); e.R = zero2(); e.up = zero2(); e.down = zero2();
        if (i >= i0 && (ROWS || (i >= 0 && i < H))) {        // (uniform) level 1 of row i
            const bool hasU = ROWS || i > 0, hasD = ROWS || i < H - 1;
            double2 in[5], o[5];
            const double2 xu = two ? cur.x[3] : cur.x[2];
            const double2 xd = hasU ? (two ? cur.x[4] : cur.x[3]) : xu;
            in[0] = cur.x[0];
            in[1] = dsel2(hasL, cur.x[1], zero2());
            in[2] = dsel2(hasR, EDGE || hasL ? cur.x[2] : cur.x[1], zero2());
            in[3] = EDGE ? cur.x[3] : dsel2(hasU && colv, xu, zero2());
            in[4] = EDGE ? cur.x[4] : dsel2(hasD && colv, xd, zero2());
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
                baseL = ishift_up(base[K - 1]); baseR = ishift_down(base[K - 1]);
                qL = dshift_up(qR[K - 1]);
            }
            // (an interior segment's rows are never clipped by the grid: row_lo / row_hi without the clamp)
            if (ROWS ? (m >= r0 - (K - j) && m < r1 + (K - j)) : dp::row_valid_at_level(m, r0, r1, H, K, j)) {      // (uniform)
                const bool mU = ROWS || m > 0, mD = ROWS || m < H - 1;
                double2 in[5], o[5];
                in[0] = P[j - 1]; in[1] = pend[j].L; in[2] = pend[j].R;
                in[3] = dsel2(mU, pend[j].U, zero2());
                in[4] = dsel2(mD, e.up, zero2());
                deep_leave_one_out(in, o);
                if (dp::lane_valid_at_level(lane, COLS ? 0 : c, COLS ? 1 : W, j)) bad = bad || deep_undefined(o, hasL, hasR, mU, mD);
                if (j < K) f = deep_emit(o, hasL, hasR, qR[j - 1], qD[j], qD[j - 1]);
                else if (own) {                              // level K of an owned row (row_valid_at_level at j = K: r0 <= m < r1): stored
                    if (hasL) f2v_out[baseL + offRofL] = deep_rule(o[1], qL);
                    if (hasR) f2v_out[baseR + lattice::rank_left() * kBlock] = deep_rule(o[2], qR[K - 1]);
                    if (mU) f2v_out[base[K] + (ROWS ? offU + kBlock : lattice::rank_down(m - 1, c, W) * kBlock)] = deep_rule(o[3], qD[K]);
                    if (mD) f2v_out[base[K - 2] + offU] = deep_rule(o[4], qD[K - 1]);
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
    }
    if (bad) *abort_word = 1u;      // (an ordinary per-lane store)
}

#ifdef CX_DEEP_STAMPS
// lab build (CX_BUILD_DEEP_STAMPS=1 python -m cortex.jl_amd.build --force; tools/lab/deep_sweep_stamps.py): every working wave of every launch
// leaves one record of 8 words at slot 4 blockIdx + wave, overwriting the launch before: the 100 MHz clock at entry and exit, the shader clock
// at both, HW_ID | XCC_ID << 32, strip | segment << 32, 1 + instance (0 general, 1 interior, 2 column-edge), blockIdx.  Never defined in the
// shipped library
constexpr int kDeepStampWaves = 4096;
__device__ unsigned long long cx_deep_stamps[kDeepStampWaves * 8];
#endif

// grid = packed_blocks workgroups (cx_lattice_deep.h: the packed map).  Wave w of workgroup (bc, seg) of a full workgroup column owns strip
// 4 bc + w, rows [seg R, seg R + R); in a last column of s < 4 strips a workgroup holds floor(4 / s) consecutive segments, wave w strip
// 4 bc + w mod s of segment seg0 + w div s, and a wave beyond them returns at once
template <int K>
__global__ __launch_bounds__(kBlock) void k_sweep_deep(int H, int W, int R, int nseg, const int32_t *__restrict__ slice_off, const double *__restrict__ q,
                                                       const double2 *__restrict__ f2v_in, double2 *__restrict__ f2v_out, unsigned *__restrict__ abort_word) {
    namespace dp = lattice::deep;
    // consecutive slabs are consecutive segments of one column of workgroups and share an XCD (their halo rows meet in its L2)
    const int s = deep_slab(blockIdx.x, gridDim.x), w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int strip, seg;
    if (!dp::packed_wave(s, w, W, nseg, K, &strip, &seg)) return;      // (wave-uniform)
    const int r0 = seg * R, r1 = min(r0 + R, H);
#ifdef CX_DEEP_STAMPS
    const unsigned long long st_wall = wall_clock64(), st_clk = __builtin_amdgcn_s_memtime();
#endif
    int cls = dp::wave_class(strip, r0, r1, H, W, K);                  // (wave-uniform)
#if defined(CX_DEEP_STAMPS) && CX_DEEP_STAMPS == 2                     // (lab: the stamps of the dispatch before the column-edge instance)
    if (cls == dp::kWaveColumnEdge) cls = dp::kWaveGeneral;
#endif
    if (cls == dp::kWaveInterior) deep_wave<K, true, true>(strip, r0, r1, H, W, slice_off, q, f2v_in, f2v_out, abort_word);
    else if (cls == dp::kWaveColumnEdge) deep_wave<K, true, false>(strip, r0, r1, H, W, slice_off, q, f2v_in, f2v_out, abort_word);
    else deep_wave<K, false, false>(strip, r0, r1, H, W, slice_off, q, f2v_in, f2v_out, abort_word);
#ifdef CX_DEEP_STAMPS
    const unsigned long long en_clk = __builtin_amdgcn_s_memtime(), en_wall = wall_clock64();
    const unsigned hw = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));       // HW_REG_HW_ID, all bits
    const unsigned xcc = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (3 << 11));      // HW_REG_XCC_ID, bits 0 .. 3
    const int slot = (int)blockIdx.x * 4 + w;
    if ((threadIdx.x & 63) == 0 && slot < kDeepStampWaves) {           // (ordinary vector stores of one lane)
        unsigned long long *rec = cx_deep_stamps + (size_t)slot * 8;
        rec[0] = st_wall; rec[1] = en_wall; rec[2] = st_clk; rec[3] = en_clk;
        rec[4] = (unsigned long long)hw | (unsigned long long)xcc << 32;
        rec[5] = (unsigned long long)(unsigned)strip | (unsigned long long)(unsigned)seg << 32;
        rec[6] = 1ull + (unsigned long long)cls; rec[7] = blockIdx.x;
    }
#endif
}

#ifdef CX_DEEP_STAMPS
// the records of the last launch, then cleared (a wave without work leaves zeros); returns the number of records copied
extern "C" __attribute__((visibility("default"))) int32_t cx_lab_deep_stamps(unsigned long long *out, int32_t max_waves) {
    const int n = max_waves < kDeepStampWaves ? max_waves : kDeepStampWaves;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(out, HIP_SYMBOL(cx_deep_stamps), (size_t)n * 64) != hipSuccess) return -1;
    static unsigned long long zeros[kDeepStampWaves * 8];
    if (hipMemcpyToSymbol(HIP_SYMBOL(cx_deep_stamps), zeros, sizeof zeros) != hipSuccess) return -1;
    return n;
}
#endif

template <int K>
static int64_t deep_capacity(const cx_handle *h) {
    int per_cu = 0, dev = h->cfg.device;
    hipDeviceProp_t prop;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_sweep_deep<K>, kBlock, 0) != hipSuccess || per_cu <= 0) { (void)hipGetLastError(); per_cu = 2; }
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) { (void)hipGetLastError(); return (int64_t)per_cu * 256; }
    return (int64_t)per_cu * prop.multiProcessorCount;
}

// workgroups of k_sweep_deep<depth> the device holds at once, depth 3 .. 6: three waves per SIMD at depths 3 and 4, two at 5 and 6
int64_t deep_capacity_blocks(const cx_handle *h, int depth) {
    switch (depth) {
    case 3: return deep_capacity<3>(h);
    case 4: return deep_capacity<4>(h);
    case 5: return deep_capacity<5>(h);
    default: return deep_capacity<6>(h);
    }
}

template <int K>
static void deep_launch(cx_handle *h, dim3 grid, int R, int nseg, const double2 *f2v_in, double2 *f2v_out) {
    hipLaunchKernelGGL(k_sweep_deep<K>, grid, dim3(kBlock), 0, h->stream, h->pair_H, h->pair_W, R, nseg, h->d_slice_off, h->d_q, f2v_in, f2v_out, h->pair_abort.dev);
}

void launch_sweep_deep(cx_handle *h, int depth, const double2 *f2v_in, double2 *f2v_out) {
    const int R = h->deep_rows[depth], nseg = (h->pair_H + R - 1) / R;
    const dim3 grid((unsigned)lattice::deep::packed_blocks(h->pair_W, nseg, depth));
    switch (depth) {
    case 3: deep_launch<3>(h, grid, R, nseg, f2v_in, f2v_out); break;
    case 4: deep_launch<4>(h, grid, R, nseg, f2v_in, f2v_out); break;
    case 5: deep_launch<5>(h, grid, R, nseg, f2v_in, f2v_out); break;
    default: deep_launch<6>(h, grid, R, nseg, f2v_in, f2v_out); break;
    }
}

}  // namespace cx
