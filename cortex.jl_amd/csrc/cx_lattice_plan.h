// cx_lattice_plan.h — a 4-neighbour grid recognised in the SELL slot space, and the strips the paired sweep (cx_sweep_pair.hip: two sweeps per
// launch) cuts it into.  Pure C++ (cx_graph_create builds the plan beside the partner runs, cx_hostlogic.cpp exports it to the CPU tests);
// the small geometry functions are also compiled for the device, so that the kernel and the plan's proof use the same arithmetic.
//
// The graph is recognised from partner, slice_off and vinfo alone, never from ids.  It qualifies when it is an H x W grid (H, W >= 2) with the
// variables in row-major order, every variable free (not observed, no stand-in, no big degree), rank 0 of every variable a partnerless slot
// (the unary message) and the other ranks in the order left, right, up, down with absent directions skipped — what ascending factor ids give
// when unary < horizontal < vertical (synth.gaussian_grid).  The proof: for every variable and direction the destination slot computed
// arithmetically, slice_off[v' >> 8] + rank'(opposite) * 256 + (v' & 255) with v' the neighbour, equals partner[slot] from the table.
// One mismatch anywhere: no plan, the handle sweeps as before.
//
// Decomposition.  A wave owns a strip of kStripCols consecutive columns plus one halo column on each side: 64 lanes = 64 consecutive
// variable ids of one grid row, so every access is a unit-stride run along the id order.  The rows are cut into segments of R; one wave per
// (strip, segment) streams down rows r0 - 1 .. r1 (one halo row on each side); four adjacent strips of one segment share a workgroup.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "cx_const.h"

#if defined(__HIPCC__)
#define CX_LAT_HD __host__ __device__ __forceinline__
#else
#define CX_LAT_HD inline
#endif

namespace cx {
namespace lattice {

constexpr int kStripCols = 62;       // owned columns per wave: 64 lanes minus the two halo lanes
constexpr int kStripsPerBlock = 4;   // waves of a workgroup = adjacent strips of one segment
// R below 4 reads (1 + 2/R) >= 1.5 times the messages, where a pair stops moving fewer bytes than two plain sweeps save for the write
// (160 x 1.5 + 128 against 320 + 256 MB on the 10 M-edge grid is still a gain, 160 x 3 + 128 at R = 1 is not): a grid too tall for one
// resident round at R = 4 runs more than one round instead.  Above 64 a wave's stream is long enough that the halo rows are 3 % and
// nothing is left to gain, while a short grid would be left to too few waves.
constexpr int kMinRows = 4, kMaxRows = 64;

// ---- geometry shared with the kernel -------------------------------------------------------------------------------------------
CX_LAT_HD int lane_col(int strip, int lane) { return strip * kStripCols - 1 + lane; }                       // (-1 and >= W: outside)
CX_LAT_HD bool lane_owned(int lane, int col, int W) { return lane >= 1 && lane <= kStripCols && col < W; }  // (lane >= 1: col >= 0)
// ranks of the four directions at variable (r, c): rank 0 is the unary slot, absent directions are skipped
CX_LAT_HD int rank_left() { return 1; }
CX_LAT_HD int rank_right(int c) { return 1 + (c > 0 ? 1 : 0); }
CX_LAT_HD int rank_up(int c, int W) { return 1 + (c > 0 ? 1 : 0) + (c < W - 1 ? 1 : 0); }
CX_LAT_HD int rank_down(int r, int c, int W) { return rank_up(c, W) + (r > 0 ? 1 : 0); }
CX_LAT_HD int degree(int r, int c, int H, int W) { return rank_down(r, c, W) + (r < H - 1 ? 1 : 0); }
CX_LAT_HD int slot_base(const int32_t *slice_off, int v) { return slice_off[v >> kSliceShift] + (v & (kBlock - 1)); }

struct Plan {
    bool ok = false;
    std::string reason;      // why there is no plan (empty with one)
    int32_t H = 0, W = 0, strips = 0, block_cols = 0;
};

inline int32_t n_segments(const Plan &p, int R) { return (p.H + R - 1) / R; }

// rows per segment such that every workgroup of the launch is resident at once: capacity_blocks = workgroups the chip holds of this kernel
inline int choose_rows(const Plan &p, int64_t capacity_blocks) {
    const int64_t seg_max = std::max<int64_t>(1, capacity_blocks / std::max<int32_t>(1, p.block_cols));
    const int64_t R = (p.H + seg_max - 1) / seg_max;
    return (int)std::min<int64_t>(kMaxRows, std::max<int64_t>(kMinRows, R));
}

// the slot that variable (r, c) sends to in direction d (0 left, 1 right, 2 up, 3 down), computed; -1: no such neighbour
inline int32_t dest_slot(const Plan &p, const int32_t *slice_off, int r, int c, int d) {
    const int W = p.W, H = p.H;
    switch (d) {
    case 0: return c > 0 ? slot_base(slice_off, r * W + c - 1) + rank_right(c - 1) * kBlock : -1;
    case 1: return c < W - 1 ? slot_base(slice_off, r * W + c + 1) + rank_left() * kBlock : -1;
    case 2: return r > 0 ? slot_base(slice_off, (r - 1) * W + c) + rank_down(r - 1, c, W) * kBlock : -1;
    default: return r < H - 1 ? slot_base(slice_off, (r + 1) * W + c) + rank_up(c, W) * kBlock : -1;
    }
}
inline int32_t source_rank(const Plan &p, int r, int c, int d) {
    return d == 0 ? rank_left() : d == 1 ? rank_right(c) : d == 2 ? rank_up(c, p.W) : rank_down(r, c, p.W);
}

// q (may be null): the rule parameter per slot; the kernel reads a factor's q at ONE of its two slots, so both must hold the same value
inline Plan build(const std::vector<int32_t> &partner, const std::vector<int32_t> &slice_off, const std::vector<uint8_t> &vinfo, int64_t nv,
                  const double *q = nullptr) {
    Plan p;
    auto no = [&p](const char *why) { p.ok = false; p.reason = why; return p; };
    if (nv < 4 || nv > (int64_t)1 << 30 || slice_off.size() < 2) return no("not a grid: fewer than 2 x 2 variables");
    for (int64_t v = 0; v < nv; v++) {
        if (vinfo[v] & (kClamped | kGhost)) return no("a variable is observed or a stand-in");
        if ((vinfo[v] & kDegMask) == kBigDeg) return no("a variable of big degree");
    }
    // the top row: corner (degree 3), inner variables (degree 4), corner — its length is W
    int64_t W = 0;
    for (int64_t v = 1; v < nv; v++) if ((vinfo[v] & kDegMask) != 4) { W = v + 1; break; }
    if (W < 2 || nv % W != 0 || nv / W < 2) return no("not a grid: the variables do not form H x W rows with H, W >= 2");
    p.H = (int32_t)(nv / W); p.W = (int32_t)W;
    const int32_t *so = slice_off.data();
    // first the shape (degrees, the unary slot), then the partners: a variable that is wrong in itself is named before its neighbours' partners are
    for (int r = 0; r < p.H; r++)
        for (int c = 0; c < p.W; c++) {
            const int v = r * p.W + c, deg = vinfo[v] & kDegMask, base = slot_base(so, v);
            const bool unary = partner[base] < 0;
            if (deg != degree(r, c, p.H, p.W)) {
                bool shifted = deg == degree(r, c, p.H, p.W) - 1 && !unary;      // the grid's variable, its four directions one rank early?
                for (int d = 0; d < 4 && shifted; d++) {
                    const int32_t want = dest_slot(p, so, r, c, d);
                    if (want >= 0 && partner[base + (source_rank(p, r, c, d) - 1) * kBlock] != want) shifted = false;
                }
                if (shifted) return no("a variable without the unary message at rank 0");
                return no("not a grid: a variable's degree does not match its place in H x W rows");
            }
            if (!unary) return no("rank 0 of a variable is not a partnerless slot");
        }
    auto var_of_slot = [&](int32_t s) -> int64_t {
        if (s < 0 || s >= slice_off.back()) return -1;
        const int64_t sl = std::upper_bound(slice_off.begin(), slice_off.end(), s) - slice_off.begin() - 1;
        return sl * kBlock + ((s - slice_off[sl]) & (kBlock - 1));
    };
    auto neighbour = [&](int r, int c, int d) -> int64_t { return d == 0 ? r * W + c - 1 : d == 1 ? r * W + c + 1 : d == 2 ? (r - 1) * W + c : (r + 1) * W + c; };
    for (int r = 0; r < p.H; r++)
        for (int c = 0; c < p.W; c++) {
            const int v = r * p.W + c, deg = vinfo[v] & kDegMask, base = slot_base(so, v);
            bool exact = true, as_set = true;
            for (int d = 0; d < 4; d++) {
                const int32_t want = dest_slot(p, so, r, c, d);
                if (want < 0) continue;
                const int32_t s = base + source_rank(p, r, c, d) * kBlock;
                if (partner[s] != want) exact = false;
                bool found = false;      // the neighbour is a partner at SOME rank: the right variables in another order
                for (int k = 1; k < deg; k++) found = found || var_of_slot(partner[base + k * kBlock]) == neighbour(r, c, d);
                if (!found) as_set = false;
                if (q && partner[s] == want && !(q[s] == q[want])) return no("a factor whose two slots hold different rule parameters");
            }
            if (!exact) return no(as_set ? "the ranks are not in the order unary, left, right, up, down" : "not a grid: a partner is not the row-major neighbour");
        }
    p.strips = (p.W + kStripCols - 1) / kStripCols;
    p.block_cols = (p.strips + kStripsPerBlock - 1) / kStripsPerBlock;
    p.ok = true;
    return p;
}

// how many (strip, segment) waves store for each variable at R rows per segment, by the kernel's own predicates (the tests want 1 everywhere)
inline void cover(const Plan &p, int R, std::vector<int32_t> &count) {
    count.assign((size_t)p.H * p.W, 0);
    const int nseg = n_segments(p, R);
    for (int bc = 0; bc < p.block_cols; bc++)
        for (int seg = 0; seg < nseg; seg++)
            for (int w = 0; w < kStripsPerBlock; w++) {
                const int strip = bc * kStripsPerBlock + w;
                if (strip * kStripCols >= p.W) continue;
                const int r0 = seg * R, r1 = std::min(r0 + R, (int)p.H);
                for (int r = r0; r < r1; r++)
                    for (int lane = 0; lane < 64; lane++) {
                        const int c = lane_col(strip, lane);
                        if (lane_owned(lane, c, p.W)) count[(size_t)r * p.W + c]++;
                    }
            }
}

}  // namespace lattice
}  // namespace cx
