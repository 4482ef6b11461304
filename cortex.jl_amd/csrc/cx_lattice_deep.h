// cx_lattice_deep.h — the strips of the deep sweep (cx_sweep_deep.hip: K sweeps per launch on the grid plan of cx_lattice_plan.h), with the depth
// K as a parameter.  Pure C++, shared by the host, the kernel and the CPU tests (cx_hostlogic.cpp: cxh_flat_lattice_deep) like the plan itself.
//
// Decomposition.  A wave owns strip_cols(K) = 64 - 2 (K - 1) consecutive columns and has K - 1 halo lanes on each side; a segment of R rows
// has K - 1 halo rows at each end: the wave loads rows r0 - (K - 1) .. r1 + (K - 1) - 1 at its 64 lanes.  Level 1 is the sweep that reads
// what was loaded, level j the j-th sweep of the launch; level K is stored, at the owned cells only.
//
// Validity.  A cell's level-j value depends on the loaded cells within distance j - 1 of it.  Here a cell is VALID at level j when it lies in
// the grid and within K - j lanes and K - j rows of the owned rectangle: then everything within j - 1 of it lies within K - 1 of the owned
// rectangle, which is what the wave loaded, or outside the grid, where a sweep reads nothing.  A cell that is not valid at a level holds
// garbage there; it feeds only cells that are not valid one level up (a valid cell's in-grid neighbours are valid one level down), and it is
// neither tested for an undefined message nor stored.  (Near the grid's edge a few more cells would qualify by the clipped distance; they
// are owned by another wave, which tests them, and leaving them out keeps the rule one comparison per side.)  Lanes 0 and 63 are valid at
// level 1 only (K >= 2) and never owned: what a level's sideways shift delivers to them — a shuffle the lane's own value, the kernel's
// whole-wave shift zero — is garbage of this kind, and nothing tested or stored depends on it.
#pragma once

#include "cx_lattice_plan.h"

namespace cx {
namespace lattice {
namespace deep {

constexpr int kMinDepth = 2, kMaxDepth = 6;

CX_LAT_HD int strip_cols(int K) { return 64 - 2 * (K - 1); }
CX_LAT_HD int lane_col(int strip, int lane, int K) { return strip * strip_cols(K) - (K - 1) + lane; }                             // (< 0 and >= W: outside)
CX_LAT_HD bool lane_owned(int lane, int col, int W, int K) { return lane >= K - 1 && lane <= 64 - K && col < W; }                  // (lane >= K - 1: col >= 0)
CX_LAT_HD bool lane_valid_at_level(int lane, int col, int W, int j) { return lane >= j - 1 && lane <= 64 - j && col >= 0 && col < W; }
// rows of segment [r0, r1) valid at level j: [row_lo, row_hi)
CX_LAT_HD int row_lo(int r0, int K, int j) { return r0 - (K - j) > 0 ? r0 - (K - j) : 0; }
CX_LAT_HD int row_hi(int r1, int H, int K, int j) { return r1 + (K - j) < H ? r1 + (K - j) : H; }
CX_LAT_HD bool row_valid_at_level(int r, int r0, int r1, int H, int K, int j) { return r >= row_lo(r0, K, j) && r < row_hi(r1, H, K, j); }
// what the wave loads: rows [load_lo, load_hi) of the grid at the lanes whose column is inside it
CX_LAT_HD int load_lo(int r0, int K) { return row_lo(r0, K, 1); }
CX_LAT_HD int load_hi(int r1, int H, int K) { return row_hi(r1, H, K, 1); }

// Interior waves (the kernel's second instance: no edge tests).  A strip is interior when every one of its 64 lanes holds a column of the grid
// that has a left and a right neighbour; a segment is interior when every row it loads, r0 - (K - 1) .. r1 + (K - 1) - 1, which are all the rows
// it touches at any level, has a row above and a row below.  For such a wave hasL, hasR, hasU, hasD and the column test are true at every lane,
// row and level, every cell has degree 5, and row_lo / row_hi are never clipped by the grid.
CX_LAT_HD bool strip_interior(int strip, int W, int K) { return lane_col(strip, 0, K) >= 1 && lane_col(strip, 63, K) <= W - 2; }
CX_LAT_HD bool segment_interior(int r0, int r1, int H, int K) { return r0 - (K - 1) >= 1 && r1 + (K - 1) - 1 <= H - 2; }

// The three instances of the kernel, by wave.  A column-edge wave has an interior segment and a strip that is not: every row it touches at
// any level lies in 1 .. H - 2, so every row test is true and what is left to test (the lane's column, its left and right neighbour) does not
// change over the wave's row loop.  On a grid narrower than a strip both edge columns lie in the one strip.  Every other wave that is not
// interior — the top and bottom segments, whatever the strip — is general.
constexpr int kWaveGeneral = 0, kWaveInterior = 1, kWaveColumnEdge = 2;
CX_LAT_HD bool column_edge(int strip, int r0, int r1, int H, int W, int K) { return segment_interior(r0, r1, H, K) && !strip_interior(strip, W, K); }
CX_LAT_HD int wave_class(int strip, int r0, int r1, int H, int W, int K) {
    if (!segment_interior(r0, r1, H, K)) return kWaveGeneral;
    return strip_interior(strip, W, K) ? kWaveInterior : kWaveColumnEdge;
}

CX_LAT_HD int32_t strips(int W, int K) { return (W + strip_cols(K) - 1) / strip_cols(K); }
inline int32_t block_cols(int W, int K) { return (strips(W, K) + kStripsPerBlock - 1) / kStripsPerBlock; }

// The packed map: which (strip, segment) wave w of workgroup `slab` runs, on nseg segments.  A full workgroup column bc (four strips) holds one
// workgroup per segment, column by column: wave w runs strip 4 bc + w.  A last column of s < 4 strips would leave 4 - s waves of every
// workgroup without work; there a workgroup takes floor(4 / s) consecutive segments, from seg0 on: wave w runs strip 4 bc + w mod s of
// segment seg0 + w div s.  False: the wave has no work (w div s beyond floor(4 / s), a segment beyond the last, a slab beyond packed_blocks)
CX_LAT_HD bool packed_wave(int slab, int w, int W, int nseg, int K, int *strip, int *seg) {
    const int full = strips(W, K) / kStripsPerBlock, s = strips(W, K) - full * kStripsPerBlock;
    if (slab < full * nseg) {
        const int bc = slab / nseg;
        *strip = bc * kStripsPerBlock + w; *seg = slab - bc * nseg;
        return true;
    }
    if (s == 0) return false;
    const int per = kStripsPerBlock / s, seg0 = (slab - full * nseg) * per;
    *strip = full * kStripsPerBlock + w % s; *seg = seg0 + w / s;
    return w / s < per && *seg < nseg;
}
// the workgroups of a launch under the packed map: the slabs that hold a wave with work
CX_LAT_HD int32_t packed_blocks(int W, int nseg, int K) {
    const int full = strips(W, K) / kStripsPerBlock, s = strips(W, K) - full * kStripsPerBlock;
    if (s == 0) return full * nseg;
    const int per = kStripsPerBlock / s;
    return full * nseg + (nseg + per - 1) / per;
}// fewer than 4 (K - 1) rows per segment read (1 + 2 (K - 1) / R) > 1.5 times the messages: a grid too tall for one resident round runs more
// than one round instead (cx_lattice_plan.h: kMinRows is this floor at K = 2)
inline int min_rows(int K) { return 4 * (K - 1); }

// rows per segment such that every workgroup of the launch is resident at once (capacity_blocks: workgroups the chip holds of the depth-K kernel)
inline int choose_rows(const Plan &p, int64_t capacity_blocks, int K) {
    const int64_t seg_max = std::max<int64_t>(1, capacity_blocks / std::max<int32_t>(1, block_cols(p.W, K)));
    const int64_t R = (p.H + seg_max - 1) / seg_max;
    return (int)std::min<int64_t>(kMaxRows, std::max<int64_t>(min_rows(K), R));
}

// the same under the packed map: the fewest rows, not below min_rows(K), at which the packed launch is resident (never more than choose_rows:
// packing only takes workgroups away)
inline int choose_rows_packed(const Plan &p, int64_t capacity_blocks, int K) {
    for (int R = min_rows(K); R < kMaxRows; R++)
        if (packed_blocks(p.W, n_segments(p, R), K) <= capacity_blocks) return R;
    return kMaxRows;
}

// how many (strip, segment) waves store for each variable at depth K and R rows per segment, by the kernel's own predicates (the tests want 1)
inline void cover(const Plan &p, int R, int K, std::vector<int32_t> &count) {
    count.assign((size_t)p.H * p.W, 0);
    const int nseg = n_segments(p, R), bcs = block_cols(p.W, K);
    for (int bc = 0; bc < bcs; bc++)
        for (int seg = 0; seg < nseg; seg++)
            for (int w = 0; w < kStripsPerBlock; w++) {
                const int strip = bc * kStripsPerBlock + w;
                if (strip * strip_cols(K) >= p.W) continue;
                const int r0 = seg * R, r1 = std::min(r0 + R, (int)p.H);
                for (int r = r0; r < r1; r++)
                    for (int lane = 0; lane < 64; lane++) {
                        const int c = lane_col(strip, lane, K);
                        if (lane_owned(lane, c, p.W, K)) count[(size_t)r * p.W + c]++;
                    }
            }
}

}  // namespace deep
}  // namespace lattice
}  // namespace cx
