// cx_partner_runs.h — the partners of the SELL slots as wave-uniform runs (pure C++: cx_graph_create builds the table, cx_hostlogic.cpp
// exports the builder to the CPU tests).
//
// On grids, chains and banded graphs partner[slot] - slot is constant over long runs of lanes.  Per 256-slot row of the slot space and
// per wave of the workgroup that owns the row (four of 64 lanes) one entry {d0, d1, split}: lanes with (tid & 63) < split have
// partner = slot + d0, the others slot + d1; a piece whose lanes all have no partner carries kNone; split < 0: the wave has three or
// more pieces and reads the per-lane index as before.  Lanes the sweep never pushes from — k >= degree, v >= nv, variables of big degree
// (their slots are in the CSR tail) — are don't-cares and join whichever piece keeps the entry representable.
// The packed instances of k_sweep (cx_kernels.hip) read the entry through a wave-uniform index: no vector register, no vector-memory
// round trip in front of the scatter stores.
#pragma once

#include <cstdint>
#include <vector>

#include "cx_const.h"

namespace cx {
namespace pruns {

constexpr int32_t kNone = INT32_MIN;
struct Entry { int32_t d0, d1, split, pad; };      // 16 bytes: one scalar load

// entries: [rows][4], rows = slice_off.back() / kBlock; returns how many have split < 0
inline int64_t build(const std::vector<int32_t> &partner, const std::vector<int32_t> &slice_off, const std::vector<uint8_t> &vinfo, int64_t nv,
                     std::vector<Entry> &out) {
    const int64_t nslices = slice_off.empty() ? 0 : (int64_t)slice_off.size() - 1;
    const int64_t rows = nslices ? slice_off[nslices] / kBlock : 0;
    out.assign((size_t)rows * 4, Entry{kNone, kNone, 64, 0});
    int64_t fallback = 0;
    for (int64_t s = 0; s < nslices; s++) {
        const int64_t off = slice_off[s], W = (slice_off[s + 1] - off) / kBlock;
        for (int64_t k = 0; k < W; k++)
            for (int w = 0; w < 4; w++) {
                Entry e{kNone, kNone, 64, 0};
                int pieces = 0;
                for (int l = 0; l < 64; l++) {
                    const int64_t t = w * 64 + l, v = s * kBlock + t;
                    if (v >= nv) break;
                    const int deg = vinfo[v] & kDegMask;
                    if (deg == kBigDeg || k >= deg) continue;
                    const int64_t slot = off + k * kBlock + t, p = partner[slot];
                    const int32_t d = p < 0 ? kNone : (int32_t)(p - slot);
                    if (pieces == 0) { e.d0 = e.d1 = d; pieces = 1; }
                    else if (pieces == 1 && d != e.d0) { e.d1 = d; e.split = l; pieces = 2; }
                    else if (pieces == 2 && d != e.d1) { pieces = 3; break; }
                }
                if (pieces == 3) { e = Entry{0, 0, -1, 0}; fallback++; }
                out[(size_t)(off / kBlock + k) * 4 + w] = e;
            }
    }
    return fallback;
}

}  // namespace pruns
}  // namespace cx
