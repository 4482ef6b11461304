"""The interior instance of the deep sweep (cortex.jl_amd/csrc/cx_lattice_deep.h: strip_interior, segment_interior) on the CPU build of the
host logic.  A wave that takes the interior instance tests no edge of the grid and loads every row at every lane unconditionally, so whenever
the two predicates say interior, every lane and every row at every level that the general path would test must have a left, a right, an upper
and a lower neighbour inside the grid.  cxh_lattice_deep_interior enumerates those cells with lane_col, row_lo and row_hi; the flagship's
count is derived by hand below, and a few shapes are enumerated again in this file from the formulas alone."""
import ctypes as C

import numpy as np
import pytest

from tests.hostlogic import lib

DEPTHS = (3, 4)
WIDTHS = range(1, 301)
HEIGHTS = range(1, 41)
ROWS = range(1, 21)


def interior(K, W, H, R, buffers=None):
    """(pred, general), one entry per wave, strips major: the kernel's choice and what the general predicates say of the wave's cells"""
    fn = lib().cxh_lattice_deep_interior
    fn.restype = C.c_int32
    fn.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    cols = 64 - 2 * (K - 1)
    n = -(-W // cols) * -(-H // R)
    pred, general = buffers if buffers else (np.empty(n, dtype=np.int8), np.empty(n, dtype=np.int8))
    assert len(pred) >= n
    pred[:n] = -7
    general[:n] = -7
    assert fn(K, W, H, R, pred.ctypes.data, general.ctypes.data) == n
    return pred[:n], general[:n]


@pytest.mark.parametrize("K", DEPTHS)
def test_an_interior_wave_meets_no_edge_of_the_grid(K):
    buffers = (np.empty(4096, dtype=np.int8), np.empty(4096, dtype=np.int8))
    said = {0: 0, 1: 0}
    for W in WIDTHS:
        for H in HEIGHTS:
            for R in ROWS:
                pred, general = interior(K, W, H, R, buffers)
                assert np.all((pred == 0) | (pred == 1)) and np.all((general == 0) | (general == 1))
                assert np.all(general[pred == 1] == 1), f"depth {K}, {H} x {W}, {R} rows per segment: waves {np.flatnonzero((pred == 1) & (general == 0))}"
                said[1] += int(pred.sum())
                said[0] += int(len(pred) - pred.sum())
    assert said[0] > 0 and said[1] > 0, said


@pytest.mark.parametrize("K", DEPTHS)
def test_the_predicates_are_exact(K):
    """not asked of the kernel, which may always take the general instance, but it is what makes the flagship's count below the whole gain"""
    for W, H, R in [(300, 40, 8), (180, 40, 8), (130, 24, 5), (299, 39, 20), (62, 40, 3)]:
        pred, general = interior(K, W, H, R)
        assert np.array_equal(pred, general), (K, W, H, R)


def _by_hand(K, W, H, R):
    """the same answer from the formulas alone: lane l of strip s is column s (64 - 2 (K - 1)) - (K - 1) + l; the wave of segment [r0, r1)
    loads rows r0 - (K - 1) .. r1 + (K - 1) - 1, and level j works on rows r0 - (K - j) .. r1 + (K - j) - 1 of them"""
    cols = 64 - 2 * (K - 1)
    out = []
    for strip in range(-(-W // cols)):
        c = strip * cols - (K - 1) + np.arange(64)
        strip_ok = bool(np.all((c >= 1) & (c <= W - 2)))
        for seg in range(-(-H // R)):
            r0, r1 = seg * R, min(seg * R + R, H)
            rows = np.arange(r0 - (K - 1), r1 + (K - 1))
            out.append(strip_ok and bool(np.all((rows >= 1) & (rows <= H - 2))))
    return np.array(out, dtype=np.int8)


@pytest.mark.parametrize("K", DEPTHS)
@pytest.mark.parametrize("shape", [(40, 180, 8), (40, 130, 8), (5, 180, 8), (24, 180, 13), (40, 300, 1), (1415, 1415, 13)], ids=str)
def test_against_the_formulas_written_out_here(K, shape):
    H, W, R = shape
    pred, _ = interior(K, W, H, R)
    assert np.array_equal(pred, _by_hand(K, W, H, R))


def test_the_flagship_count():
    """1415 x 1415, depth 4, 13 rows per segment.  58 owned columns per strip: 25 strips, strip s at columns 58 s - 3 .. 58 s + 60.  Strip 0
    starts at column -3 and strip 24 ends at 1452 > 1413: not interior; strips 1 .. 23 lie within 55 .. 1394: 23 strips.  109 segments of
    13 rows (the last one 1404 .. 1414); segment g loads rows 13 g - 3 .. 13 g + 15.  Segment 0 starts at row -3; segment 107 ends at
    1406 <= 1413; segment 108 would end at 1417: segments 1 .. 107, 107 of them.  23 x 107 = 2461 of the 2725 waves."""
    pred, general = interior(4, 1415, 1415, 13)
    assert len(pred) == 25 * 109
    assert int(pred.sum()) == 23 * 107 == 2461
    assert np.array_equal(pred, general)
    by_wave = pred.reshape(25, 109)
    assert not by_wave[0].any() and not by_wave[24].any() and not by_wave[:, 0].any() and not by_wave[:, 108].any()
    assert by_wave[1:24, 1:108].all()
