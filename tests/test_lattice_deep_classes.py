"""The three instances of the deep sweep (cortex.jl_amd/csrc/cx_lattice_deep.h: wave_class, column_edge) on the CPU build of the host logic.
A column-edge wave tests no row: whenever the predicates say column-edge (or interior), every row the wave loads and every row it works on at
every level must have an upper and a lower neighbour inside the grid, unclipped.  cxh_lattice_deep_classes enumerates those rows with row_lo
and row_hi beside the kernel's choice; the flagship's counts are derived by hand below, and a few shapes are written out in this file."""
import ctypes as C

import numpy as np
import pytest

from tests.hostlogic import lib
from tests.test_lattice_deep_interior import interior

DEPTHS = (3, 4)
WIDTHS = range(1, 301)
HEIGHTS = range(1, 41)
ROWS = range(1, 21)
GENERAL, INTERIOR, COLUMN_EDGE = 0, 1, 2


def classes(K, W, H, R, buffers=None):
    """(cls, rows_ok, cols_ok), one entry per wave, strips major: the kernel's choice, and what the general path finds of the wave's rows and
    of its lanes' columns"""
    fn = lib().cxh_lattice_deep_classes
    fn.restype = C.c_int32
    fn.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    cols = 64 - 2 * (K - 1)
    n = -(-W // cols) * -(-H // R)
    bufs = buffers if buffers else tuple(np.empty(n, dtype=np.int8) for _ in range(3))
    assert len(bufs[0]) >= n
    for b in bufs:
        b[:n] = -7
    assert fn(K, W, H, R, *(b.ctypes.data for b in bufs)) == n
    return tuple(b[:n] for b in bufs)


@pytest.mark.parametrize("K", DEPTHS)
def test_a_column_edge_wave_meets_no_row_edge_and_the_interior_class_is_the_interior_instance(K):
    buffers = tuple(np.empty(4096, dtype=np.int8) for _ in range(3))
    old = (np.empty(4096, dtype=np.int8), np.empty(4096, dtype=np.int8))
    said = {GENERAL: 0, INTERIOR: 0, COLUMN_EDGE: 0}
    for W in WIDTHS:
        for H in HEIGHTS:
            for R in ROWS:
                what = f"depth {K}, {H} x {W}, {R} rows per segment"
                cls, rows_ok, cols_ok = classes(K, W, H, R, buffers)
                assert np.all((cls >= 0) & (cls <= 2)) and np.all((rows_ok == 0) | (rows_ok == 1)) and np.all((cols_ok == 0) | (cols_ok == 1)), what
                pred, _ = interior(K, W, H, R, old)
                assert np.array_equal(cls == INTERIOR, pred == 1), what
                assert np.all(rows_ok[cls == COLUMN_EDGE] == 1), f"{what}: waves {np.flatnonzero((cls == COLUMN_EDGE) & (rows_ok == 0))}"
                assert np.all(rows_ok[cls == INTERIOR] == 1) and np.all(cols_ok[cls == INTERIOR] == 1), what
                # exact: the class says all that the cells allow
                assert np.array_equal(cls == COLUMN_EDGE, (rows_ok == 1) & (cols_ok == 0)), what
                assert np.array_equal(cls == GENERAL, rows_ok == 0), what
                for k in said:
                    said[k] += int((cls == k).sum())
    assert all(v > 0 for v in said.values()), said


def _by_hand(K, W, H, R):
    """from the formulas alone: lane l of strip s is column s (64 - 2 (K - 1)) - (K - 1) + l; the wave of segment [r0, r1) touches rows
    r0 - (K - 1) .. r1 + (K - 1) - 1"""
    cols = 64 - 2 * (K - 1)
    out = []
    for strip in range(-(-W // cols)):
        c = strip * cols - (K - 1) + np.arange(64)
        strip_ok = bool(np.all((c >= 1) & (c <= W - 2)))
        for seg in range(-(-H // R)):
            r0, r1 = seg * R, min(seg * R + R, H)
            rows = np.arange(r0 - (K - 1), r1 + (K - 1))
            rows_ok = bool(np.all((rows >= 1) & (rows <= H - 2)))
            out.append(GENERAL if not rows_ok else INTERIOR if strip_ok else COLUMN_EDGE)
    return np.array(out, dtype=np.int8)


@pytest.mark.parametrize("K", DEPTHS)
@pytest.mark.parametrize("shape", [(40, 180, 8), (40, 130, 8), (5, 180, 8), (24, 180, 13), (40, 300, 1), (40, 2, 3), (40, 57, 12), (1415, 1415, 12)], ids=str)
def test_against_the_formulas_written_out_here(K, shape):
    H, W, R = shape
    assert np.array_equal(classes(K, W, H, R)[0], _by_hand(K, W, H, R))


def test_shapes_written_out_by_hand():
    """40 x 180 at depth 4, 8 rows per segment: strips of 58 columns at -3 .. 60, 55 .. 118, 113 .. 176, 171 .. 234: strips 1 and 2 lie in
    1 .. 178, strips 0 and 3 do not.  Five segments; segment g touches rows 8 g - 3 .. 8 g + 10: segment 0 starts at -3, segment 4 ends at 42,
    segments 1 .. 3 lie in 5 .. 34, within 1 .. 38."""
    G, I, E = GENERAL, INTERIOR, COLUMN_EDGE
    assert classes(4, 180, 40, 8)[0].reshape(4, 5).tolist() == [[G, E, E, E, G], [G, I, I, I, G], [G, I, I, I, G], [G, E, E, E, G]]
    # a grid narrower than a strip (depth 3: one strip of 60 columns at -2 .. 61): both edge columns in the one wave; 40 rows in segments of
    # 12: rows -2 .. 13, 10 .. 25, 22 .. 37, 34 .. 41
    assert classes(3, 2, 40, 12)[0].tolist() == [G, E, E, G]
    # 20 rows at the floor 4 (K - 1) = 12 rows per segment at depth 4: rows -3 .. 14 and 9 .. 22: no row-interior segment
    assert classes(4, 130, 20, 12)[0].tolist() == [G] * 6
    # depth 3, 20 x 125, 1 row per segment: segment g touches rows g - 2 .. g + 2: segments 3 .. 16; strips at -2 .. 61, 58 .. 121, 118 .. 181
    want = np.full((3, 20), G)
    want[0, 3:17] = E; want[1, 3:17] = I; want[2, 3:17] = E
    assert np.array_equal(classes(3, 125, 20, 1)[0].reshape(3, 20), want)


@pytest.mark.parametrize("K, interior_n, edge_n, other_n", [(4, 2668, 232, 50), (3, 2552, 232, 48)])
def test_the_flagship_counts(K, interior_n, edge_n, other_n):
    """1415 x 1415 at 12 rows per segment: 118 segments, segment g touches rows 12 g - (K - 1) .. 12 g + 12 + (K - 1) - 1.  Segment 0 starts
    above the grid; segment 117 (rows 1404 .. 1414) ends at the grid's last row; segment 116 ends at 1403 + K <= 1413: 116 row-interior
    segments.  Depth 4: 25 strips of 58 columns, strips 0 and 24 not interior: 23 x 116 = 2,668 interior, 2 x 116 = 232 column-edge,
    25 x 2 = 50 other.  Depth 3: 24 strips of 60, strip 23 at 1378 .. 1441: 22 x 116 = 2,552, 232 and 24 x 2 = 48."""
    cls, rows_ok, cols_ok = classes(K, 1415, 1415, 12)
    nstrips = -(-1415 // (64 - 2 * (K - 1)))
    assert len(cls) == nstrips * 118 == interior_n + edge_n + other_n
    assert (int((cls == INTERIOR).sum()), int((cls == COLUMN_EDGE).sum()), int((cls == GENERAL).sum())) == (interior_n, edge_n, other_n)
    by_wave = cls.reshape(nstrips, 118)
    assert np.all(by_wave[:, 0] == GENERAL) and np.all(by_wave[:, 117] == GENERAL)
    assert np.all(by_wave[0, 1:117] == COLUMN_EDGE) and np.all(by_wave[-1, 1:117] == COLUMN_EDGE) and np.all(by_wave[1:-1, 1:117] == INTERIOR)
