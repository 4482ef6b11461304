"""The geometry of the deep sweep (cortex.jl_amd/csrc/cx_lattice_deep.h) at K = 5 and 6, five and six sweeps per launch, on the CPU build of
the host logic, through the exports and the checks the tests of K = 2 .. 4 use: every variable is stored by exactly one wave and the validity
rule holds level by level (tests/test_lattice_deep.py: check); wave_class says what the general predicates find, cell by cell
(tests/test_lattice_deep_classes.py); the packed map is a bijection onto the working waves for last workgroup columns of 1, 2 and 3 strips
(tests/test_lattice_deep_packed.py); and the rows per segment that the flagship grid gets at two and at three waves per SIMD."""
import ctypes as C

import numpy as np
import pytest

from tests.hostlogic import lib
from tests.test_lattice_deep import check
from tests.test_lattice_deep_classes import COLUMN_EDGE, GENERAL, INTERIOR, _by_hand, classes
from tests.test_lattice_deep_packed import packed

DEPTHS = (5, 6)
HEIGHTS = (2, 20)
ROWS_SHAPES = [(20, 37), (9, 125)]
ROWS = (1, 2, 3, 7, 64)


def strip_cols(K):
    return 64 - 2 * (K - 1)


def widths(K):
    """the widths of tests/test_gpu_sweep_deep_56.py: fewer columns than levels, around one strip and around four (a workgroup column)"""
    c = strip_cols(K)
    return (2, K, 2 * K - 1, c - 1, c, c + 1, 4 * c - 1, 4 * c, 4 * c + 1)


def test_lanes_0_and_63_are_valid_at_level_1_only_and_never_owned():
    """lane_valid_at_level: j - 1 <= lane <= 64 - j; lane_owned: K - 1 <= lane <= 64 - K.  By the window of cxh_flat_lattice_deep, whose lane
    axis starts at -1: lanes 0 and 63 are columns 1 and 64 of it"""
    from tests.test_lattice_deep import deep, flat
    for K in DEPTHS:
        c = strip_cols(K)
        _, _, _, wave, level, owned = deep(flat((20, 4 * c + 1)), K, 4)
        assert level[:, :, (1, 64)].max() == 1 and not owned[:, :, (1, 64)].any(), K
        assert strip_cols(K) == 64 - 2 * (K - 1) and np.all(owned.sum(axis=2) <= c)


@pytest.mark.parametrize("K", DEPTHS)
def test_levels_and_owners(K):
    for H in HEIGHTS + (K - 1, 2 * (K - 1) + 1):
        for W in widths(K):
            check((H, W), K, 4 * (K - 1))
            check((H, W), K, 3)
    for shape in ROWS_SHAPES:
        for rows in ROWS:
            check(shape, K, rows)
    check((24, 130), K, 4)


@pytest.mark.parametrize("K,rows", [(5, 19), (6, 20)])
def test_levels_and_owners_on_the_flagship_grid(K, rows):
    check((1415, 1415), K, rows)


@pytest.mark.parametrize("K", DEPTHS)
def test_wave_class_agrees_with_the_general_predicates(K):
    buffers = tuple(np.empty(4096, dtype=np.int8) for _ in range(3))
    said = {GENERAL: 0, INTERIOR: 0, COLUMN_EDGE: 0}
    c = strip_cols(K)
    for W in sorted(set(range(1, 3 * c + 4)) | set(widths(K))):
        for H in (1, 2, K - 1, 2 * K - 1, 2 * K, 20, 24, 40):
            for R in (1, 2, 3, 4, 7, 4 * (K - 1), 24):
                what = f"depth {K}, {H} x {W}, {R} rows per segment"
                cls, rows_ok, cols_ok = classes(K, W, H, R, buffers)
                assert np.array_equal(cls == INTERIOR, (rows_ok == 1) & (cols_ok == 1)), what
                assert np.array_equal(cls == COLUMN_EDGE, (rows_ok == 1) & (cols_ok == 0)), what
                assert np.array_equal(cls == GENERAL, rows_ok == 0), what
                assert np.array_equal(cls, _by_hand(K, W, H, R)), what
                for k in said:
                    said[k] += int((cls == k).sum())
    assert all(v > 0 for v in said.values()), said


@pytest.mark.parametrize("K", DEPTHS)
def test_all_three_instances_on_24_x_130_at_4_rows_per_segment(K):
    """the grid of the GPU test: three strips (54 / 52 owned columns: strip 1 holds columns 50 .. 113 / 47 .. 110, inside 1 .. 128), six
    segments; segment g touches rows 4 g - (K - 1) .. 4 g + 4 + (K - 1) - 1: within 1 .. 22 for g = 2, 3 at depth 5 (rows 4 .. 15, 8 .. 19;
    g = 1 starts at row 0) and for g = 2, 3 at depth 6 (rows 3 .. 16, 7 .. 20; g = 1 starts at -1, g = 4 ends at 24)"""
    G, I, E = GENERAL, INTERIOR, COLUMN_EDGE
    assert classes(K, 130, 24, 4)[0].reshape(3, 6).tolist() == [[G, G, E, E, G, G], [G, G, I, I, G, G], [G, G, E, E, G, G]]


@pytest.mark.parametrize("K", DEPTHS)
def test_the_packed_map_is_a_bijection_onto_the_working_waves(K):
    c = strip_cols(K)
    for s, W in ((1, 4 * c + 1), (2, 5 * c + 1), (3, 6 * c + 1), (0, 4 * c), (1, 2), (3, 3 * c)):
        strips = -(-W // c)
        assert strips % 4 == s, (K, W)
        for nseg in (1, 2, 3, 4, 5, 7, 10, 71, 75):
            what = f"depth {K}, W {W} ({strips} strips), {nseg} segments"
            count, waves = packed(K, W, nseg)
            idle = (waves[:, :, 0] == -1) & (waves[:, :, 1] == -1)
            work = waves[~idle]
            assert np.all((work[:, 0] >= 0) & (work[:, 0] < strips)) and np.all((work[:, 1] >= 0) & (work[:, 1] < nseg)), what
            seen = np.zeros((strips, nseg), dtype=np.int64)
            np.add.at(seen, (work[:, 0], work[:, 1]), 1)
            assert np.all(seen == 1), f"{what}: waves per (strip, segment) {np.unique(seen)}"
            assert np.array_equal(np.flatnonzero((~idle).any(axis=1)), np.arange(count)), what
            full = strips // 4
            assert count == full * nseg + (-(-nseg // (4 // s)) if s else 0), what
            # a packed workgroup holds floor(4 / s) consecutive segments of the last column's s strips
            for slab in range(full * nseg, count):
                w = waves[slab][~idle[slab]]
                assert np.all(w[:, 0] >= 4 * full) and np.array_equal(w[:, 1], np.sort(w[:, 1])) and w[:, 1].max() - w[:, 1].min() < 4 // s, what


def test_the_flagship_strips_and_workgroups():
    """1415 columns: 26 strips of 54 at depth 5 (a last column of 2 strips, two segments a workgroup), 27 of 52 at depth 6 (3 strips, one
    segment a workgroup: nothing gained by packing); 75 and 71 segments at the chosen rows"""
    assert packed(5, 1415, 75)[0] == 6 * 75 + 38 == 488 and packed(5, 1415, 79)[0] == 6 * 79 + 40 == 514
    assert packed(6, 1415, 71)[0] == 7 * 71 == 497 and packed(6, 1415, 75)[0] == 7 * 75 == 525


def test_rows_chosen_for_the_flagship_grid():
    """two waves per SIMD of 256 compute units hold 512 workgroups of four waves, three hold 768.  Depth 5: 18 rows are 79 segments and 514
    workgroups, 19 rows 75 and 488.  Depth 6 starts at its floor of 20 rows: 71 segments, 497 workgroups.  Depth 4 at 768: 12, as before"""
    fn = lib().cxh_lattice_deep_rows_packed
    fn.restype = C.c_int32
    fn.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int64]
    assert fn(5, 1415, 1415, 512) == 19
    assert fn(6, 1415, 1415, 512) == 20
    assert fn(4, 1415, 1415, 768) == 12
    assert fn(7, 1415, 1415, 512) == -1 and fn(1, 1415, 1415, 512) == -1      # (depths the kernel is not built at)
    for K in DEPTHS:
        for H, W in [(1415, 1415), (24, 1415), (300, 3), (4000, 233)]:
            for capacity in (1, 7, 36, 512, 768, 100000):
                want = next((R for R in range(4 * (K - 1), 64) if packed(K, W, -(-H // R), extra=0)[0] <= capacity), 64)
                assert fn(K, H, W, capacity) == want, (K, H, W, capacity)
