"""The packed map of the deep sweep (cortex.jl_amd/csrc/cx_lattice_deep.h: packed_wave, packed_blocks) on the CPU build of the host logic, for
K = 3, 4: a last workgroup column of s < 4 strips puts floor(4 / s) consecutive segments into one workgroup.  Every (strip, segment) is run
by exactly one (workgroup, wave), no wave gets a strip or a segment that does not exist, and the workgroup count that the launch uses is
the number of workgroups that hold a wave.  And the rows per segment chosen under that map (choose_rows_packed)."""
import ctypes as C

import numpy as np
import pytest

from tests.hostlogic import lib

DEPTHS = (3, 4)
# (H, rows per segment): 1 segment; 7 and 9 (odd); 10 (even, no multiple of 4); 4; the flagship's 109 and 118
SEGMENT_CASES = [(5, 8), (20, 3), (9, 1), (20, 2), (20, 5), (1415, 13), (1415, 12)]


def widths(K):
    """4, 5 and 6 strips plus one column (a last workgroup column of 1, 2 and 3 strips), exactly 4 strips, less than one strip, the flagship"""
    sc = 64 - 2 * (K - 1)
    return (4 * sc + 1, 5 * sc + 1, 6 * sc + 1, 4 * sc, 57, 1415)


def packed(K, W, nseg, extra=3):
    """(workgroup count, [count + extra, 4, 2] = strip, segment of every wave; -1, -1 for a wave without work)"""
    fn = lib().cxh_lattice_deep_packed
    fn.restype = C.c_int32
    fn.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    count = fn(K, W, nseg, 0, None)
    assert count > 0, count
    out = np.full((count + extra, 4, 2), -7, dtype=np.int32)
    assert fn(K, W, nseg, count + extra, out.ctypes.data) == count
    return count, out


@pytest.mark.parametrize("K", DEPTHS)
def test_every_strip_and_segment_has_one_wave(K):
    sc = 64 - 2 * (K - 1)
    for W in widths(K):
        strips = -(-W // sc)
        for H, R in SEGMENT_CASES:
            nseg = -(-H // R)
            what = f"depth {K}, W {W} ({strips} strips), {nseg} segments"
            count, waves = packed(K, W, nseg)
            idle = (waves[:, :, 0] == -1) & (waves[:, :, 1] == -1)
            work = waves[~idle]
            assert np.all((work[:, 0] >= 0) & (work[:, 0] < strips)), f"{what}: a strip at or beyond W"
            assert np.all(work[:, 0] * sc < W), what
            assert np.all((work[:, 1] >= 0) & (work[:, 1] < nseg)), f"{what}: a segment at or beyond the count"
            seen = np.zeros((strips, nseg), dtype=np.int64)
            np.add.at(seen, (work[:, 0], work[:, 1]), 1)
            assert np.all(seen == 1), f"{what}: waves per (strip, segment) {np.unique(seen)}"
            holds = np.flatnonzero((~idle).any(axis=1))
            assert len(holds) == count and np.array_equal(holds, np.arange(count)), f"{what}: {count} workgroups launched, {len(holds)} hold a wave"
            # full columns are not packed; a last column of s strips holds ceil(nseg / floor(4 / s)) workgroups
            full, s = divmod(strips, 4)
            assert count == full * nseg + (-(-nseg // (4 // s)) if s else 0), what


@pytest.mark.parametrize("K", DEPTHS)
def test_the_flagship_counts(K):
    """1415 columns: 25 strips at depth 4 (a seventh column of one strip, four segments a workgroup), 24 at depth 3 (nothing to pack)"""
    want = {(4, 109): 6 * 109 + 28, (4, 118): 6 * 118 + 30, (3, 118): 6 * 118, (3, 109): 6 * 109}
    for nseg in (109, 118):
        assert packed(K, 1415, nseg)[0] == want[(K, nseg)]


@pytest.mark.parametrize("K", DEPTHS)
def test_rows_per_segment_under_the_packed_map(K):
    """the fewest rows, not below 4 (K - 1) and not above 64, at which the packed launch is resident; worked out here from the count"""
    fn = lib().cxh_lattice_deep_rows_packed
    fn.restype = C.c_int32
    fn.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int64]
    for H, W in [(1415, 1415), (24, 1415), (300, 3), (5, 59), (4000, 233), (100000, 117)]:
        for capacity in (1, 7, 36, 512, 768, 1024, 100000):
            want = next((R for R in range(4 * (K - 1), 64) if packed(K, W, -(-H // R), extra=0)[0] <= capacity), 64)
            assert fn(K, H, W, capacity) == want, (K, H, W, capacity)
    # the flagship grid at three waves per SIMD of 256 compute units: depth 4 gains a row on the unpacked rule's 13, depth 3 keeps its 12
    assert fn(4, 1415, 1415, 768) == 12 and fn(3, 1415, 1415, 768) == 12
