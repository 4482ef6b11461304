"""The geometry of the deep sweep (cortex.jl_amd/csrc/cx_lattice_deep.h: K sweeps per launch on the grid plan) on the CPU build of the host
logic, for K = 2, 3, 4: the waves own every variable exactly once; a cell valid at level j has itself and every in-grid neighbour valid at
level j - 1, down to level 1; nothing outside what the wave loads is ever valid; every stored cell is valid at level K; and the rows per
segment chosen for a capacity respect their floor and ceiling.  The predicates are the ones the kernel compiles."""
import ctypes as C

import numpy as np
import pytest

import cortex.jl_amd as cx
from tests.hostlogic import FlatGraph, lib

DEPTHS = (2, 3, 4)
# the shapes of tests/test_gpu_sweep_deep.py: widths around the strip and workgroup-column boundaries of depth 3 (60 columns a strip) and
# depth 4 (58), grids smaller than the pipeline, C4's own width
WIDTHS = (57, 58, 59, 60, 61, 116, 117, 120, 121, 232, 233, 240, 241)
SHAPES = [(h, w) for h in (5, 20) for w in WIDTHS] + [(2, 2), (3, 3), (2, 300), (40, 2), (300, 3), (24, 1415)]
ROWS_SHAPES = [(20, 37), (9, 125)]
ROWS = (1, 2, 3, 7, 64)
C4_ROWS = {2: 9, 3: 12, 4: 13}      # what the device's occupancy gives on 1415 x 1415 (profiles/deep_sweep.md)

_graphs = {}


def flat(shape):
    if shape not in _graphs:
        m = cx.synth.gaussian_grid(*shape, seed=7)
        g = FlatGraph(m.edge_var, m.edge_fac, m.factor_ids, m.factor_kind, m.factor_var, edge_role=m.edge_role)
        assert g.status == 0, g.error
        _graphs[shape] = g
    return _graphs[shape]


def deep(g, K, rows, capacity=None, levels=True):
    """({strip_cols, strips, block_cols, segments, min_rows, max_rows}, count [nv], rows chosen for `capacity`, wave [n, 3] = strip, r0, r1,
    level [n, rows + 2 K + 2, 66], owned likewise) — the window of a wave starts at row r0 - K - 1 and lane -1"""
    lb = lib()
    fn = lb.cxh_flat_lattice_deep
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p]
    geom = np.zeros(6, dtype=np.int64)
    count = np.full(g.scalar("nv"), -7, dtype=np.int32)
    cap = C.c_int64(capacity or 0)
    n = fn(g.p, K, rows, geom.ctypes.data, count.ctypes.data if levels else None, C.byref(cap) if capacity else None, None, None, None)
    assert n > 0, n
    gd = dict(zip(("strip_cols", "strips", "block_cols", "segments", "min_rows", "max_rows"), map(int, geom)))
    if not levels:
        return gd, count, int(cap.value), None, None, None
    win = rows + 2 * K + 2
    wave = np.zeros((n, 3), dtype=np.int32)
    level, owned = np.full((n, win, 66), -7, dtype=np.int8), np.full((n, win, 66), -7, dtype=np.int8)
    assert fn(g.p, K, rows, None, None, None, wave.ctypes.data, level.ctypes.data, owned.ctypes.data) == n
    return gd, count, int(cap.value), wave, level, owned


def check(shape, K, rows):
    H, W = shape
    gd, count, _, wave, level, owned = deep(flat(shape), K, rows)
    what = f"{H}x{W}, depth {K}, {rows} rows per segment"
    assert gd["strip_cols"] == 64 - 2 * (K - 1) and gd["strips"] == -(-W // gd["strip_cols"]) and gd["block_cols"] == -(-gd["strips"] // 4), what
    assert gd["segments"] == -(-H // rows) and len(wave) == gd["strips"] * gd["segments"], what
    assert np.all(count == 1), f"{what}: owners per variable {np.unique(count)}"
    # grid coordinates of every window cell, worked out here: lane -1 of strip s is column s * strip_cols - (K - 1) - 1
    win = level.shape[1]
    r = wave[:, 1, None, None] - K - 1 + np.arange(win)[None, :, None]
    c = wave[:, 0, None, None] * gd["strip_cols"] - (K - 1) - 1 + np.arange(66)[None, None, :] + 0 * r
    r = r + 0 * c
    lane = np.arange(-1, 65)[None, None, :] + 0 * r
    in_grid = (r >= 0) & (r < H) & (c >= 0) & (c < W)
    # what the wave loads: rows r0 - (K - 1) .. r1 + (K - 1) - 1 of the grid at lanes 0 .. 63
    loaded = in_grid & (lane >= 0) & (lane <= 63) & (r >= wave[:, 1, None, None] - (K - 1)) & (r <= wave[:, 2, None, None] + (K - 1) - 1)
    assert np.all((level >= 0) & (level <= K)) and set(np.unique(owned)) <= {0, 1}, what
    assert not np.any((level >= 1) & ~loaded), f"{what}: a cell the wave does not load is marked valid"
    # (the window has a margin of one row and one lane beyond anything that can be valid: the shifted views below never wrap a valid cell)
    assert not level[:, 0].any() and not level[:, -1].any() and not level[:, :, 0].any() and not level[:, :, -1].any(), what
    for j in range(2, K + 1):
        v, below = level >= j, level >= j - 1
        assert not np.any(v & ~below), f"{what}: level {j} without level {j - 1}"
        for dr, dc in ((0, -1), (0, 1), (-1, 0), (1, 0)):
            nb_in_grid = (r + dr >= 0) & (r + dr < H) & (c + dc >= 0) & (c + dc < W)
            nb_below = np.roll(below, (-dr, -dc), axis=(1, 2))
            assert not np.any(v & nb_in_grid & ~nb_below), f"{what}: a cell valid at level {j} has a neighbour ({dr}, {dc}) not valid at level {j - 1}"
    stored = owned == 1
    assert np.all(level[stored] == K), f"{what}: a stored cell is not valid at level {K}"
    assert np.all(in_grid[stored]) and stored.sum() == H * W, what
    # the stored cells are the segment's rows at the owned lanes
    assert np.all((r[stored] >= (wave[:, 1, None, None] + 0 * r)[stored]) & (r[stored] < (wave[:, 2, None, None] + 0 * r)[stored])), what
    assert np.all((lane[stored] >= K - 1) & (lane[stored] <= 64 - K)), what


@pytest.mark.parametrize("K", DEPTHS)
def test_levels_and_owners_on_the_gpu_tests_shapes(K):
    for shape in SHAPES:
        check(shape, K, 4 * (K - 1))       # what choose_rows gives a grid this small: its floor
    for shape in ROWS_SHAPES:
        for rows in ROWS:
            check(shape, K, rows)


@pytest.mark.parametrize("K", DEPTHS)
def test_levels_and_owners_on_the_flagship_grid(K):
    check((1415, 1415), K, C4_ROWS[K])


@pytest.mark.parametrize("K", DEPTHS)
def test_rows_per_segment_respect_floor_and_ceiling(K):
    for shape in [(24, 1415), (300, 3), (5, 59)]:
        g = flat(shape)
        gd, *_ = deep(g, K, 1, levels=False)
        assert gd["min_rows"] == 4 * (K - 1) and gd["max_rows"] == 64
        for capacity in (1, 4, 7, 36, 75, 512, 768, 1024, 100000):
            _, _, rows, *_ = deep(g, K, 1, capacity=capacity, levels=False)
            assert gd["min_rows"] <= rows <= gd["max_rows"], (shape, K, capacity, rows)
            # between floor and ceiling: the fewest rows at which every workgroup of the launch is resident at once
            seg_max = max(1, capacity // gd["block_cols"])
            assert rows == min(64, max(gd["min_rows"], -(-shape[0] // seg_max))), (shape, K, capacity, rows)
    # the flagship grid at the occupancies of the resource report: 4, 3 and 3 waves per SIMD of 256 compute units
    for K_, capacity, want in ((2, 1024, 9), (3, 768, 12), (4, 768, 13), (4, 512, 20)):
        if K_ == K:
            assert deep(flat((1415, 1415)), K, 1, capacity=capacity, levels=False)[2] == want
