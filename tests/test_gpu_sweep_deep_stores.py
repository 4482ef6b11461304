"""-m gpu: the deep sweep's stores under its packed map (cortex.jl_amd/csrc/cx_sweep_deep.hip, cx_lattice_deep.h: packed_wave).  A last
workgroup column of fewer than four strips puts several segments into one workgroup.  The shapes here put lanes that must not store on
both sides of a strip boundary, make grids narrower than one strip, leave iterations without a level-K row at both ends of a segment (rows
per segment of 1, 3 and the floor 4 (K - 1)), and give packed workgroups a last wave without a segment.  Every comparison is bit for bit
against a handle that swept the same sweeps under CX_SWEEP_PAIRS=0.  (The file was written for a variant that issued level K's stores in
every iteration, with an offset beyond the buffer where nothing is stored; that variant was not faster and is not in, see
profiles/deep_sweep_stores.md.  The shapes are what such a change has to pass.)"""
import numpy as np
import pytest

from tests.sweep_graphs import clean_env, fused_device, launches, model_of, read_back, rows_cases
from tests.test_gpu_sweep_deep import greedy

pytestmark = pytest.mark.gpu

DEPTHS = (3, 4)
HEIGHTS = (5, 9, 20)
N = 17


def widths(K):
    """4, 5 and 6 strips plus one column (a last workgroup column of 1, 2 and 3 strips), exactly 4 strips, less than a strip, 2 and 3 columns"""
    sc = 64 - 2 * (K - 1)
    return (4 * sc + 1, 5 * sc + 1, 6 * sc + 1, 4 * sc, 57, 2, 3)


_plain = {}


def plain(monkeypatch, shape):
    """(messages to variables, marginals) after sweep(17) under CX_SWEEP_PAIRS=0: computed once per grid, shared by every depth and rows case"""
    if shape not in _plain:
        monkeypatch.setenv("CX_SWEEP_PAIRS", "0")
        c = fused_device(model_of(shape))
        c.sweep(N)
        monkeypatch.delenv("CX_SWEEP_PAIRS")
        assert launches(c) == (0, 0, 0), shape
        _plain[shape] = read_back(c, model_of(shape))
        c.close()
    return _plain[shape]


@pytest.mark.parametrize("height", HEIGHTS)
@pytest.mark.parametrize("depth", DEPTHS)
def test_strip_edges_and_packed_columns_leave_every_bit_as_it_was(hip_lib, clean_env, depth, height):
    clean_env.setenv("CX_SWEEP_DEPTH", str(depth))
    for W in widths(depth):
        shape = (height, W)
        model, want = model_of(shape), plain(clean_env, shape)
        for rows in rows_cases(depth):
            what = f"{shape}, depth {depth}, {rows} rows per segment: sweep({N})"
            clean_env.setenv("CX_DEEP_ROWS", str(rows))
            a = fused_device(model)
            a.sweep(N)
            assert launches(a) == greedy(N, depth), what
            d = a.sweep_deep_stats()
            assert d["depth"] == depth and d["rows"] == rows, (what, d)
            got = read_back(a, model)
            a.close()
            assert np.all(np.isfinite(got[0])), f"{what}: a seeded grid, every message defined"
            for x, y, name in zip(got, want, ("messages to variables", "marginals")):
                assert np.array_equal(x, y, equal_nan=True), f"{what}: {name} differ from CX_SWEEP_PAIRS=0"


@pytest.mark.parametrize("depth", DEPTHS)
def test_a_second_call_starts_from_what_the_first_call_stored(hip_lib, clean_env, depth):
    """sweep(16) then sweep(17) on one handle, marginals in the last sweep of a call only: the second call's first launch reads buffers that
    the first call's last launches stored, packed workgroups included"""
    sc = 64 - 2 * (depth - 1)
    model = model_of((20, 4 * sc + 1))
    clean_env.setenv("CX_SWEEP_DEPTH", str(depth))
    a = fused_device(model)
    a.sweep(16)
    a.sweep(17)
    clean_env.setenv("CX_SWEEP_PAIRS", "0")
    c = fused_device(model)
    c.sweep(16)
    c.sweep(17)
    assert launches(a) == tuple(x + y for x, y in zip(greedy(16, depth), greedy(17, depth)))
    assert launches(c) == (0, 0, 0)
    assert a.stats()["sweeps_done"] == c.stats()["sweeps_done"] == 33
    for x, y, name in zip(read_back(a, model), read_back(c, model), ("messages to variables", "marginals")):
        assert np.array_equal(x, y, equal_nan=True), f"depth {depth}: {name} differ from CX_SWEEP_PAIRS=0"
    a.close(); c.close()
