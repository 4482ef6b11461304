"""-m gpu: three or four fused sweeps per launch on grids (cortex.jl_amd/csrc/cx_sweep_deep.hip), in calls of at least 16 sweeps.  The n - 1
sweeps before the last are decomposed greedily (launches of the depth while that many sweeps remain, one launch of the remainder's depth, a
plain sweep for a remainder of one); the arithmetic of every level is the plain sweep's, term by term, so every comparison here is bit for
bit on the float64 read-backs, NaN pattern included: against n calls of one sweep, and against the same call with CX_SWEEP_PAIRS=0."""
import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from tests.sweep_graphs import assert_same, clean_env, everything, fused_device, grid_with_star, launches, load_undefined_midcall, model_of, random_sparse

pytestmark = pytest.mark.gpu

DEPTHS = (3, 4)
NS = (16, 17, 18, 19)      # (n - 1) mod 3 = 0, 1, 2, 0 and (n - 1) mod 4 = 3, 0, 1, 2
# widths around the strip (60 / 58 owned columns) and workgroup-column (four strips) boundaries of each depth
WIDTHS = {3: (59, 60, 61, 120, 121, 240, 241), 4: (57, 58, 59, 116, 117, 232, 233)}
# grids smaller than the pipeline (fewer rows or columns than levels, one lane with both neighbours or none); C4's own width
SMALL = [(2, 2), (3, 3), (2, 300), (40, 2), (300, 3), (24, 1415)]
ROWS_CASES = [(s, r) for s in ((20, 37), (9, 125)) for r in (1, 2, 3, 7, 64)]


def greedy(n, depth):
    """the launches of one call of n sweeps at `depth`, as (pairs, depth 3, depth 4)"""
    count = {2: 0, 3: 0, 4: 0}
    rem = n - 1
    if n < 16:
        depth = 2
    while rem >= 2:
        d = min(depth, rem)
        count[d] += 1
        rem -= d
    return count[2], count[3], count[4]


def test_the_decomposition_this_file_expects():
    assert [greedy(n, 3) for n in NS] == [(0, 5, 0), (0, 5, 0), (1, 5, 0), (0, 6, 0)]
    assert [greedy(n, 4) for n in NS] == [(0, 1, 3), (0, 0, 4), (0, 0, 4), (1, 0, 4)]
    assert greedy(8, 4) == (3, 0, 0) and greedy(17, 2) == (8, 0, 0)


_singles = {}


def singles(shape, seed=7):
    """the read-backs after n = 16 .. 19 calls of sweep(1), computed once per grid and shared by every depth and rows case"""
    if (shape, seed) not in _singles:
        model = model_of(shape, seed)
        b = fused_device(model)
        out = {}
        for n in range(1, max(NS) + 1):
            b.sweep(1)
            if n in NS:
                out[n] = everything(b, model)
        assert launches(b) == (0, 0, 0)
        b.close()
        _singles[(shape, seed)] = out
    return _singles[(shape, seed)]


def _check_shape(monkeypatch, shape, depth, rows=None, seed=7):
    model, ref = model_of(shape, seed), singles(shape, seed)
    for n in NS:
        what = f"{shape}, depth {depth}, rows {rows or 'chosen'}: sweep({n})"
        monkeypatch.setenv("CX_SWEEP_DEPTH", str(depth))
        if rows:
            monkeypatch.setenv("CX_DEEP_ROWS", str(rows))
        a = fused_device(model)
        a.sweep(n)
        monkeypatch.setenv("CX_SWEEP_PAIRS", "0")
        c = fused_device(model)
        c.sweep(n)
        monkeypatch.delenv("CX_SWEEP_PAIRS")
        assert launches(a) == greedy(n, depth), what
        assert launches(c) == (0, 0, 0), what
        d = a.sweep_deep_stats()
        assert d["depth"] == depth and (d["rows"] == rows if rows else d["rows"] >= 4 * (depth - 1)), (what, d)
        assert a.stats()["sweeps_done"] == c.stats()["sweeps_done"] == n, what
        assert a.sweep_stats()["sweeps_without_marginals"] == c.sweep_stats()["sweeps_without_marginals"] == n - 1, what
        ra = everything(a, model)
        assert np.all(np.isfinite(ra[0])), "a seeded grid: every message defined"
        assert_same(ra, ref[n], f"{what} against {n} x sweep(1)")
        assert_same(ra, everything(c, model), f"{what} against CX_SWEEP_PAIRS=0")
        a.close(); c.close()


@pytest.mark.parametrize("height", (5, 20))
@pytest.mark.parametrize("depth", DEPTHS)
def test_widths_around_strip_and_workgroup_column_boundaries(hip_lib, clean_env, depth, height):
    for W in WIDTHS[depth]:
        _check_shape(clean_env, (height, W), depth)


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("depth", DEPTHS)
def test_grids_smaller_than_the_pipeline_and_the_flagship_width(hip_lib, clean_env, depth, shape):
    _check_shape(clean_env, shape, depth)


@pytest.mark.parametrize("shape,rows", ROWS_CASES, ids=lambda x: "%dx%d" % x if isinstance(x, tuple) else str(x))
@pytest.mark.parametrize("depth", DEPTHS)
def test_any_rows_per_segment(hip_lib, clean_env, depth, shape, rows):
    """CX_DEEP_ROWS: segments shorter than the halo (every row a halo row of several waves), a short last segment, one segment"""
    _check_shape(clean_env, shape, depth, rows=rows, seed=11)


@pytest.mark.parametrize("depth", DEPTHS)
def test_two_consecutive_calls(hip_lib, clean_env, depth):
    model = model_of((20, 37))
    clean_env.setenv("CX_SWEEP_DEPTH", str(depth))
    a, b = fused_device(model), fused_device(model)
    a.sweep(17)
    a.sweep(16)
    for _ in range(33):
        b.sweep(1)
    assert launches(a) == tuple(x + y for x, y in zip(greedy(17, depth), greedy(16, depth)))
    assert a.stats()["sweeps_done"] == 33
    assert_same(everything(a, model), everything(b, model), "sweep(17) then sweep(16) against 33 x sweep(1)")
    a.close(); b.close()


def test_a_short_call_runs_pairs_only(hip_lib, clean_env):
    model = model_of((20, 37))
    a, b = fused_device(model), fused_device(model)
    a.sweep(8)
    for _ in range(8):
        b.sweep(1)
    assert launches(a) == (3, 0, 0)
    assert a.sweep_deep_stats()["depth"] == 2
    assert_same(everything(a, model), everything(b, model), "sweep(8), no depth forced")
    a.close(); b.close()


@pytest.mark.parametrize("name", ["star", "row", "random", "every_sweep_marginals", "damped"])
@pytest.mark.parametrize("depth", DEPTHS)
def test_refused_graphs_and_handles_sweep_plain(hip_lib, clean_env, depth, name):
    model = {"star": grid_with_star, "row": lambda: cx.synth.gaussian_grid(1, 300, seed=7), "random": random_sparse}.get(
        name, lambda: cx.synth.gaussian_grid(20, 37, seed=7))()
    clean_env.setenv("CX_SWEEP_DEPTH", str(depth))
    if name == "every_sweep_marginals":
        clean_env.setenv("CX_MARG_EVERY_SWEEP", "1")
    a, b = fused_device(model, 50.0), fused_device(model, 50.0)
    if name == "damped":
        a.set_damping(0.25); b.set_damping(0.25)
    a.sweep(17)
    for _ in range(17):
        b.sweep(1)
    assert launches(a) == (0, 0, 0)
    assert_same(everything(a, model), everything(b, model), name)
    a.close(); b.close()


@pytest.mark.parametrize("depth", DEPTHS)
def test_a_deep_launch_that_meets_an_undefined_message_is_reported_once(hip_lib, clean_env, depth):
    """tests/sweep_graphs.py: undefined_midcall_grid — every input defined, so the check lets the call start; sweep 1 divides by 1 + q w = 0,
    sweep 2 stores undefined messages and sweep 3 — level 3 of the first launch — reads them: the NaN path, no fault.  The word is found by
    whichever checked call comes first once the launch has run, and the later launches of the call, which raise it again, are not reported."""
    clean_env.setenv("CX_SWEEP_DEPTH", str(depth))
    model, a = load_undefined_midcall()
    errors = []
    for call in (lambda: a.sweep(17), a.sync, a.sync, lambda: a.get_marginals(model.x_ids), a.sync):
        try:
            call()
        except cx.CortexHipError as e:
            errors.append(e)
    assert len(errors) == 1, [str(e) for e in errors]
    assert errors[0].code == L.ERR_DEVICE and "CX_SWEEP_PAIRS=0" in str(errors[0]) and "undefined" in str(errors[0])
    assert a.stats()["sweeps_done"] == 17
    ran = launches(a)
    assert ran == greedy(17, depth)
    a.sweep(17)
    a.sync()
    assert launches(a) == ran, "the handle sweeps plain from then on"
    assert a.stats()["sweeps_done"] == 34
    a.close()
    # plain sweeps keep the older value of a slot whose input is undefined: the same inputs run to completion, one call or seventeen
    clean_env.setenv("CX_SWEEP_PAIRS", "0")
    _, c = load_undefined_midcall()
    _, b = load_undefined_midcall()
    c.sweep(17)
    c.sync()
    for _ in range(17):
        b.sweep(1)
    assert launches(c) == (0, 0, 0) and launches(b) == (0, 0, 0)
    assert_same(everything(c, model), everything(b, model), "CX_SWEEP_PAIRS=0: sweep(17) against 17 x sweep(1)")
    c.close(); b.close()
