"""-m gpu: two fused sweeps per launch on grids (cortex.jl_amd/csrc/cx_sweep_pair.hip).  A call of n sweeps runs floor((n - 1) / 2) paired
launches and then one or two plain sweeps; the arithmetic is that of the plain sweep, term by term, so every comparison here is bit for bit
on the float64 read-backs, NaN pattern included: against n calls of one sweep, and against the same call with CX_SWEEP_PAIRS=0."""
import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from tests.sweep_graphs import assert_same, everything, fused_device, grid_with_star, paired_launches, random_sparse

pytestmark = pytest.mark.gpu

ACCEPTED = [(2, 2), (3, 3), (5, 61), (5, 62), (5, 63), (5, 64), (7, 124), (9, 125), (20, 37), (24, 1415),
            (40, 2), (300, 3), (2, 300), (130, 70), (4, 248), (6, 249)]
# 40 x 2: no lane with a left AND a right neighbour, below more than two rows; 300 x 3: many segments in one column of workgroups, three of
# its four waves returning at once, rows in the slices 0 .. 3; 2 x 300, 130 x 70, 4 x 248: two columns of workgroups (4 x 248: four full
# strips, exactly one); 6 x 249: the last column of workgroups holds one strip of one column
NS = (3, 4, 5, 8)


@pytest.mark.parametrize("shape", ACCEPTED, ids=lambda s: "%dx%d" % s)
def test_pairs_equal_single_sweeps_and_the_switch(hip_lib, monkeypatch, shape):
    model = cx.synth.gaussian_grid(*shape, seed=7)
    for n in NS:
        monkeypatch.delenv("CX_SWEEP_PAIRS", raising=False)
        a, b = fused_device(model), fused_device(model)
        a.sweep(n)
        for _ in range(n):
            b.sweep(1)
        monkeypatch.setenv("CX_SWEEP_PAIRS", "0")
        c = fused_device(model)
        c.sweep(n)
        monkeypatch.delenv("CX_SWEEP_PAIRS", raising=False)
        assert paired_launches(a) == (n - 1) // 2 and paired_launches(b) == 0 and paired_launches(c) == 0
        assert a.stats()["sweeps_done"] == b.stats()["sweeps_done"] == c.stats()["sweeps_done"] == n
        assert a.sweep_stats()["sweeps_without_marginals"] == c.sweep_stats()["sweeps_without_marginals"] == n - 1
        ra = everything(a, model)
        assert np.all(np.isfinite(ra[0])), "a seeded grid: every message defined"
        assert_same(ra, everything(b, model), f"{shape}: sweep({n}) against {n} x sweep(1)")
        assert_same(ra, everything(c, model), f"{shape}: sweep({n}) against CX_SWEEP_PAIRS=0")
        for d in (a, b, c):
            d.close()


ROWS_CASES = [(s, r) for s in ((20, 37), (9, 125)) for r in (1, 3, 7, 64)] + [(s, r) for s in ((300, 3), (6, 249)) for r in (1, 7)]


@pytest.mark.parametrize("shape,rows", ROWS_CASES, ids=lambda x: "%dx%d" % x if isinstance(x, tuple) else str(x))
def test_any_rows_per_segment(hip_lib, monkeypatch, shape, rows):
    """CX_PAIR_ROWS: segments of one row (every row a halo row of two waves), odd lengths with a short last segment, one segment;
    300 x 3: 300 and 43 workgroups in the one column, 6 x 249: the one-column strip alone in its workgroups"""
    model = cx.synth.gaussian_grid(*shape, seed=11)
    monkeypatch.setenv("CX_PAIR_ROWS", str(rows))
    a, b = fused_device(model), fused_device(model)
    a.sweep(8)
    for _ in range(8):
        b.sweep(1)
    assert paired_launches(a) == 3
    assert_same(everything(a, model), everything(b, model), f"{shape}, {rows} rows per segment")


def test_two_consecutive_calls(hip_lib):
    model = cx.synth.gaussian_grid(20, 37, seed=7)
    a, b = fused_device(model), fused_device(model)
    a.sweep(5)
    a.sweep(4)
    for _ in range(9):
        b.sweep(1)
    assert paired_launches(a) == 2 + 1
    assert a.stats()["sweeps_done"] == 9
    assert_same(everything(a, model), everything(b, model), "sweep(5) then sweep(4) against 9 x sweep(1)")


@pytest.mark.parametrize("name", ["star", "row", "random", "every_sweep_marginals", "damped"])
def test_refused_graphs_and_handles_sweep_plain(hip_lib, monkeypatch, name):
    model = {"star": grid_with_star, "row": lambda: cx.synth.gaussian_grid(1, 300, seed=7), "random": random_sparse}.get(
        name, lambda: cx.synth.gaussian_grid(20, 37, seed=7))()
    if name == "every_sweep_marginals":
        monkeypatch.setenv("CX_MARG_EVERY_SWEEP", "1")
    a, b = fused_device(model, 50.0), fused_device(model, 50.0)
    if name == "damped":
        a.set_damping(0.25); b.set_damping(0.25)
    a.sweep(5)
    for _ in range(5):
        b.sweep(1)
    assert paired_launches(a) == 0
    assert_same(everything(a, model), everything(b, model), name)


def test_observed_variable_turns_pairs_off(hip_lib):
    """point-mass data on one variable after pairs have run: the variable is observed from then on, which no pair handles"""
    model = cx.synth.gaussian_grid(20, 37, seed=7)
    a, b = fused_device(model), fused_device(model)
    v = np.array([1 + 4 * 37 + 9], dtype=np.int64)
    f = model.edge_fac[np.flatnonzero(model.edge_var == v[0])[1:2]]      # one of its pairwise factors
    a.sweep(5)
    for _ in range(5):
        b.sweep(1)
    assert paired_launches(a) == 2
    for d in (a, b):
        d.set_messages(v, f, L.TO_FACTOR, L.FORM_POINT, np.array([0.3]))
    a.sweep(5)
    for _ in range(5):
        b.sweep(1)
    assert paired_launches(a) == 2
    assert_same(everything(a, model), everything(b, model), "after an observation")


def test_unseeded_grid_runs_plain_until_defined(hip_lib):
    """no seed: definedness spreads from nothing (every message depends on an undefined one), so the messages stay undefined, the
    check fails in the first eligible call and the grid sweeps plain"""
    model = cx.synth.gaussian_grid(5, 7, seed=7)
    a, b = fused_device(model, None), fused_device(model, None)
    a.sweep(5)
    for _ in range(5):
        b.sweep(1)
    assert paired_launches(a) == 0
    ra = everything(a, model)
    assert np.isnan(ra[0]).any()
    assert_same(ra, everything(b, model), "unseeded 5 x 7")
    # seeded now: the next call checks again (a seed is a change), finds every message defined and pairs
    for d in (a, b):
        d.seed_messages(L.TO_VARIABLE, 0.0, 1e6)
    a.sweep(5)
    for _ in range(5):
        b.sweep(1)
    assert paired_launches(a) == 2
    assert_same(everything(a, model), everything(b, model), "seeded afterwards")


def test_set_messages_makes_the_check_due_again(hip_lib):
    """an undefined message set into a defined grid: the call after it must look again and sweep plain (a pair cannot keep the older value of
    a slot as a plain sweep does); sixteen sweeps later the handle looks once more, finds every message defined and pairs again"""
    model = cx.synth.gaussian_grid(9, 125, seed=7)
    a, b = fused_device(model), fused_device(model)
    v = np.array([1 + 3 * 125 + 60], dtype=np.int64)
    f = model.edge_fac[np.flatnonzero(model.edge_var == v[0])[2:3]]      # a pairwise factor of variable (3, 60)
    nan = np.array([[np.nan, np.nan]])

    def both(n):
        a.sweep(n)
        for _ in range(n):
            b.sweep(1)

    both(5)
    assert paired_launches(a) == 2
    for d in (a, b):
        d.set_messages(v, f, L.TO_VARIABLE, L.FORM_NATURAL, nan)
    both(5)
    assert paired_launches(a) == 2, "the input held an undefined message: no pair in this call"
    assert_same(everything(a, model), everything(b, model), "after an undefined message was set")
    both(5)                      # 15 sweeps done: not looked at yet
    assert paired_launches(a) == 2
    both(6)                      # 21 sweeps done
    both(5)                      # looked at again: defined by now
    assert paired_launches(a) == 4
    assert_same(everything(a, model), everything(b, model), "pairs again")
