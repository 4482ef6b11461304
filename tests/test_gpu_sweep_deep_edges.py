"""-m gpu: the column-edge instance of the deep sweep (cortex.jl_amd/csrc/cx_sweep_deep.hip; cx_lattice_deep.h: wave_class, column_edge): a wave
whose rows are interior and whose strip holds the grid's first or last column tests no row, forms everything that depends on the lane once
in front of its row loop and loads every row without a branch, each direction from its own rank.  The shapes put the grid's left and right
edge into one wave (grids narrower than a strip), the right edge on the first owned lane of a strip, on its last, and into a packed
workgroup beside a general wave; heights of 20 and 40 rows, because at 4 (K - 1) rows per segment 20 rows have no row-interior segment.
Every comparison is bit for bit against a handle that swept the same sweeps under CX_SWEEP_PAIRS=0."""
import dataclasses

import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from tests.sweep_graphs import GridIds, clean_env, fused_device, launches, model_of, read_back, rows_cases
from tests.test_gpu_sweep_deep import greedy
from tests.test_lattice_deep_classes import COLUMN_EDGE, GENERAL, classes

pytestmark = pytest.mark.gpu

DEPTHS = (3, 4)
HEIGHTS = (20, 40)
N = 17


def widths(K):
    sc = 64 - 2 * (K - 1)
    return (2, 3, 57, sc, sc + 1, 2 * sc, 4 * sc + 1, 5 * sc + 1)


_plain = {}


def plain(monkeypatch, shape, calls=(N,)):
    """(messages to variables, marginals) after the calls under CX_SWEEP_PAIRS=0: computed once per grid, shared by every depth and rows case"""
    if (shape, calls) not in _plain:
        monkeypatch.setenv("CX_SWEEP_PAIRS", "0")
        c = fused_device(model_of(shape))
        for n in calls:
            c.sweep(n)
        monkeypatch.delenv("CX_SWEEP_PAIRS")
        assert launches(c) == (0, 0, 0), shape
        _plain[(shape, calls)] = read_back(c, model_of(shape))
        c.close()
    return _plain[(shape, calls)]


def column_edge_waves(depth, shape, rows):
    """[strips, segments] of bool from the host logic: the waves that take the column-edge instance"""
    H, W = shape
    cls = classes(depth, W, H, rows)[0]
    return (cls == COLUMN_EDGE).reshape(-(-W // (64 - 2 * (depth - 1))), -(-H // rows))


@pytest.mark.parametrize("height", HEIGHTS)
@pytest.mark.parametrize("depth", DEPTHS)
def test_column_edge_waves_leave_every_bit_as_it_was(hip_lib, clean_env, depth, height):
    clean_env.setenv("CX_SWEEP_DEPTH", str(depth))
    sc = 64 - 2 * (depth - 1)
    for W in widths(depth):
        shape = (height, W)
        model, want = model_of(shape), plain(clean_env, shape)
        for rows in rows_cases(depth):
            what = f"{shape}, depth {depth}, {rows} rows per segment: sweep({N})"
            edge = column_edge_waves(depth, shape, rows)
            if (depth, height, rows) == (4, 20, 12):      # segments 0 .. 11 and 12 .. 19 touch rows -3 .. 14 and 9 .. 22: none is row-interior
                assert not edge.any() and np.all(classes(depth, W, height, rows)[0] == GENERAL), what
            else:
                assert edge[0].any() and edge[-1].any(), f"{what}: a column-edge wave in the first and in the last strip"
            if W == 4 * sc + 1 and rows == 3 and height == 40:      # the packed workgroup of segments 0 .. 3 of strip 4 mixes general and column-edge waves
                assert edge.shape[0] == 5 and not edge[4, 0] and edge[4, 3], what
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
    """sweep(16) then sweep(17) on (40, 4 sc + 1) at the chosen rows per segment: the second call's first launch reads what column-edge waves,
    those of the packed workgroups included, stored in the first"""
    sc = 64 - 2 * (depth - 1)
    shape = (40, 4 * sc + 1)
    model, want = model_of(shape), plain(clean_env, shape, (16, 17))
    clean_env.setenv("CX_SWEEP_DEPTH", str(depth))
    a = fused_device(model)
    a.sweep(16)
    a.sweep(17)
    assert launches(a) == tuple(x + y for x, y in zip(greedy(16, depth), greedy(17, depth)))
    edge = column_edge_waves(depth, shape, a.sweep_deep_stats()["rows"])
    assert edge[0].any() and edge[-1].any()
    assert a.stats()["sweeps_done"] == 33
    for x, y, name in zip(read_back(a, model), want, ("messages to variables", "marginals")):
        assert np.array_equal(x, y, equal_nan=True), f"depth {depth}: {name} differ from CX_SWEEP_PAIRS=0"
    a.close()


# ---- an undefined message born on the grid's first and last column, in a row-interior segment: the recipe of tests/sweep_graphs.py:
# undefined_midcall_grid with the sender moved to (12, 0) and (12, W - 1) of 24 x 130 at 6 rows per segment ----
UNDEF_SHAPE, UNDEF_ROW, UNDEF_ROWS = (24, 130), 12, 6


def _undefined_model(col):
    """the factor between the sender and its one horizontal neighbour has variance 0.5; the sender's unary message is (0, -2) in natural form
    and its neighbours send zeros: in sweep 1 the factor divides by 1 + q w = 0"""
    H, W = UNDEF_SHAPE
    ids = GridIds(H, W)
    m = model_of(UNDEF_SHAPE)
    fv = m.factor_var.copy()
    fv[m.factor_ids == ids.factor(UNDEF_ROW, col, "right" if col == 0 else "left")] = 0.5
    model = dataclasses.replace(m, factor_var=fv)
    pv, pf = ids.pairwise_edges(UNDEF_ROW, col)
    assert len(pv) == 3
    set_vars = np.concatenate([[ids.var(UNDEF_ROW, col)], pv]).astype(np.int64)
    set_facs = np.concatenate([[ids.unary(UNDEF_ROW, col)], pf]).astype(np.int64)
    payload = np.zeros((len(set_vars), 2))
    payload[0] = (0.0, -2.0)
    return model, set_vars, set_facs, payload


@pytest.mark.parametrize("side", ("first", "last"))
@pytest.mark.parametrize("depth", DEPTHS)
def test_an_undefined_message_born_on_an_edge_column_is_reported_once(hip_lib, clean_env, depth, side):
    H, W = UNDEF_SHAPE
    col = 0 if side == "first" else W - 1
    edge = column_edge_waves(depth, UNDEF_SHAPE, UNDEF_ROWS)
    strip = col // (64 - 2 * (depth - 1))
    assert strip == (0 if side == "first" else edge.shape[0] - 1)
    assert edge[strip, 1] and edge[strip, 2] and UNDEF_ROW // UNDEF_ROWS == 2, "the sender, the receiver and its neighbours lie in column-edge waves"
    clean_env.setenv("CX_SWEEP_DEPTH", str(depth))
    clean_env.setenv("CX_DEEP_ROWS", str(UNDEF_ROWS))
    model, sv, sf, payload = _undefined_model(col)
    a = fused_device(model)
    a.set_messages(sv, sf, L.TO_VARIABLE, L.FORM_NATURAL, payload)
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
