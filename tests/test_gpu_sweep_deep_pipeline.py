"""-m gpu: the row pipeline of the deep sweep (cortex.jl_amd/csrc/cx_sweep_deep.hip) where its two instances and its loop can go wrong: every
length of the row loop around the pipeline's depth, launches in which edge and interior waves (cx_lattice_deep.h: strip_interior,
segment_interior) work side by side, the seam between two strips on the lanes that a whole-wave shift fills differently from a shuffle, an
undefined message met by an interior wave, and two calls in a row.  Every case sweeps one handle deep and one under CX_SWEEP_PAIRS=0 the
same number of sweeps and wants all marginals and all factor→variable messages (natural form, float64) identical, NaN pattern included."""
import dataclasses

import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from tests.sweep_graphs import GridIds, clean_env, fused_device, launches, model_of, natural_form_sweeps, read_back

pytestmark = pytest.mark.gpu

DEPTHS = (3, 4)
SEED = 1e6
STRIP_COLS = {3: 60, 4: 58}

_plain = {}


def greedy(n, depth):
    """the launches of one call of n >= 16 sweeps at `depth`, as (pairs, depth 3, depth 4): launches of the depth while that many of the
    n - 1 sweeps before the last remain, then one launch of the remainder's depth (a remainder of one is a plain sweep)"""
    count = {2: 0, 3: 0, 4: 0}
    rem = n - 1
    while rem >= 2:
        d = min(depth, rem)
        count[d] += 1
        rem -= d
    return count[2], count[3], count[4]


def plain(monkeypatch, shape, calls):
    """the read-back of a handle swept under CX_SWEEP_PAIRS=0, once per grid and sequence of calls"""
    if (shape, calls) not in _plain:
        monkeypatch.setenv("CX_SWEEP_PAIRS", "0")
        model = model_of(shape)
        dev = fused_device(model)
        for n in calls:
            dev.sweep(n)
        assert launches(dev) == (0, 0, 0)
        _plain[(shape, calls)] = read_back(dev, model)
        dev.close()
        monkeypatch.delenv("CX_SWEEP_PAIRS")
    return _plain[(shape, calls)]


def _check(monkeypatch, shape, depth, rows, calls):
    want = plain(monkeypatch, shape, calls)
    what = f"{shape}, depth {depth}, rows {rows or 'chosen'}, calls {calls}"
    monkeypatch.setenv("CX_SWEEP_DEPTH", str(depth))
    if rows:
        monkeypatch.setenv("CX_DEEP_ROWS", str(rows))
    model = model_of(shape)
    dev = fused_device(model)
    for n in calls:
        dev.sweep(n)
    expect = tuple(sum(x) for x in zip(*(greedy(n, depth) for n in calls)))
    assert launches(dev) == expect and expect[depth - 2] > 0, (what, launches(dev), expect)
    d = dev.sweep_deep_stats()
    assert d["depth"] == depth and (d["rows"] == rows if rows else d["rows"] >= 4 * (depth - 1)), (what, d)
    got = read_back(dev, model)
    dev.close()
    if rows:
        monkeypatch.delenv("CX_DEEP_ROWS")
    assert np.all(np.isfinite(got[0])), f"{what}: a seeded grid, every message defined"
    for x, y, name in zip(got, want, ("messages to variables", "marginals")):
        assert np.array_equal(x, y, equal_nan=True), f"{what}: {name} differ from CX_SWEEP_PAIRS=0"


def interior_waves(H, W, K, R):
    """[strips, segments] of bool, from the formulas alone: lane l of strip s holds column s (64 - 2 (K - 1)) - (K - 1) + l, the wave of
    segment [r0, r1) loads rows r0 - (K - 1) .. r1 + (K - 1) - 1; interior: all of them have four neighbours in the grid"""
    cols = STRIP_COLS[K]
    out = np.zeros((-(-W // cols), -(-H // R)), dtype=bool)
    for s in range(out.shape[0]):
        for g in range(out.shape[1]):
            r0, r1 = g * R, min(g * R + R, H)
            out[s, g] = s * cols - (K - 1) >= 1 and s * cols - (K - 1) + 63 <= W - 2 and r0 - (K - 1) >= 1 and r1 + (K - 1) - 1 <= H - 2
    return out


@pytest.mark.parametrize("height", (23, 7))
@pytest.mark.parametrize("depth", DEPTHS)
def test_every_length_of_the_row_loop(hip_lib, clean_env, depth, height):
    """CX_DEEP_ROWS = 1 .. 12: the loop runs R + 2 (K - 1) rows, fewer at the grid's ends and in a short last segment: every residue modulo
    the pipeline's periods (K, K + 1, 2), and segments shorter than the pipeline is deep"""
    for rows in range(1, 13):
        for n in (16, 19):
            _check(clean_env, (height, 130), depth, rows, (n,))


@pytest.mark.parametrize("height", (40, 5))
@pytest.mark.parametrize("depth", DEPTHS)
def test_edge_and_interior_waves_in_one_launch(hip_lib, clean_env, depth, height):
    """one, two and three or more strips; with 40 rows in segments of 8 the first, the middle and the last segments and, from the third
    width on, edge and interior strips occur in one launch; 5 rows have no interior segment"""
    widths = {4: (40, 100, 130, 180), 3: (40, 100, 125, 185)}[depth]
    some = [bool(interior_waves(height, W, depth, 8).any()) for W in widths]
    assert some == ([False, False, True, True] if height == 40 else [False] * 4)
    if height == 40:
        w = interior_waves(40, widths[3], depth, 8)
        assert w.shape == (4, 5) and w[1:3, 1:4].all() and not w[0].any() and not w[3].any() and not w[:, 0].any() and not w[:, 4].any()
    for W in widths:
        _check(clean_env, (height, W), depth, 8, (17,))


@pytest.mark.parametrize("depth", DEPTHS)
def test_the_seam_between_two_strips(hip_lib, clean_env, depth):
    """W = two strips and 0, 1, 2 columns: the last owned column of strip 0 and the first of strip 1 are each other's neighbours, and what
    crosses the seam at the levels below K comes through the halo lanes, up to lanes 0 and 63, which a whole-wave shift fills with zero where
    a shuffle left the lane's own value: nothing stored may depend on either"""
    for extra in (0, 1, 2):
        for rows in (None, 8):
            _check(clean_env, (20, 2 * STRIP_COLS[depth] + extra), depth, rows, (17,))


@pytest.mark.parametrize("depth", DEPTHS)
def test_two_consecutive_calls(hip_lib, clean_env, depth):
    """nothing of a launch's pipeline (which register holds which age) survives into the next launch or the next call"""
    assert interior_waves(40, 180, depth, 4 * (depth - 1)).any()
    _check(clean_env, (40, 180), depth, None, (17, 17))


# ---- an undefined message met by an interior wave: the recipe of tests/sweep_graphs.py: undefined_midcall_grid at the centre of 24 x 180 ----
UNDEF_SHAPE, UNDEF_SENDER, UNDEF_ROWS = (24, 180), (12, 90), 6


def _undefined_model():
    H, W = UNDEF_SHAPE
    r, c = UNDEF_SENDER
    ids = GridIds(H, W)
    m = model_of(UNDEF_SHAPE)
    fv = m.factor_var.copy()
    fv[m.factor_ids == ids.factor(r, c, "right")] = 0.5
    model = dataclasses.replace(m, factor_var=fv)
    pv, pf = ids.pairwise_edges(r, c)
    set_vars = np.concatenate([[ids.var(r, c)], pv]).astype(np.int64)
    set_facs = np.concatenate([[ids.unary(r, c)], pf]).astype(np.int64)
    payload = np.zeros((len(set_vars), 2))
    payload[0] = (0.0, -2.0)
    return model, set_vars, set_facs, payload


def _load_undefined():
    model, sv, sf, payload = _undefined_model()
    dev = fused_device(model)
    dev.set_messages(sv, sf, L.TO_VARIABLE, L.FORM_NATURAL, payload)
    return model, dev


def test_when_the_message_turns_undefined():
    """float64 numpy on the CPU: every input defined; sweep 1 sends (nan, -inf), sweep 2 stores nan precisions, sweep 3 is the first that
    reads an undefined variable→factor message — level 3 of the first deep launch of a call of 17 sweeps at either depth.  The receiver
    (12, 91) and its neighbours lie in strip 1 and, at 6 rows per segment, in segments 1 and 2 (rows 6 .. 17): interior waves all"""
    model, sv, sf, payload = _undefined_model()
    per_sweep = natural_form_sweeps(model, SEED, sv, sf, payload, 3)
    assert per_sweep == [(1, 0, 0), (0, 3, 0), (0, 0, 9)], per_sweep      # (three neighbours of the receiver with three other edges each)
    for depth in DEPTHS:
        assert greedy(17, depth)[depth - 2] >= 1 and depth >= 3
        w = interior_waves(*UNDEF_SHAPE, depth, UNDEF_ROWS)
        cols = STRIP_COLS[depth]
        assert (UNDEF_SENDER[1] + 1) // cols == 1 and (UNDEF_SENDER[1] + 1) % cols >= depth and (UNDEF_SENDER[1] + 1) % cols < cols - depth
        assert w[1, 1] and w[1, 2] and UNDEF_SENDER[0] // UNDEF_ROWS == 2


@pytest.mark.parametrize("depth", DEPTHS)
def test_an_undefined_message_met_by_an_interior_wave_is_reported_once(hip_lib, clean_env, depth):
    clean_env.setenv("CX_SWEEP_DEPTH", str(depth))
    clean_env.setenv("CX_DEEP_ROWS", str(UNDEF_ROWS))
    model, a = _load_undefined()
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
    a.close()
    # under CX_SWEEP_PAIRS=0 the plain sweeps carry on: one call or seventeen
    clean_env.setenv("CX_SWEEP_PAIRS", "0")
    _, c = _load_undefined()
    _, b = _load_undefined()
    c.sweep(17)
    c.sync()
    for _ in range(17):
        b.sweep(1)
    assert launches(c) == (0, 0, 0) and launches(b) == (0, 0, 0)
    for x, y in zip(read_back(c, model), read_back(b, model)):
        assert np.array_equal(x, y, equal_nan=True)
    c.close(); b.close()
