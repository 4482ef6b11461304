"""-m gpu: the point-mass branch of the additive rule in the deep sweep (cortex.jl_amd/csrc/cx_sweep_deep.hip: deep_rule, one division
for both branches).  The other deep-sweep tests never reach it: their priors are finite, and an observed variable turns the paired path
off.  Here a handful of unary factor→variable messages are set, in natural form, to (x, +inf): a unary message is never rewritten, so
the variable→factor messages of those cells carry m.y == +inf at level 1 and at every deeper level of every launch, next to cells that
take the ordinary branch.  They sit in the grid's interior, on its first column, on its top row, in its last corner, and two of them side
by side (each is then the other's neighbour at a point mass).  Two more unary messages are set to (x, 0.0).  The library does not look at
the values of stored messages, so the deep path stays on (asserted).  One model has factor variances of 1e-12 and 1e12 mixed with the
usual ones, so that the one division sees denominators far from 1 in both branches.  Every comparison is bit for bit on all
factor→variable messages and all marginals, NaN pattern included, against the same call under CX_SWEEP_PAIRS=0."""
import dataclasses

import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from tests.sweep_graphs import GridIds, clean_env, read_back

pytestmark = pytest.mark.gpu

DEPTHS = (3, 4, 5, 6)
N = 17
SEED = 1e6
# (shape, CX_DEEP_ROWS or None for the chosen rows, extreme factor variances); 24 x 130 at 4 rows per segment: general, interior and column-edge waves
CASES = (((24, 130), 4, False), ((20, 37), None, False), ((20, 37), None, True))
IDS = ("24x130-rows4", "20x37", "20x37-extreme-q")


def point_masses(H, W):
    return ((H // 2, W // 2), (H // 3, 0), (0, W // 2 + 3), (H // 2 + 2, W - 7), (H // 2 + 2, W - 6), (H - 1, W - 1))


def zero_precisions(H, W):
    return ((H // 2 - 3, W // 3), (H - 2, 1))


_models, _plain = {}, {}


def model_of(shape, extreme):
    if (shape, extreme) not in _models:
        m = cx.synth.gaussian_grid(*shape, seed=7)
        if extreme:
            rng = np.random.default_rng(11)
            fv = m.factor_var.copy()
            pairwise = np.flatnonzero(m.factor_kind == L.FACTOR_GAUSS_ADDITIVE)
            fv[pairwise] *= rng.choice([1e-12, 1.0, 1e12], size=len(pairwise))
            m = dataclasses.replace(m, factor_var=fv)
        _models[(shape, extreme)] = m
    return _models[(shape, extreme)]


def _device(shape, extreme):
    H, W = shape
    ids = GridIds(H, W)
    dev = cx.DeviceGraph(schedule=L.SCHED_FUSED)
    cx.synth.load_into_device(model_of(shape, extreme), dev, SEED)
    pm, z = point_masses(H, W), zero_precisions(H, W)
    cells = pm + z
    payload = np.array([(0.25 * (k + 1) * (-1) ** k, np.inf) for k in range(len(pm))] + [(0.5, 0.0), (-1.5, 0.0)][:len(z)])
    dev.set_messages([ids.var(r, c) for r, c in cells], [ids.unary(r, c) for r, c in cells], L.TO_VARIABLE, L.FORM_NATURAL, payload)
    return dev


def plain(env, shape, extreme):
    """the read-back after sweep(N) under CX_SWEEP_PAIRS=0: once per model, shared by the four depths"""
    if (shape, extreme) not in _plain:
        env.setenv("CX_SWEEP_PAIRS", "0")
        c = _device(shape, extreme)
        c.sweep(N)
        env.delenv("CX_SWEEP_PAIRS")
        assert c.sweep_deep_launches() == (0,) * 7
        _plain[(shape, extreme)] = read_back(c, model_of(shape, extreme))
        c.close()
    return _plain[(shape, extreme)]


def test_the_cells_lie_in_the_grid_and_two_are_adjacent():
    for shape, _, _ in CASES:
        H, W = shape
        cells = point_masses(H, W) + zero_precisions(H, W)
        assert len(set(cells)) == len(cells) and all(0 <= r < H and 0 <= c < W for r, c in cells)
        pm = point_masses(H, W)
        assert pm[3][0] == pm[4][0] and pm[3][1] + 1 == pm[4][1]
        assert any(c == 0 for _, c in pm) and any(r == 0 for r, _ in pm) and any(0 < r < H - 1 and 0 < c < W - 1 for r, c in pm)


@pytest.mark.parametrize("case", CASES, ids=IDS)
@pytest.mark.parametrize("depth", DEPTHS)
def test_point_masses_as_the_plain_sweeps(hip_lib, clean_env, depth, case):
    shape, rows, extreme = case
    want = plain(clean_env, shape, extreme)
    clean_env.setenv("CX_SWEEP_DEPTH", str(depth))
    if rows:
        clean_env.setenv("CX_DEEP_ROWS", str(rows))
    a = _device(shape, extreme)
    a.sweep(N)
    ran = a.sweep_deep_launches()
    got = read_back(a, model_of(shape, extreme))
    a.close()
    assert ran[depth] == (N - 1) // depth and sum(d * k for d, k in enumerate(ran)) >= N - 2, f"the deep kernel ran: {ran}"
    # the branch was taken where it should be: a pairwise message sent by a cell at a point mass is (x / q, 1 / q), finite whatever came in
    model = model_of(shape, extreme)
    ids = GridIds(*shape)
    r, c = point_masses(*shape)[0]
    sent = np.flatnonzero((model.edge_var == ids.var(r, c + 1)) & (model.edge_fac == ids.factor(r, c, "right")))
    q = model.factor_var[model.factor_ids == ids.factor(r, c, "right")][0]
    assert len(sent) == 1 and got[0][sent[0], 1] == 1.0 / q, (got[0][sent[0]], q)
    for x, y, name in zip(got, want, ("messages to variables", "marginals")):
        differ = np.flatnonzero(~((x == y) | (np.isnan(x) & np.isnan(y))).all(axis=1))
        assert differ.size == 0, f"{shape}, depth {depth}, extreme q {extreme}: {name} differ at {differ.size} rows, first {differ[:5]}: {x[differ[:5]]} against {y[differ[:5]]}"
