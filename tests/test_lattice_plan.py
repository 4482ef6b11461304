"""The grid plan of the paired sweep (cortex.jl_amd/csrc/cx_lattice_plan.h) on the CPU build of the host logic: which graphs it accepts,
why it refuses the others, that every destination slot it computes is the partner table's, and that the (strip, segment) waves own every
variable exactly once whatever the rows per segment."""
import ctypes as C

import numpy as np
import pytest

import cortex.jl_amd as cx
from tests.hostlogic import FlatGraph, lib
from tests.sweep_graphs import grid_with_star, natural_form_sweeps, undefined_midcall_grid

ACCEPTED = [(2, 2), (3, 3), (5, 61), (5, 62), (5, 63), (5, 64), (7, 124), (9, 125), (20, 37), (24, 1415),
            (40, 2), (300, 3), (2, 300), (130, 70), (4, 248), (6, 249)]


def flat(model):
    g = FlatGraph(model.edge_var, model.edge_fac, model.factor_ids, model.factor_kind, model.factor_var, edge_role=model.edge_role)
    assert g.status == 0, g.error
    return g


def plan(g, rows=0, capacity=None):
    """(accepted, reason, {H, W, strips, block_cols}, dest [nv, 4], src [nv, 4], count [nv], rows chosen for `capacity` workgroups)"""
    lb = lib()
    lb.cxh_flat_lattice.restype = C.c_int32
    lb.cxh_flat_lattice.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_char_p, C.c_int32]
    nv = g.scalar("nv")
    hw = np.zeros(4, dtype=np.int64)
    dest, src = np.full((nv, 4), -7, dtype=np.int32), np.full((nv, 4), -7, dtype=np.int32)
    count = np.full(nv, -7, dtype=np.int32)
    cap = C.c_int64(capacity or 0)
    reason = C.create_string_buffer(256)
    ok = lb.cxh_flat_lattice(g.p, rows, hw.ctypes.data, dest.ctypes.data, src.ctypes.data, count.ctypes.data if rows else None,
                             C.byref(cap) if capacity else None, reason, 256)
    return bool(ok), reason.value.decode(), dict(zip(("H", "W", "strips", "block_cols"), map(int, hw))), dest, src, count, int(cap.value)


@pytest.mark.parametrize("shape", ACCEPTED, ids=lambda s: "%dx%d" % s)
def test_accepted_grid_destinations_are_the_partner_table(shape):
    H, W = shape
    g = flat(cx.synth.gaussian_grid(H, W, seed=7))
    ok, reason, hw, dest, src, _, _ = plan(g)
    assert ok, reason
    assert reason == ""
    assert (hw["H"], hw["W"]) == (H, W)
    assert hw["strips"] == -(-W // 62) and hw["block_cols"] == -(-hw["strips"] // 4)
    partner, slice_off, vinfo = g.arr("partner"), g.arr("slice_off"), g.arr("vinfo")
    # the sending slots, worked out here from the layout alone: rank 0 unary, then left, right, up, down with absent directions skipped
    v = np.arange(H * W)
    r, c = v // W, v % W
    has = np.stack([c > 0, c < W - 1, r > 0, r < H - 1], axis=1)
    rank = 1 + np.cumsum(has, axis=1) - has
    base = slice_off[v >> 8] + (v & 255)
    want_src = np.where(has, base[:, None] + rank * 256, -1)
    assert np.array_equal(src, want_src)
    assert np.array_equal((vinfo & 15), 1 + has.sum(axis=1))
    assert np.all(partner[base] == -1), "rank 0 is the unary slot"
    # every computed destination is what the partner table says
    assert np.array_equal(dest[has], partner[want_src[has]])
    assert np.all(dest[~has] == -1)
    # ... and together they are every slot with a partner, once
    assert np.array_equal(np.sort(dest[has]), np.flatnonzero(partner >= 0))


@pytest.mark.parametrize("shape", ACCEPTED, ids=lambda s: "%dx%d" % s)
def test_owners_cover_every_variable_once(shape):
    H, W = shape
    g = flat(cx.synth.gaussian_grid(H, W, seed=7))
    for rows in (1, 2, 4, 7, H, H + 3, 64):
        ok, reason, _, _, _, count, _ = plan(g, rows=rows)
        assert ok, reason
        assert np.all(count == 1), f"{H}x{W}, {rows} rows per segment: owners per variable {np.unique(count)}"


def test_rows_per_segment_fill_the_device_once():
    g = flat(cx.synth.gaussian_grid(24, 1415, seed=7))      # 23 strips: 6 columns of workgroups
    for capacity, want in ((1024, 4), (36, 4), (12, 12), (6, 24), (1, 24)):      # 170 / 6 / 2 / 1 / 1 segments fit: rows clamped to 4 .. 64
        *_, rows = plan(g, capacity=capacity)
        assert rows == want, (capacity, rows)
    g = flat(cx.synth.gaussian_grid(300, 3, seed=7))        # one strip, one column of workgroups: every workgroup a segment
    for capacity, want in ((1024, 4), (75, 4), (50, 6), (10, 30), (4, 64), (1, 64)):     # 300 rows over 1024 / 75 / 50 / 10 segments; above 64 rows: more than one round
        *_, rows = plan(g, capacity=capacity)
        assert rows == want, (capacity, rows)


def _permuted_ranks():
    """the 6 x 9 grid with the factor ids of the vertical factors BELOW those of the horizontal ones: up / down come before left / right"""
    m = cx.synth.gaussian_grid(6, 9, seed=7)
    V, Hf = 6 * 9, 6 * 8
    ids = m.factor_ids.copy()
    horiz = (ids > 2 * V) & (ids <= 2 * V + Hf)
    vert = ids > 2 * V + Hf
    nvert = int(vert.sum())
    remap = {int(f): int(f) + nvert for f in ids[horiz]}
    remap.update({int(f): int(f) - Hf for f in ids[vert]})
    f = lambda a: np.array([remap.get(int(x), int(x)) for x in a], dtype=np.int64)
    return cx.synth.Model(edge_var=m.edge_var, edge_fac=f(m.edge_fac), factor_ids=f(m.factor_ids), factor_kind=m.factor_kind, factor_var=m.factor_var,
                          x_ids=m.x_ids, prior_var=m.prior_var, prior_fac=m.prior_fac, prior_mean=m.prior_mean, prior_variance=m.prior_variance)


def _missing_prior():
    m = cx.synth.gaussian_grid(6, 9, seed=7)
    gone = 9 * 6 + (1 + 3 * 9 + 4)      # the unary factor of variable (3, 4)
    ke, kf = m.edge_fac != gone, m.factor_ids != gone
    return cx.synth.Model(edge_var=m.edge_var[ke], edge_fac=m.edge_fac[ke], factor_ids=m.factor_ids[kf], factor_kind=m.factor_kind[kf],
                          factor_var=m.factor_var[kf], x_ids=m.x_ids, prior_var=m.prior_var, prior_fac=m.prior_fac, prior_mean=m.prior_mean,
                          prior_variance=m.prior_variance)


def test_refusals_name_their_reason():
    def refused(g, word):
        ok, reason, *_ = plan(g)
        assert not ok
        assert word in reason, reason

    refused(flat(cx.synth.ssm_chain(300, seed=3)), "not a grid")
    g = flat(cx.synth.gaussian_grid(6, 9, seed=7))
    assert plan(g)[0]
    g.clamp([1 + 2 * 9 + 5])
    refused(g, "observed")
    refused(flat(_missing_prior()), "without the unary message")
    refused(flat(_permuted_ranks()), "not in the order")
    refused(flat(grid_with_star()), "big degree")
    refused(flat(cx.synth.gaussian_grid(40, 12, seed=7, row0=8, row1=20)), "not a grid")      # a row block with its stand-in rows of degree 1


def test_the_grid_that_goes_undefined_in_the_middle_of_a_call():
    """tests/sweep_graphs.py: undefined_midcall_grid, which tests/test_gpu_grid_between_calls.py sweeps in pairs.  The plan takes it (a factor
    variance of 0.5 is a variance like any other) and every input is defined; in float64 numpy, natural form, plain sweeps: sweep 1 stores
    one message of precision -inf (1 + q w = 0), sweep 2 three undefined ones, sweep 3 reads eight undefined variable→factor messages —
    the second launch of a paired call — and, keeping the older values, leaves every message defined again"""
    model, sv, sf, payload = undefined_midcall_grid()
    ok, reason, hw, *_ = plan(flat(model))
    assert ok, reason
    assert (hw["H"], hw["W"]) == (4, 5)
    assert np.all(np.isfinite(payload)) and payload[0, 1] == -2.0
    assert natural_form_sweeps(model, 1e6, sv, sf, payload, 5) == [(1, 0, 0), (0, 3, 0), (0, 0, 8), (0, 0, 0), (0, 0, 0)]
