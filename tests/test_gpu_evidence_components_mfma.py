"""-m gpu: cx_log_evidence_components_mfma — the log-evidence of every connected component of one handle at the matrix-core dims
(cx_create dim 5 .. 64) — against the dense joint of each component alone (tests/evidence_support.py) on the graphs of
tests/components_mfma_support.py (pinned by tests/test_components_mfma_checker.py); learn.profile and learn.multi_start_em at d = 16."""
import ctypes as C
import math

import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from cortex.jl_amd import learn
from tests import components_mfma_support as M
from tests import components_support as CS
from tests import evidence_mfma_support as S
from tests import evidence_support as E
from tests import missing_data as MD
from tests.gpu_support import assert_reader_refusals, demo_chain, run_demo

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.asarray(a, dtype=np.float64).tobytes()


def _dev(model, schedule, sweeps=1, opaque=None):
    dev = cx.DeviceGraph(dim=model.dim, schedule=schedule)
    cx.synth.load_into_device(model, dev, seed_variance=1e6 if schedule == L.SCHED_FUSED else None)
    if opaque is not None:
        S.set_opaque(dev, opaque)
    dev.sweep(sweeps)
    return dev


def _calls(dev, what):
    """on one handle: the sum against log_evidence_mfma, repeatability, cap, and log_evidence_mfma untouched.  Returns (values, comp_counts)"""
    before, cnt = dev.log_evidence_mfma()
    values, cc, counts = dev.log_evidence_components_mfma()
    again, cc2, _ = dev.log_evidence_components_mfma()
    assert _bits(values) == _bits(again) and (cc == cc2).all(), what
    two, cc_two, counts_two = dev.log_evidence_components_mfma(cap=2)
    assert len(two) == min(2, len(values)) and _bits(two) == _bits(values[:2]) and (cc_two == cc[:2]).all() and counts_two == counts, what
    after, cnt_after = dev.log_evidence_mfma()
    assert _bits(before) == _bits(after) and cnt == cnt_after, what
    assert counts == cnt and [int(x) for x in cc.sum(axis=0)] == list(cnt.values()), (what, counts, cnt, cc.sum(axis=0))
    if np.isfinite(values).all():
        gap, scale = abs(math.fsum(values.tolist()) - before), float(np.abs(values).sum())
        print(f"{what}: |fsum(values) - log_evidence_mfma| = {gap:.3e}, sum |values| = {scale:.6e}, relative {gap / scale:.3e}")
        assert gap <= 1e-12 * scale, (what, gap, scale)
    return values, cc


# ---- 1: exact per component, every tile size, native and embedded ----------------------------------------------------------------------
@pytest.mark.parametrize("d", M.DIMS)
def test_chains_exact_per_component(hip_lib, d):
    parts, model, wants = M.chains(d)
    ids, lab, n = CS.labels(model)
    assert n == len(parts)
    for schedule, sweeps in ((L.SCHED_CHAIN_SCAN, 1), (L.SCHED_TREE, 1), (L.SCHED_REFERENCE, 1), (L.SCHED_FUSED, 2 * max(M.LENGTHS) + 40)):
        dev = _dev(model, schedule, sweeps)
        got_lab, got_n = dev.components()
        assert got_n == n and (got_lab == lab).all()
        values, cc = _calls(dev, f"d {d} schedule {schedule}")
        assert cc[:, 2:].sum() == 0
        for k, want in enumerate(wants):
            print(f"d {d} schedule {schedule} component {k}: got {values[k]!r} want {want!r}")
            assert abs(want) >= 1
            assert abs(values[k] - want) <= 1e-9 * abs(want), (d, schedule, k, values[k], want)
        assert [int(x) for x in cc[:, 0]] == [2 * T - 1 for T in M.LENGTHS]
        dev.close()


# ---- 2: trees, relabelled ids ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [5, 17])
def test_forest_as_built_and_relabelled(hip_lib, d):
    model = M.forest(d)
    for m in (model, CS.relabel(model, np.random.default_rng(31))):
        gm = E.gmodel(m)
        lab, n = CS.gm_labels(gm)
        assert n == 3 and (lab == CS.labels(m)[1]).all()
        dev = _dev(m, L.SCHED_TREE)
        got_lab, got_n = dev.components()
        assert got_n == n and (got_lab == lab).all()
        values, cc = _calls(dev, f"forest d {d}")
        assert cc[:, 2:].sum() == 0
        for k in range(n):
            want = E.dense_log_z(CS.restrict(gm, k, lab))
            assert abs(want) >= 1
            assert abs(values[k] - want) <= 1e-9 * abs(want), (d, k, values[k], want)
        assert cc[:, 0].sum() == sum(len(g["fid"]) for g in gm.groups.values())
        dev.close()


# ---- 3: segments against tile borders ----------------------------------------------------------------------------------------------------
def test_segments_against_tile_borders(hip_lib):
    model, opq, comp_of_part, wants, n = M.borders()
    dev = _dev(model, L.SCHED_TREE, 1, opaque=opq)
    assert dev.components()[1] == n
    values, cc = _calls(dev, "tile borders")
    assert cc[:, 2:].sum() == 0
    for part, (k, want) in enumerate(zip(comp_of_part[:-1], wants[:-1])):
        assert abs(values[k] - want) <= 1e-9 * abs(want), (part, k, values[k], want)
    lone = values[comp_of_part[-1]]
    print(f"the lone variable: value {lone!r} (exact 0; dense reference {wants[-1]!r})")
    assert abs(lone) <= 1e-12
    assert list(cc[comp_of_part[-1]]) == [0, 1, 0, 0] and list(cc[comp_of_part[0]][:2]) == [2 * M.LONG - 1, M.LONG]
    dev.close()


# ---- 4: loopy ----------------------------------------------------------------------------------------------------------------------------
def test_two_rings_match_the_restatement(hip_lib):
    d = 16
    assert d in S.RING_DIMS
    model = M.rings(d)
    gm = E.gmodel(model)
    lab, n = CS.gm_labels(gm)
    assert n == 2
    dev = _dev(model, L.SCHED_FUSED, S.RING_SWEEPS)
    values, cc = _calls(dev, "two rings")
    f2v, opq = E.device_messages(gm, dev)
    for k in range(n):
        fk, ok = CS.restrict_messages(gm, f2v, opq, k, lab)
        want = E.bethe_log_z(CS.restrict(gm, k, lab), fk, ok)
        print(f"ring {k}: got {values[k]!r} bethe {want!r}")
        assert abs(values[k] - want) <= 1e-10 * abs(want), (k, values[k], want)
    dev.close()


# ---- 5: isolation, in bits ---------------------------------------------------------------------------------------------------------------
def test_an_undefined_component_leaves_the_others_alone(hip_lib):
    parts, model, _ = M.chains(16)
    dev = _dev(model, L.SCHED_TREE)
    clean, _, _ = dev.log_evidence_components_mfma()
    dev.close()
    assert np.isfinite(clean).all()
    broken = list(parts)
    broken[1] = MD.tail(parts[1], 3)                      # a forecast tail on the T = 3 chain; its end message is left unset
    dev = _dev(cx.synth.concat_models(broken), L.SCHED_TREE)
    values, cc, counts = dev.log_evidence_components_mfma()
    assert np.isnan(values[1]) and cc[1, 2] > 0, (values, cc)
    for k in (0, 2):
        assert _bits(values[k]) == _bits(clean[k]) and cc[k, 2] == 0 and cc[k, 3] == 0, (k, values[k], clean[k])
    total, cnt = dev.log_evidence_mfma()
    assert np.isnan(total) and cnt == counts and cnt["undefined"] == cc[1, 2]
    dev.close()


# ---- 6: refusals and arguments -----------------------------------------------------------------------------------------------------------
class _Out:
    """output arrays of the raw call, filled with marks: a refused call leaves them as they are"""

    def __init__(self, n=3):
        self.val, self.cc = np.full(n, 7.25), np.full((n, 4), -5, np.int64)
        self.nc, self.out = C.c_int64(-9), (C.c_int64 * 4)(-1, -2, -3, -4)
        self.pv, self.pc = self.val.ctypes.data_as(C.POINTER(C.c_double)), self.cc.ctypes.data_as(C.POINTER(C.c_int64))

    def untouched(self):
        return (self.val == 7.25).all() and (self.cc == -5).all() and self.nc.value == -9 and list(self.out) == [-1, -2, -3, -4]


def _raw(dev, o, cap=2):
    return dev.lib.cx_log_evidence_components_mfma(dev.h, cap, o.pv, o.pc, C.byref(o.nc), o.out)


def test_refusals_and_arguments(hip_lib):
    # (call: the C entry itself, raised by the binding's own check — DeviceGraph.log_evidence_components_mfma counts the components
    # first, and a handle without a graph is refused by that count under another name)
    assert_reader_refusals("cx_log_evidence_components_mfma", "cx_log_evidence_components", lambda dev: dev._check(_raw(dev, _Out())),
                           lambda dev: dev.log_evidence_components(), lambda dev: _raw(dev, _Out()))
    # a dim 2 handle: a refused call leaves its outputs as they are
    dev = _dev(cx.synth.concat_models(CS.chain_parts(2, (2, 3))), L.SCHED_TREE)
    o = _Out()
    assert dev.lib.cx_log_evidence_components_mfma(dev.h, 2, o.pv, o.pc, C.byref(o.nc), o.out) == L.ERR_UNSUPPORTED and o.untouched()
    assert "cx_log_evidence_components" in dev.last_error().replace("cx_log_evidence_components_mfma", "")
    dev.close()
    # a variational family
    dev = cx.DeviceGraph(schedule=L.SCHED_CHAIN_SCAN, family=L.FAMILY_VMP_STRUCTURED)
    cx.synth.load_vmp_into_device(cx.synth.vmp_ssm(8), dev)
    assert dev.lib.cx_log_evidence_components_mfma(dev.h, 2, o.pv, o.pc, C.byref(o.nc), o.out) == L.ERR_UNSUPPORTED and o.untouched()
    assert "Gaussian family" in dev.last_error()
    dev.close()
    # no graph
    dev = cx.DeviceGraph(dim=16, schedule=L.SCHED_TREE)
    assert dev.lib.cx_log_evidence_components_mfma(dev.h, 2, o.pv, o.pc, C.byref(o.nc), o.out) == L.ERR_STATE and o.untouched()
    # ... then a graph on the same handle: it works on
    parts, model, _ = M.chains(16)
    cx.synth.load_into_device(model, dev)
    dev.sweep(1)
    good, good_cc, good_counts = dev.log_evidence_components_mfma()
    assert len(good) == 3 and np.isfinite(good).all()
    call = dev.lib.cx_log_evidence_components_mfma
    bad = ((3, o.pv, o.pc, None, o.out), (3, o.pv, o.pc, C.byref(o.nc), None), (3, None, o.pc, C.byref(o.nc), o.out), (-1, o.pv, o.pc, C.byref(o.nc), o.out))
    for args in bad:
        assert call(dev.h, *args) == L.ERR_INVALID_ARGUMENT and o.untouched(), args[0]
        assert _bits(dev.log_evidence_components_mfma()[0]) == _bits(good)
    # the sizing call: the count and counts4, which do not depend on cap
    nc, out = C.c_int64(), (C.c_int64 * 4)()
    assert call(dev.h, 0, None, None, C.byref(nc), out) == L.OK and nc.value == 3 and list(out) == list(good_counts.values())
    val = np.zeros(3)
    assert call(dev.h, 3, val.ctypes.data_as(C.POINTER(C.c_double)), None, C.byref(nc), out) == L.OK and _bits(val) == _bits(good)
    assert list(out) == list(good_counts.values())
    # the dim 1 - 4 call keeps refusing these dims, and writes nothing
    assert dev.lib.cx_log_evidence_components(dev.h, 3, o.pv, o.pc, C.byref(o.nc), o.out) == L.ERR_UNSUPPORTED and o.untouched()
    dev.close()
    # a partitioned handle (a halo list: x_1 and the first transition of a T = 4 chain)
    m16 = cx.synth.lgssm_chain(4, d=16, seed=92)
    dev = _dev(m16, L.SCHED_FUSED, 2)
    dev.halo_configure_state([m16.x_ids[0]], [3 * 4 + 1], [], [])
    assert dev.lib.cx_log_evidence_components_mfma(dev.h, 3, o.pv, o.pc, C.byref(o.nc), o.out) == L.ERR_UNSUPPORTED and o.untouched()
    assert "partitioned handle" in dev.last_error()
    dev.close()


# ---- 7: learn.profile at d = 16 ----------------------------------------------------------------------------------------------------------
def test_profile_over_q_scales(hip_lib):
    d = 16
    model = cx.synth.lgssm_chain(40, d=d, seed=41)
    A, Q = model.psets[0]
    scales = (0.25, 0.5, 1.0, 2.0, 4.0)
    cands = [{0: (A, s * Q)} for s in scales]
    loglik, cc = learn.profile(model, cands)
    assert loglik.shape == (5,) and cc.shape == (5, 4) and cc[:, 2:].sum() == 0
    single = []
    for cand in cands:
        dev = cx.DeviceGraph(dim=d, schedule=L.SCHED_TREE)
        cx.synth.load_into_device(model, dev)
        dev.set_factor_matrices(0, *cand[0])
        dev.sweep(1)
        single.append(dev.log_evidence_mfma()[0])
        dev.close()
    for got, want in zip(loglik, single):
        print(f"profile: got {got!r} want {want!r}")
        assert abs(got - want) <= 1e-9 * abs(want), (got, want)
    assert int(np.argmax(loglik)) == int(np.argmax(single))


# ---- 8: learn.multi_start_em at d = 16 ---------------------------------------------------------------------------------------------------
def test_multi_start_em(hip_lib):
    d, n_iter = 16, 4
    model = cx.synth.lgssm_chain(60, d=d, seed=43)
    A, Q = model.psets[0]
    starts = [{0: (0.5 * A, 3.0 * Q)}, {0: (np.eye(d) * 0.7, np.eye(d))}, {0: (A, 0.2 * Q)}]
    which = {0: ("A", "Q"), 1: ()}
    trace, params, best = learn.multi_start_em(model, starts, n_iter, learn=which)
    assert trace.shape == (n_iter + 1, 3) and np.isfinite(trace).all() and len(params) == 3
    assert best == int(np.argmax(trace[-1]))
    # non-decreasing (the chain scan is an exact E-step), up to 1e-9 relative of its own size
    assert (np.diff(trace, axis=0) >= -1e-9 * np.abs(trace[:-1])).all(), trace
    assert (trace[-1] > trace[0]).all()
    for k, start in enumerate(starts):
        one = cx.DeviceGraph(dim=d, schedule=L.SCHED_CHAIN_SCAN)
        cx.synth.load_into_device(model, one)
        alone, fitted = learn.em(one, {**model.psets, **start}, n_iter, learn=which)
        one.close()
        alone = np.asarray(alone)
        print(f"start {k}: trace {trace[:, k]!r} alone {alone!r}")
        assert (np.abs(trace[:, k] - alone) <= 1e-9 * np.abs(alone)).all(), (k, trace[:, k], alone)
        assert sorted(params[k]) == sorted(model.psets)
        for s in model.psets:
            for got, want in zip(params[k][s], fitted[s]):
                assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), (k, s, np.abs(got - want).max())


# ---- 9: the C++ client -------------------------------------------------------------------------------------------------------------------
def test_cpp_host_class_components_mfma(hip_lib, tmp_path):
    lines = [line.split() for line in run_demo("components_mfma_demo", tmp_path)]
    assert [l for l in lines if l[0] == "components"][0][1:] == ["2"]
    d = 16
    rows = [l for l in lines if l[0] == "value"]
    assert len(rows) == 2
    for row, T in zip(rows, (5, 9)):
        A, Q, R, y = demo_chain(T, d)
        want = E.kalman_log_lik(np.broadcast_to(A, (T - 1, d, d)), np.zeros((T - 1, d)), np.broadcast_to(Q, (T - 1, d, d)),
                                np.broadcast_to(R, (T, d, d)), y)
        got = float(row[2])
        assert abs(got - want) <= 1e-9 * abs(want), (T, got, want)
        assert row[3:] == [str(2 * T - 1), str(T), "0", "0"]
    assert [l for l in lines if l[0] == "counts"][0][1:] == [str(2 * 14 - 2), "14", "0", "0"]
