"""-m gpu: cx_graph_components / cx_log_evidence_components — the log-evidence of every connected component of one handle (DESIGN.md
§4l) — against the dense joint of each component alone (tests/evidence_support.py) with the helpers of tests/components_support.py
(pinned by tests/test_components_checker.py)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from cortex.jl_amd import learn
from tests import components_support as CS
from tests import evidence_support as E
from tests import missing_data as MD
from tests.gpu_support import code_of, run_demo

pytestmark = pytest.mark.gpu
LENGTHS = (2, 3, 65, 300)


def _bits(a):
    return np.asarray(a, dtype=np.float64).tobytes()


@functools.lru_cache(maxsize=None)
def _chains(d):
    """(parts, the parts as one graph, dense_log_z of every part alone) — computed once, never changed"""
    parts = CS.chain_parts(d, LENGTHS)
    return parts, cx.synth.concat_models(parts), tuple(E.dense_log_z(E.gmodel(p)) for p in parts)


def _dev(model, schedule, sweeps=1, opaque=None):
    dev = cx.DeviceGraph(dim=model.dim, schedule=schedule)
    cx.synth.load_into_device(model, dev, seed_variance=1e6 if schedule == L.SCHED_FUSED else None)
    if opaque is not None:
        v, f, eta, lam = opaque
        dev.set_messages(v, f, L.TO_VARIABLE, L.FORM_NATURAL, np.concatenate([eta, lam.reshape(len(v), -1)], axis=1))
    dev.sweep(sweeps)
    return dev


def _calls(dev, what):
    """test 4 on one handle: the sum against log_evidence, repeatability, cap, and log_evidence untouched.  Returns (values, comp_counts)"""
    before, cnt = dev.log_evidence()
    values, cc, counts = dev.log_evidence_components()
    again, cc2, _ = dev.log_evidence_components()
    assert _bits(values) == _bits(again) and (cc == cc2).all(), what
    two, cc_two, counts_two = dev.log_evidence_components(cap=2)
    assert len(two) == min(2, len(values)) and _bits(two) == _bits(values[:2]) and (cc_two == cc[:2]).all() and counts_two == counts, what
    after, cnt_after = dev.log_evidence()
    assert _bits(before) == _bits(after) and cnt == cnt_after, what
    assert counts == cnt and [int(x) for x in cc.sum(axis=0)] == list(cnt.values()), (what, counts, cnt, cc.sum(axis=0))
    if np.isfinite(values).all():
        gap, scale = abs(math.fsum(values.tolist()) - before), float(np.abs(values).sum())
        print(f"{what}: |fsum(values) - log_evidence| = {gap:.3e}, sum |values| = {scale:.6e}")
        assert gap <= 1e-12 * scale, (what, gap, scale)
    return values, cc


# ---- 1 (+ 4): exact per component, dim 2 - 4 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 3, 4])
def test_chains_exact_per_component(hip_lib, d):
    parts, model, wants = _chains(d)
    ids, lab, n = CS.labels(model)
    assert n == len(parts)
    for schedule, sweeps in ((L.SCHED_CHAIN_SCAN, 1), (L.SCHED_TREE, 1), (L.SCHED_FUSED, 2 * max(LENGTHS) + 40)):
        dev = _dev(model, schedule, sweeps)
        got_lab, got_n = dev.components()
        assert got_n == n and (got_lab == lab).all()
        some = ids[::7]
        assert (dev.components(some)[0] == lab[::7]).all()
        values, cc = _calls(dev, f"d {d} schedule {schedule}")
        assert cc[:, 2:].sum() == 0
        for k, want in enumerate(wants):
            print(f"d {d} schedule {schedule} component {k}: got {values[k]!r} want {want!r}")
            assert abs(want) >= 1
            assert abs(values[k] - want) <= 1e-9 * abs(want), (d, schedule, k, values[k], want)
        assert [int(x) for x in cc[:, 0]] == [2 * T - 1 for T in LENGTHS]
        dev.close()


# ---- 2: dim 1, k-ary factors, interleaved ids ----------------------------------------------------------------------------------------
def _tree():
    return cx.synth.tree_model(60, seed=23, k_choices=(1, 2, 3, 4, 5, 6), observe=0.2, components=5)


def test_dim1_kary_forest_with_interleaved_ids(hip_lib):
    model = _tree()
    assert len(np.unique(model.edge_var)) == 214
    rng = np.random.default_rng(17)
    for m, schedules in ((model, ((L.SCHED_TREE, 1), (L.SCHED_REFERENCE, 1), (L.SCHED_FUSED, 160))), (CS.relabel(model, rng), ((L.SCHED_TREE, 1),))):
        gm = E.gmodel(m)
        lab, n = CS.gm_labels(gm)
        assert n == 5 and (lab == CS.labels(m)[1]).all()
        wants = [E.dense_log_z(CS.restrict(gm, k, lab)) for k in range(n)]
        for schedule, sweeps in schedules:
            dev = _dev(m, schedule, sweeps)
            got_lab, got_n = dev.components()
            assert got_n == n and (got_lab == lab).all()
            values, cc = _calls(dev, f"dim 1 forest schedule {schedule}")
            for k, want in enumerate(wants):
                assert abs(want) >= 1
                assert abs(values[k] - want) <= 1e-9 * abs(want), (schedule, k, values[k], want)
            assert cc[:, 0].sum() == sum(len(g["fid"]) for g in gm.groups.values())
            dev.close()


# ---- 3 (+ 4): segments against tile borders ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _borders():
    """one chain of 3500 states, 300 chains of 2 and a lone variable with an opaque prior, dim 2, ids relabelled: (model, opaque message of
    the lone variable under the new ids, component of every part, dense_log_z of every part alone)"""
    d = 2
    first = cx.synth.lgssm_chain(3500, d=d, seed=77)
    A, Q, R = first.meta["A"], first.meta["Q"], first.meta["R"]
    parts = [first] + [cx.synth.lgssm_chain(2, d=d, seed=1000 + i, A=A, Q=Q, R=R) for i in range(300)]
    lone, opq = CS.lone_variable(d)
    lone.data_y = np.zeros((0, d))
    wants = [E.dense_log_z(E.gmodel(p)) for p in parts] + [E.dense_log_z(E.gmodel(lone, opaque=opq))]
    cat = cx.synth.concat_models(parts + [lone])
    model = CS.relabel(cat, np.random.default_rng(29))
    offs = [o for _, o in cat.meta["parts"]]
    ids, lab, n = CS.labels(model)
    comp_of_part = [int(lab[np.searchsorted(ids, CS.new_id(model, 1 + o))]) for o in offs]
    opq_new = (np.array([CS.new_id(model, 1 + offs[-1])], np.int64), np.array([CS.new_id(model, 2 + offs[-1])], np.int64), opq[2], opq[3])
    return model, opq_new, comp_of_part, wants, n


def test_segments_against_tile_borders(hip_lib):
    model, opq, comp_of_part, wants, n = _borders()
    assert n == 302 and sorted(comp_of_part) == list(range(n))
    dev = _dev(model, L.SCHED_TREE, 1, opaque=opq)
    assert dev.components()[1] == n
    values, cc = _calls(dev, "tile borders")
    assert cc[:, 2:].sum() == 0
    for part, (k, want) in enumerate(zip(comp_of_part[:-1], wants[:-1])):
        assert abs(values[k] - want) <= 1e-9 * abs(want), (part, k, values[k], want)
    lone = values[comp_of_part[-1]]
    print(f"the lone variable: value {lone!r} (exact 0; dense reference {wants[-1]!r})")
    assert abs(wants[-1]) <= 1e-12 and abs(lone) <= 1e-12
    assert list(cc[comp_of_part[-1]]) == [0, 1, 0, 0] and list(cc[comp_of_part[0]][:2]) == [2 * 3500 - 1, 3500]
    dev.close()


# ---- 5: loopy ------------------------------------------------------------------------------------------------------------------------
def test_two_loopy_grids_match_the_restatement(hip_lib):
    model = CS.join_scalar([cx.synth.gaussian_grid(12, 10, seed=5), cx.synth.gaussian_grid(7, 9, seed=6)])
    gm = E.gmodel(model)
    lab, n = CS.gm_labels(gm)
    assert n == 2
    dev = _dev(model, L.SCHED_FUSED, 400)
    values, cc = _calls(dev, "two grids")
    f2v, opq = E.device_messages(gm, dev)
    for k in range(n):
        fk, ok = CS.restrict_messages(gm, f2v, opq, k, lab)
        want = E.bethe_log_z(CS.restrict(gm, k, lab), fk, ok)
        assert abs(values[k] - want) <= 1e-10 * abs(want), (k, values[k], want)
    dev.close()


# ---- 6: isolation --------------------------------------------------------------------------------------------------------------------
def test_an_undefined_component_leaves_the_others_alone(hip_lib):
    parts, model, _ = _chains(2)
    dev = _dev(model, L.SCHED_TREE)
    clean, _, _ = dev.log_evidence_components()
    dev.close()
    broken = list(parts)
    broken[2] = MD.tail(parts[2], 3)                      # a forecast tail on the T = 65 chain; its end message is left unset
    dev = _dev(cx.synth.concat_models(broken), L.SCHED_TREE)
    values, cc, counts = dev.log_evidence_components()
    assert np.isnan(values[2]) and cc[2, 2] > 0, (values, cc)
    for k in (0, 1, 3):
        assert _bits(values[k]) == _bits(clean[k]) and cc[k, 2] == 0 and cc[k, 3] == 0, (k, values[k], clean[k])
    total, cnt = dev.log_evidence()
    assert np.isnan(total) and cnt == counts and cnt["undefined"] == cc[2, 2]
    dev.close()


# ---- 7: refusals and arguments -------------------------------------------------------------------------------------------------------
def test_refusals_and_arguments(hip_lib):
    # dim 16: the components, no evidence
    m16 = cx.synth.lgssm_chain(4, d=16)
    dev = cx.DeviceGraph(dim=16, schedule=L.SCHED_FUSED)
    cx.synth.load_into_device(m16, dev)                   # (cx_graph_create and the data; no sweep)
    lab, n = dev.components()
    assert n == 1 and len(lab) == 8 and not lab.any()
    assert code_of(dev.log_evidence_components)[0] == L.ERR_UNSUPPORTED
    assert dev.components()[1] == 1
    dev.close()
    # a variational family
    vm = cx.synth.vmp_ssm(8)
    dev = cx.DeviceGraph(schedule=L.SCHED_CHAIN_SCAN, family=L.FAMILY_VMP_STRUCTURED)
    cx.synth.load_vmp_into_device(vm, dev)
    nc, out = C.c_int64(), (C.c_int64 * 4)()
    assert dev.lib.cx_log_evidence_components(dev.h, 0, None, None, C.byref(nc), out) == L.ERR_UNSUPPORTED
    dev.close()
    # no graph
    dev = cx.DeviceGraph(dim=2, schedule=L.SCHED_TREE)
    assert dev.lib.cx_log_evidence_components(dev.h, 0, None, None, C.byref(nc), out) == L.ERR_STATE
    assert dev.lib.cx_graph_components(dev.h, 0, None, None, C.byref(nc)) == L.ERR_STATE
    # ... then a graph on the same handle: it works on
    model = cx.synth.concat_models(CS.chain_parts(2, (2, 3)))
    cx.synth.load_into_device(model, dev)
    dev.sweep(1)
    good, good_cc, _ = dev.log_evidence_components()
    assert len(good) == 2 and np.isfinite(good).all()
    val, cc = np.zeros(2), np.zeros((2, 4), np.int64)
    pv, pc = val.ctypes.data_as(C.POINTER(C.c_double)), cc.ctypes.data_as(C.POINTER(C.c_int64))
    bad = ((2, pv, pc, None, out), (2, pv, pc, C.byref(nc), None), (2, None, pc, C.byref(nc), out), (-1, pv, pc, C.byref(nc), out))
    for args in bad:
        assert dev.lib.cx_log_evidence_components(dev.h, *args) == L.ERR_INVALID_ARGUMENT, args[0]
        assert _bits(dev.log_evidence_components()[0]) == _bits(good)
    assert dev.lib.cx_log_evidence_components(dev.h, 0, None, None, C.byref(nc), out) == L.OK and nc.value == 2      # the sizing call
    assert dev.lib.cx_log_evidence_components(dev.h, 2, pv, None, C.byref(nc), out) == L.OK and _bits(val) == _bits(good)
    code, msg = code_of(dev.components, [1, 987654321])
    assert code == L.ERR_NOT_FOUND and "987654321" in msg
    assert dev.lib.cx_graph_components(dev.h, 0, None, None, None) == L.ERR_INVALID_ARGUMENT
    assert dev.components()[1] == 2
    dev.close()
    # a partitioned handle
    dev = _dev(model, L.SCHED_FUSED, 2)
    dev.halo_configure_state([], [], [], [])
    assert code_of(dev.log_evidence_components)[0] == L.ERR_UNSUPPORTED
    assert dev.components()[1] == 2
    dev.close()


# ---- 8: helpers ----------------------------------------------------------------------------------------------------------------------
def test_profile_over_q_scales(hip_lib):
    model = cx.synth.lgssm_chain(200, d=2, seed=41)
    A, Q = model.psets[0]
    scales = (0.25, 0.5, 1.0, 2.0, 4.0)
    cands = [{0: (A, s * Q)} for s in scales]
    loglik, cc = learn.profile(model, cands)
    assert loglik.shape == (5,) and cc.shape == (5, 4) and cc[:, 2:].sum() == 0
    single = []
    for cand in cands:
        dev = cx.DeviceGraph(dim=2, schedule=L.SCHED_TREE)
        cx.synth.load_into_device(model, dev)
        dev.set_factor_matrices(0, *cand[0])
        dev.sweep(1)
        single.append(dev.log_evidence()[0])
        dev.close()
    for got, want in zip(loglik, single):
        assert abs(got - want) <= 1e-9 * abs(want), (got, want)
    assert int(np.argmax(loglik)) == int(np.argmax(single))
    rep = cx.synth.replicas(model, cands)
    assert sorted(rep.psets) == list(range(10)) and rep.meta["replica_offset"] == [k * 799 for k in range(5)]


def test_multi_start_em_by_component(hip_lib):
    model = cx.synth.lgssm_chain(120, d=2, seed=43)
    A, Q = model.psets[0]
    starts = [{0: (0.5 * A, 3.0 * Q)}, {0: (np.eye(2) * 0.7, np.eye(2))}, {0: (A, 0.2 * Q)}]
    rep = cx.synth.replicas(model, starts)
    S = rep.meta["S"]
    dev = cx.DeviceGraph(dim=2, schedule=L.SCHED_CHAIN_SCAN)
    cx.synth.load_into_device(rep, dev)
    learn_sets = {k * S + s: (("A", "Q") if s == 0 else ()) for k in range(3) for s in range(S)}
    trace, params = learn.em(dev, rep.psets, 5, learn=learn_sets, by_component=True)
    dev.close()
    assert trace.shape == (6, 3)
    # non-decreasing (learn.em's guarantee for exact E-steps), up to the rounding of the compensated sums: the bound of the sum test
    assert (np.diff(trace, axis=0) >= -1e-12 * np.abs(trace[:-1])).all(), trace
    for k, start in enumerate(starts):
        one = cx.DeviceGraph(dim=2, schedule=L.SCHED_CHAIN_SCAN)
        cx.synth.load_into_device(model, one)
        alone, _ = learn.em(one, {**model.psets, **start}, 5, learn={0: ("A", "Q"), 1: ()})
        one.close()
        assert abs(trace[0, k] - alone[0]) <= 1e-9 * abs(alone[0]), (k, trace[0, k], alone[0])
        psets = {s: params[k * S + s] for s in range(S)}
        want = E.dense_log_z(E.gmodel(model, psets=psets))
        assert abs(trace[-1, k] - want) <= 1e-9 * abs(want), (k, trace[-1, k], want)


# ---- 9: the C++ client ---------------------------------------------------------------------------------------------------------------
def test_cpp_host_class_components(hip_lib, tmp_path):
    out_lines = run_demo("components_demo", tmp_path)
    lines = [line.split() for line in out_lines]
    # the same graph here: two scalar chains of 5 and 9 states with the demo's data
    parts = []
    for T in (5, 9):
        m = cx.synth.ssm_chain(T, seed=1)
        m.data_y = np.array([0.5 * t + (7 * t) % 5 for t in range(1, T + 1)], dtype=np.float64)
        parts.append(m)
    model = CS.join_scalar(parts)
    dev = _dev(model, L.SCHED_TREE)
    lab, n = dev.components()
    values, cc, counts = dev.log_evidence_components()
    assert [int(x) for x in [l for l in lines if l[0] == "components"][0][1:]] == [n]
    assert [int(x) for x in [l for l in lines if l[0] == "labels"][0][1:]] == list(lab)
    got = np.array([float(l[2]) for l in lines if l[0] == "value"])
    assert got.shape == values.shape and (np.abs(got - values) <= 1e-12 * np.abs(values)).all(), (got, values)
    assert [[int(x) for x in l[3:]] for l in lines if l[0] == "value"] == cc.tolist()
    assert [int(x) for x in [l for l in lines if l[0] == "counts"][0][1:]] == list(counts.values())
    for k, p in enumerate(parts):
        want = E.dense_log_z(E.gmodel(p))
        assert abs(values[k] - want) <= 1e-9 * abs(want)
    dev.close()
