"""-m gpu: cx_log_evidence — log p(data) of Gaussian models from the stored messages — against the dense joint, the
Kalman filter and the numpy restatement of the formula (tests/evidence_support.py, pinned by tests/test_evidence_checker.py)."""
import math

import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from cortex.jl_amd import get_value, get_variable_marginal, update_marginals
from tests import evidence_support as E
from tests.test_gpu_kary_mv import _kary_tree, _load as _load_kary
from tests.test_host_mirror import make_ssm
from tests.gpu_support import code_of, iterative_device, run_demo

pytestmark = pytest.mark.gpu


def _exact(dev, want, rtol=1e-9, what=""):
    got, cnt = dev.log_evidence()
    assert cnt["undefined"] == 0 and cnt["not_positive_definite"] == 0, (what, cnt)
    assert abs(got - want) <= rtol * abs(want), (what, got, want)
    return got, cnt


DIM1 = [("ssm_chain", lambda: cx.synth.ssm_chain(200, seed=21), 420, True),
        ("ssm_chain_linear", lambda: cx.synth.ssm_chain_linear(150, seed=22), 320, True),
        ("tree_model", lambda: cx.synth.tree_model(60, seed=23, k_choices=(1, 2, 3, 4, 5, 6), observe=0.2), 160, False),
        ("kary_model", lambda: cx.synth.kary_model(40, seed=24, observe=0.2), 160, False)]


@pytest.mark.parametrize("name,make,n_iter,chain", DIM1, ids=[c[0] for c in DIM1])
def test_dim1_exact_after_every_schedule(hip_lib, name, make, n_iter, chain):
    model = make()
    gm = E.gmodel(model)
    want = E.dense_log_z(gm)
    schedules = [L.SCHED_TREE, L.SCHED_REFERENCE, L.SCHED_FUSED, L.SCHED_FLOODING] + ([L.SCHED_CHAIN_SCAN] if chain else [])
    for s in schedules:
        dev = iterative_device(model, s, n_iter)
        _, cnt = _exact(dev, want, what=f"{name} schedule {s}")
        assert cnt["factor_terms"] == sum(len(g["fid"]) for g in gm.groups.values())
        dev.close()


def _dim_models(d):
    return [("lgssm_chain", cx.synth.lgssm_chain(60, d=d, seed=30 + d), True), ("lgssm_comb", cx.synth.lgssm_comb(15, d=d, teeth=1, seed=40 + d), False)]


@pytest.mark.parametrize("d", [2, 3, 4])
def test_dims_2_to_4_exact_after_every_schedule(hip_lib, d):
    for name, model, chain in _dim_models(d):
        want = E.dense_log_z(E.gmodel(model))
        for s in [L.SCHED_TREE, L.SCHED_REFERENCE, L.SCHED_FUSED] + ([L.SCHED_CHAIN_SCAN] if chain else []):
            dev = iterative_device(model, s, 200)
            _exact(dev, want, what=f"d {d} {name} schedule {s}")
            dev.close()
    # a k-ary tree (factors of 3 .. 6 variables, a parameter set per input)
    model, prior, facs, fid, sets, _mean, _cov = _kary_tree(12, d, 50 + d, k_choices=(2, 3, 5))
    n = len(model.x_ids)
    edge_sets = {(int(model.x_ids[i]), int(f)): s for f, (_o, ins, ss, _q) in zip(fid, facs) for i, s in zip(ins, ss)}
    gm = E.gmodel(model, edge_sets=edge_sets, opaque=(model.x_ids, model.x_ids + n, prior[0], prior[1]))
    want = E.dense_log_z(gm)
    for s in (L.SCHED_TREE, L.SCHED_REFERENCE, L.SCHED_FUSED):
        dev = _load_kary(model, prior, facs, fid, sets, s, seed_variance=1e6 if s == L.SCHED_FUSED else None)
        dev.sweep(4 * len(facs) + 40 if s == L.SCHED_FUSED else 1)
        _exact(dev, want, what=f"d {d} k-ary tree schedule {s}")
        dev.close()


def test_size_scalar_chain_of_a_million_states(hip_lib):
    model = cx.synth.ssm_chain(10**6, seed=31)
    dev = iterative_device(model, L.SCHED_CHAIN_SCAN)
    _exact(dev, E.kalman_of_chain(model), what="T = 1e6, chain scan")
    dev.close()


def test_size_d4_chain_of_1e5_states(hip_lib):
    model = cx.synth.lgssm_chain(10**5, d=4, seed=32)
    dev = iterative_device(model, L.SCHED_CHAIN_SCAN)
    _exact(dev, E.kalman_of_chain(model), what="d = 4, T = 1e5, chain scan")
    dev.close()


def _loopy_check(model, n_sweeps):
    dev = iterative_device(model, L.SCHED_FUSED, n_sweeps)
    gm = E.gmodel(model)
    got, cnt = dev.log_evidence()
    again, _ = dev.log_evidence()
    assert np.float64(got).tobytes() == np.float64(again).tobytes()         # two calls on one state: bit-identical
    assert cnt["undefined"] == 0 and cnt["not_positive_definite"] == 0
    f2v, opq = E.device_messages(gm, dev)
    want = E.bethe_log_z(gm, f2v, opq)
    assert abs(got - want) <= 1e-10 * abs(want), (got, want)
    dev.close()
    return gm, got


def test_loopy_grid_matches_the_restatement(hip_lib):
    gm, got = _loopy_check(cx.synth.gaussian_grid(12, 10, seed=5), 400)
    assert abs(got - E.dense_log_z(gm)) > 1e-6 * abs(got)          # the Bethe estimate, not the exact value


def test_loopy_c4_after_200_fused_sweeps_matches_the_restatement(hip_lib):
    _loopy_check(cx.synth.gaussian_grid(1415, 1415), 200)


def test_new_parameters_are_read(hip_lib):
    # dim 2, chain scan: new (A, Q) of the transition set
    model = cx.synth.lgssm_chain(40, d=2, seed=61)
    dev = iterative_device(model, L.SCHED_CHAIN_SCAN)
    first, _ = _exact(dev, E.dense_log_z(E.gmodel(model)), what="old (A, Q)")
    A2, Q2 = 0.7 * np.array([[0.9, -0.3], [0.2, 0.8]]), np.array([[0.3, 0.05], [0.05, 0.2]])
    dev.set_factor_matrices(0, A2, Q2)
    dev.sweep(1)
    psets = dict(model.psets)
    psets[0] = (A2, Q2)
    second, _ = _exact(dev, E.dense_log_z(E.gmodel(model, psets=psets)), what="new (A, Q)")
    assert abs(second - first) > 1e-3
    dev.close()
    # dim 1, tree: new coefficients of the factors of more than two variables
    model = cx.synth.tree_model(30, seed=62, k_choices=(2, 3), observe=0.2)
    dev = iterative_device(model, L.SCHED_TREE)
    _exact(dev, E.dense_log_z(E.gmodel(model)), what="old coefficients")
    meta = model.meta
    new = np.asarray(meta["coef"]) * 1.3 + 0.1
    dev.set_factor_coefficients(meta["coef_var"], meta["coef_fac"], new)
    dev.sweep(1)
    coef = {(int(v), int(f)): float(a) for v, f, a in zip(meta["all_coef_var"], meta["all_coef_fac"], meta["all_coef"])}
    coef.update({(int(v), int(f)): float(a) for v, f, a in zip(meta["coef_var"], meta["coef_fac"], new)})
    _exact(dev, E.dense_log_z(E.gmodel(model, coef=coef)), what="new coefficients")
    dev.close()
    # dim 3, tree: other parameter sets on the inputs of the k-ary factors
    model, prior, facs, fid, sets, _m, _c = _kary_tree(8, 3, 63, k_choices=(2, 3))
    n = len(model.x_ids)
    dev = _load_kary(model, prior, facs, fid, sets, L.SCHED_TREE)
    dev.sweep(1)
    ev_, ef_ = [int(model.x_ids[i]) for (_o, ins, _s, _q) in facs for i in ins], [int(f) for f, (_o, ins, _s, _q) in zip(fid, facs) for _ in ins]
    es = [(s + 1) % len(sets) for (_o, _ins, ss, _q) in facs for s in ss]
    dev.set_factor_edge_sets(ev_, ef_, es)
    dev.sweep(1)
    gm = E.gmodel(model, edge_sets=dict(zip(zip(ev_, ef_), es)), opaque=(model.x_ids, model.x_ids + n, prior[0], prior[1]))
    _exact(dev, E.dense_log_z(gm), what="new edge sets")
    dev.close()


def test_no_side_effects(hip_lib):
    # reference order: the state blob and the trace are unchanged by the call
    model = cx.synth.tree_model(40, seed=71, k_choices=(1, 2, 3), observe=0.2)
    dev = iterative_device(model, L.SCHED_REFERENCE)
    blob, trace = dev.export_state(), dev.ref_trace()
    dev.log_evidence()
    assert np.array_equal(blob, dev.export_state())
    assert dev.ref_trace() == trace
    dev.close()
    # dim 4 chain scan: the blob too
    model = cx.synth.lgssm_chain(50, d=4, seed=72)
    dev = iterative_device(model, L.SCHED_CHAIN_SCAN)
    dev.log_evidence()
    blob = dev.export_state()
    dev.log_evidence()
    assert np.array_equal(blob, dev.export_state())
    dev.close()
    # fused: the next sweeps are those of a twin handle that never called it, bit for bit
    model = cx.synth.gaussian_grid(12, 10, seed=73)
    a, b = iterative_device(model, L.SCHED_FUSED, 5), iterative_device(model, L.SCHED_FUSED, 5)
    a.log_evidence()
    a.sweep(3); b.sweep(3)
    assert np.array_equal(a.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE), b.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE))
    assert np.array_equal(a.get_marginals(model.x_ids), b.get_marginals(model.x_ids))
    a.close(); b.close()


def test_undefined_states_are_nan(hip_lib):
    model = cx.synth.ssm_chain(50, seed=81)
    dev = cx.DeviceGraph(schedule=L.SCHED_TREE)
    cx.synth.load_into_device(model, dev)
    v, cnt = dev.log_evidence()                     # before any sweep
    assert math.isnan(v) and cnt["undefined"] > 0
    dev.sweep(1)
    _exact(dev, E.dense_log_z(E.gmodel(model)))
    dev.close()
    dev = cx.DeviceGraph(schedule=L.SCHED_REFERENCE)
    cx.synth.load_into_device(model, dev)
    dev.sweep_for(model.x_ids[:10])                 # a subset: messages from the far end are not computed
    v, cnt = dev.log_evidence()
    assert math.isnan(v) and cnt["undefined"] > 0
    dev.sweep(1)
    _exact(dev, E.dense_log_z(E.gmodel(model)))
    dev.close()


def test_refusals(hip_lib):
    dev = cx.DeviceGraph()
    assert code_of(dev.log_evidence)[0] == L.ERR_STATE                          # no graph
    dev.close()
    dev = cx.DeviceGraph(family=L.FAMILY_NATURAL2)
    assert code_of(dev.log_evidence)[0] == L.ERR_UNSUPPORTED
    dev.close()
    vm = cx.synth.vmp_ssm(8)
    dev = cx.DeviceGraph(schedule=L.SCHED_CHAIN_SCAN, family=L.FAMILY_VMP_STRUCTURED)
    cx.synth.load_vmp_into_device(vm, dev)
    assert code_of(dev.log_evidence)[0] == L.ERR_UNSUPPORTED
    dev.close()
    m16 = cx.synth.lgssm_chain(4, d=16, seed=91)
    dev = iterative_device(m16, L.SCHED_FUSED, 2)
    assert code_of(dev.log_evidence)[0] == L.ERR_UNSUPPORTED                    # dim >= 5
    dev.close()
    model = cx.synth.ssm_chain(20, seed=92)
    dev = iterative_device(model, L.SCHED_FUSED, 5)
    assert dev.lib.cx_log_evidence(dev.h, None, None) == L.ERR_INVALID_ARGUMENT
    dev.halo_configure([1], [2 * 20 + 1], [], [])                             # a halo list: a partitioned handle
    assert code_of(dev.log_evidence)[0] == L.ERR_UNSUPPORTED
    dev.close()
    model = cx.synth.ssm_chain(10, seed=93, q=0.0)
    dev = cx.DeviceGraph(schedule=L.SCHED_TREE)
    cx.synth.load_into_device(model, dev)
    code, msg = code_of(dev.log_evidence)
    assert code == L.ERR_UNSUPPORTED and "factor 31" in msg                   # the first transition (ids 3T + 1 ..)
    dev.close()


def test_hip_processor_log_evidence(hip_lib):
    n = 60
    rng = np.random.default_rng(5)
    data = [2 * i + rng.standard_normal() for i in range(1, n + 1)]
    want = E.kalman_log_lik(np.ones(n - 1), np.zeros(n - 1), np.ones(n - 1), np.ones(n), np.asarray(data).reshape(n, 1))
    for proc in (cx.HipProcessor(mode="sweep", n_sweeps=1, schedule=L.SCHED_TREE), cx.HipProcessor(mode="reference")):
        engine, x, y, likelihood, _tr = make_ssm(n, proc, trace=False)
        for i in range(n):
            proc.set_value(engine.get_connection_message_to_factor(y[i], likelihood[i]), data[i])
        update_marginals(engine, x)
        get_value(get_variable_marginal(engine.get_variable(x[0])))
        v, cnt = proc.log_evidence()
        assert cnt["undefined"] == 0 and abs(v - want) <= 1e-9 * abs(want), (proc.mode, v, want)


def test_cpp_host_class_log_evidence(hip_lib, tmp_path):
    out_lines = run_demo("evidence_demo", tmp_path)
    rows = {line.split()[0]: line.split()[1:] for line in out_lines}
    T = 50
    y = np.array([0.5 * t + (7 * t) % 5 for t in range(1, T + 1)], dtype=np.float64)
    want = E.kalman_log_lik(np.ones(T - 1), np.zeros(T - 1), np.ones(T - 1), np.ones(T), y.reshape(T, 1))
    assert math.isnan(float(rows["before"][0])) and int(rows["before"][3]) > 0
    got = float(rows["evidence"][0])
    assert abs(got - want) <= 1e-9 * abs(want), (got, want)
    assert rows["evidence"][1:] == [str(2 * T - 1), str(T), "0", "0"]      # every state has two or three factors
