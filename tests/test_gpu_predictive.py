"""-m gpu: cx_predictive — the predictive distribution, log score and squared standardised residual of every datum that a Gaussian rule
factor generates, from the stored messages — against the dense leave-one-out solve, the Kalman innovations and the numpy
restatement of the formula (tests/predictive_support.py, pinned by tests/test_predictive_checker.py)."""
import math

import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from cortex.jl_amd import get_value, get_variable_marginal, update_marginals
from tests import evidence_support as E
from tests import predictive_support as P
from tests.test_gpu_kary_mv import _kary_tree, _load as _load_kary
from tests.test_host_mirror import make_ssm
from tests.gpu_support import code_of, iterative_device, run_demo

pytestmark = pytest.mark.gpu
EXACT, PARITY = 1e-9, 1e-10      # against exact solves (test_gpu_evidence.py: _exact); against the restatement on the device's messages


def _kalman_rows(model, fids):
    yh, S, term, maha = P.innovations_of_chain(model)
    return {"factor_ids": fids, "mean": yh, "cov": S, "log_density": term, "mahalanobis": maha}


def _check_chain(model, dev, what):
    """LOO rows = the dense solve, none improper; causal rows = the Kalman innovations, one improper; causal total = evidence = Kalman"""
    T = model.meta["T"]
    gm = E.gmodel(model)
    loo = dev.predictive("loo")
    assert loo["counts"] == {"rows": T, "scored": T, "undefined": 0, "improper": 0}, (what, loo["counts"])
    print(what, "loo", P.assert_rows_close(loo, P.dense_loo_all(gm), EXACT, what + " loo"))
    cau = dev.predictive("causal")
    assert cau["counts"] == {"rows": T, "scored": T - 1, "undefined": 0, "improper": 1}, (what, cau["counts"])
    print(what, "causal", P.assert_rows_close(cau, _kalman_rows(model, loo["factor_ids"]), EXACT, what + " causal"))
    ev, _ = dev.log_evidence()
    kal = E.kalman_of_chain(model)
    print(what, "totals", cau["total"], ev, kal)
    assert abs(cau["total"] - ev) <= EXACT * abs(ev) and abs(cau["total"] - kal) <= EXACT * abs(kal), (what, cau["total"], ev, kal)


DIM1_CHAINS = [("ssm_chain", lambda: cx.synth.ssm_chain(200, seed=21, random_variances=True), 420),
               ("ssm_chain_linear", lambda: cx.synth.ssm_chain_linear(150, seed=22), 320)]


@pytest.mark.parametrize("name,make,n_iter", DIM1_CHAINS, ids=[c[0] for c in DIM1_CHAINS])
def test_dim1_chains_after_every_schedule(hip_lib, name, make, n_iter):
    model = make()
    for s in (L.SCHED_CHAIN_SCAN, L.SCHED_TREE, L.SCHED_REFERENCE, L.SCHED_FUSED, L.SCHED_FLOODING):
        dev = iterative_device(model, s, n_iter)
        _check_chain(model, dev, f"{name} schedule {s}")
        dev.close()


@pytest.mark.parametrize("d", [2, 3, 4])
def test_dims_2_to_4_chains_and_comb_after_every_schedule(hip_lib, d):
    model = cx.synth.lgssm_chain(60, d=d, seed=30 + d)
    for s in (L.SCHED_CHAIN_SCAN, L.SCHED_TREE, L.SCHED_REFERENCE, L.SCHED_FUSED):
        dev = iterative_device(model, s, 200)
        _check_chain(model, dev, f"d {d} lgssm_chain schedule {s}")
        dev.close()
    model = cx.synth.lgssm_comb(15, d=d, teeth=1, seed=40 + d)
    want = P.dense_loo_all(E.gmodel(model))
    for s in (L.SCHED_TREE, L.SCHED_REFERENCE, L.SCHED_FUSED):
        dev = iterative_device(model, s, 200)
        loo = dev.predictive("loo")
        assert loo["counts"] == {"rows": 30, "scored": 30, "undefined": 0, "improper": 0}
        print(d, s, "comb loo", P.assert_rows_close(loo, want, EXACT, f"d {d} lgssm_comb schedule {s}"))
        dev.close()


def test_dim1_tree_with_kary_rows_after_every_schedule(hip_lib):
    model = cx.synth.tree_model(120, seed=23, k_choices=(1, 2, 3, 5, 6), observe=0.25)
    gm = E.gmodel(model)
    rows = P.rows_of(gm)
    assert sum(1 for r in rows if r[1] == 2) >= 2 and sum(1 for r in rows if r[1] > 2) >= 2
    want = P.dense_loo_all(gm)
    for s in (L.SCHED_TREE, L.SCHED_REFERENCE, L.SCHED_FUSED, L.SCHED_FLOODING):
        dev = iterative_device(model, s, 400)
        loo = dev.predictive("loo")
        assert loo["counts"] == {"rows": len(rows), "scored": len(rows), "undefined": 0, "improper": 0}
        print(s, "tree loo", P.assert_rows_close(loo, want, EXACT, f"tree_model schedule {s}"))
        dev.close()


@pytest.mark.parametrize("seed", [3, 6, 10, 13, 17])
def test_a_cavity_with_no_message_left_is_improper_by_structure(hip_lib, seed):
    # (M - m_lik) - m_transition at x_1 rounds to a tiny positive precision on these chains (tests/test_predictive_checker.py)
    model = cx.synth.ssm_chain_linear(6, seed=seed)
    want = E.kalman_of_chain(model)
    for s in (L.SCHED_CHAIN_SCAN, L.SCHED_TREE, L.SCHED_REFERENCE):
        dev = iterative_device(model, s)
        cau = dev.predictive("causal")
        assert cau["counts"] == {"rows": 6, "scored": 5, "undefined": 0, "improper": 1}, (s, cau["counts"])
        assert np.isnan(cau["log_density"][0]) and abs(cau["total"] - want) <= EXACT * abs(want)
        dev.close()


def _observed_kary_tree(d, seed):
    """tests.test_gpu_kary_mv._kary_tree with a datum on every OUT state that is a leaf: k-ary rows at dim > 1"""
    model, prior, facs, fid, sets, _mean, _cov = _kary_tree(12, d, seed, k_choices=(2, 3, 5))
    n = len(model.x_ids)
    used = {i for (_o, ins, _s, _q) in facs for i in ins}
    leaves = [(int(model.x_ids[o]), int(f)) for f, (o, _ins, _s, _q) in zip(fid, facs) if o not in used]
    assert len(leaves) >= 3
    rng = np.random.default_rng(seed + 100)
    model.data_var, model.data_fac = np.array([v for v, _ in leaves], np.int64), np.array([f for _, f in leaves], np.int64)
    model.data_y = rng.standard_normal((len(leaves), d)) * 1.5
    edge_sets = {(int(model.x_ids[i]), int(f)): s for f, (_o, ins, ss, _q) in zip(fid, facs) for i, s in zip(ins, ss)}
    gm = E.gmodel(model, edge_sets=edge_sets, opaque=(model.x_ids, model.x_ids + n, prior[0], prior[1]))
    return model, prior, facs, fid, sets, gm, len(leaves)


@pytest.mark.parametrize("d", [2, 3])
def test_kary_rows_at_dim_2_and_3(hip_lib, d):
    model, prior, facs, fid, sets, gm, n_rows = _observed_kary_tree(d, 50 + d)
    want = P.dense_loo_all(gm)
    assert len(want["factor_ids"]) == n_rows and all(r[1] > 2 for r in P.rows_of(gm))
    for s in (L.SCHED_TREE, L.SCHED_REFERENCE, L.SCHED_FUSED):
        dev = _load_kary(model, prior, facs, fid, sets, s, seed_variance=1e6 if s == L.SCHED_FUSED else None)
        dev.sweep(4 * len(facs) + 40 if s == L.SCHED_FUSED else 1)
        loo = dev.predictive("loo")
        assert loo["counts"] == {"rows": n_rows, "scored": n_rows, "undefined": 0, "improper": 0}, loo["counts"]
        print(d, s, "k-ary loo", P.assert_rows_close(loo, want, EXACT, f"d {d} k-ary tree schedule {s}"))
        # parity of the causal mode with the restatement on the device's own messages
        f2v, opq = E.device_messages(gm, dev)
        cau = dev.predictive("causal")
        print(d, s, "k-ary causal", P.assert_rows_close(cau, P.predictive_from_messages(gm, f2v, opq, P.CAUSAL), PARITY, f"d {d} k-ary causal"))
        dev.close()


def _parity(model, gm, dev, what):
    f2v, opq = E.device_messages(gm, dev)
    for mode, m in (("loo", P.LOO), ("causal", P.CAUSAL)):
        got, want = dev.predictive(mode), P.predictive_from_messages(gm, f2v, opq, m)
        assert got["counts"] == want["counts"], (what, mode, got["counts"], want["counts"])
        assert want["counts"]["scored"] > 0
        print(what, mode, P.assert_rows_close(got, want, PARITY, f"{what} {mode}"))
        assert abs(got["total"] - want["total"]) <= PARITY * abs(want["total"]), (what, mode, got["total"], want["total"])
    return f2v, opq


def test_formula_parity_off_a_fixed_point(hip_lib):
    # a loopy scalar model of k-ary factors with observed leaves, after a few fused sweeps
    model = cx.synth.kary_model(60, seed=24, tree=False, observe=0.5)
    gm = E.gmodel(model)
    assert len(P.rows_of(gm)) >= 2
    dev = iterative_device(model, L.SCHED_FUSED, 6)
    _parity(model, gm, dev, "kary_model(tree=False)")
    dev.close()
    # a loopy grid with an observed end hung on some of its variables (CX_FACTOR_GAUSS_ADDITIVE rows, the datum on the higher id)
    grid = cx.synth.gaussian_grid(6, 5, seed=5)
    V, top = 30, int(max(grid.edge_var.max(), grid.edge_fac.max()))
    xs = np.arange(1, V + 1, 4, dtype=np.int64)
    ys, fs = top + 1 + np.arange(len(xs)), top + 1 + len(xs) + np.arange(len(xs))
    rng = np.random.default_rng(6)
    model = cx.synth.Model(edge_var=np.concatenate([grid.edge_var, xs, ys]), edge_fac=np.concatenate([grid.edge_fac, fs, fs]),
                           factor_ids=np.concatenate([grid.factor_ids, fs]),
                           factor_kind=np.concatenate([grid.factor_kind, np.full(len(xs), L.FACTOR_GAUSS_ADDITIVE, np.int32)]),
                           factor_var=np.concatenate([grid.factor_var, rng.uniform(0.5, 2.0, len(xs))]), x_ids=grid.x_ids, data_var=ys, data_fac=fs,
                           data_y=rng.standard_normal(len(xs)) * 2, prior_var=grid.prior_var, prior_fac=grid.prior_fac, prior_mean=grid.prior_mean,
                           prior_variance=grid.prior_variance, meta={"kind": "grid+obs"})
    gm = E.gmodel(model)
    assert len(P.rows_of(gm)) == len(xs)
    dev = iterative_device(model, L.SCHED_FUSED, 5)
    _parity(model, gm, dev, "grid with observed ends")
    dev.close()
    # on a forest the dense solve itself stays within the parity tolerance of the restatement on the device's messages
    model = cx.synth.lgssm_chain(30, d=3, seed=8)
    gm = E.gmodel(model)
    dev = iterative_device(model, L.SCHED_CHAIN_SCAN)
    f2v, opq = _parity(model, gm, dev, "lgssm_chain d 3")
    print("dense vs restatement", P.assert_rows_close(P.dense_loo_all(gm), P.predictive_from_messages(gm, f2v, opq, P.LOO), PARITY, "dense vs restatement"))
    dev.close()


def _same_bits(a, b):
    return all(np.asarray(a[k], np.float64).tobytes() == np.asarray(b[k], np.float64).tobytes() for k in ("mean", "cov", "log_density", "mahalanobis", "total"))


def test_semantics(hip_lib):
    model = cx.synth.ssm_chain_linear(80, seed=41)
    dev = iterative_device(model, L.SCHED_TREE)
    for mode in ("loo", "causal"):
        full = dev.predictive(mode)
        again = dev.predictive(mode)
        assert _same_bits(full, again) and full["counts"] == again["counts"]             # two calls on one state: bit-identical
        assert np.array_equal(full["factor_ids"], dev.predictive_rows()) and np.array_equal(full["factor_ids"], np.sort(model.data_fac))
        short = dev.predictive(mode, rows=False)
        assert short["mean"] is None and short["counts"] == full["counts"]
        assert np.float64(short["total"]).tobytes() == np.float64(full["total"]).tobytes()
        # the caller's order; a subset equals the same rows of the full call bit for bit
        pick = np.array([70, 3, 41, 0, 79, 12])
        sub = dev.predictive(mode, factor_ids=full["factor_ids"][pick])
        assert np.array_equal(sub["factor_ids"], full["factor_ids"][pick])
        for k in ("mean", "cov", "log_density", "mahalanobis"):
            assert sub[k].tobytes() == full[k][pick].tobytes(), (mode, k)
        assert sub["counts"]["rows"] == len(pick)
        ld = sub["log_density"][~np.isnan(sub["log_density"])]
        assert abs(sub["total"] - math.fsum(ld.tolist())) <= 1e-13 * abs(sub["total"])
        # total only (NULL out, NULL total)
        cnt = (L.C.c_int64 * 4)()
        assert dev.lib.cx_predictive(dev.h, L.PREDICT_LOO, 0, None, None, None, cnt) == L.OK and cnt[0] == 80
    dev.close()


def test_no_side_effects(hip_lib):
    model = cx.synth.tree_model(60, seed=23, k_choices=(1, 2, 3), observe=0.25)
    dev = iterative_device(model, L.SCHED_REFERENCE)
    blob, trace, health, stats = dev.export_state(), dev.ref_trace(), dev.message_health(), dev.ref_plan_stats()
    msgs, marg = dev.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE), dev.get_marginals(model.x_ids)
    stats = dev.ref_plan_stats()
    dev.predictive("loo"); dev.predictive("causal"); dev.predictive("loo", rows=False)
    assert dev.ref_plan_stats() == stats and dev.message_health() == health and dev.ref_trace() == trace
    assert np.array_equal(blob, dev.export_state())
    assert np.array_equal(msgs, dev.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE), equal_nan=True)
    assert np.array_equal(marg, dev.get_marginals(model.x_ids), equal_nan=True)
    dev.close()
    model = cx.synth.lgssm_chain(50, d=4, seed=72)
    dev = iterative_device(model, L.SCHED_CHAIN_SCAN)
    dev.predictive("causal")                            # (the chain messages go to their slots on the first read-out)
    blob, health = dev.export_state(), dev.message_health()
    dev.predictive("causal"); dev.predictive("loo")
    assert np.array_equal(blob, dev.export_state()) and dev.message_health() == health
    dev.close()
    # fused: the next sweeps are those of a twin handle that never called it, bit for bit
    model = cx.synth.ssm_chain(40, seed=73)
    a, b = iterative_device(model, L.SCHED_FUSED, 5), iterative_device(model, L.SCHED_FUSED, 5)
    a.predictive("loo"); a.predictive("causal")
    a.sweep(3); b.sweep(3)
    assert np.array_equal(a.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE), b.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE), equal_nan=True)
    assert np.array_equal(a.get_marginals(model.x_ids), b.get_marginals(model.x_ids), equal_nan=True)
    a.close(); b.close()


def test_new_parameters_are_read(hip_lib):
    model = cx.synth.lgssm_chain(200, d=2, seed=61)
    dev = iterative_device(model, L.SCHED_CHAIN_SCAN)
    first = dev.predictive("causal")
    kal = E.kalman_of_chain(model)
    assert abs(first["total"] - kal) <= EXACT * abs(kal)
    A, Q = model.psets[0]
    dev.set_factor_matrices(0, 0.5 * A, Q)
    dev.sweep(1)
    second = dev.predictive("causal")
    other = cx.synth.lgssm_chain(200, d=2, seed=61)
    other.meta["A"] = 0.5 * A
    want = E.kalman_of_chain(other)
    assert abs(second["total"] - want) <= EXACT * abs(want), (second["total"], want)
    assert first["total"] > second["total"]             # the data came from A: the true parameters score higher
    assert P.scaled_err(second["mean"][1:], first["mean"][1:]) > 1e-3
    dev.close()


def test_undefined_rows_are_nan_and_counted_apart(hip_lib):
    model = cx.synth.ssm_chain(50, seed=81)
    dev = cx.DeviceGraph(schedule=L.SCHED_TREE)
    cx.synth.load_into_device(model, dev)
    for mode in ("loo", "causal"):
        res = dev.predictive(mode)                      # before any sweep
        assert res["counts"] == {"rows": 50, "scored": 0, "undefined": 50, "improper": 0}, res["counts"]
        assert np.isnan(res["log_density"]).all() and np.isnan(res["mean"]).all() and res["total"] == 0.0
    dev.sweep(1)
    assert dev.predictive("loo")["counts"]["scored"] == 50
    dev.close()
    one = cx.synth.ssm_chain(1, seed=82)                # one state and no prior: improper, not undefined
    dev = iterative_device(one, L.SCHED_TREE)
    assert dev.predictive("loo")["counts"] == {"rows": 1, "scored": 0, "undefined": 0, "improper": 1}
    dev.close()


def test_refusals(hip_lib):
    dev = cx.DeviceGraph()
    assert code_of(dev.predictive)[0] == L.ERR_STATE                            # no graph
    dev.close()
    dev = cx.DeviceGraph(family=L.FAMILY_NATURAL2)
    assert code_of(dev.predictive)[0] == L.ERR_UNSUPPORTED
    dev.close()
    vm = cx.synth.vmp_ssm(8)
    dev = cx.DeviceGraph(schedule=L.SCHED_CHAIN_SCAN, family=L.FAMILY_VMP_STRUCTURED)
    cx.synth.load_vmp_into_device(vm, dev)
    assert code_of(dev.predictive)[0] == L.ERR_UNSUPPORTED
    dev.close()
    m16 = cx.synth.lgssm_chain(4, d=16, seed=91)
    dev = iterative_device(m16, L.SCHED_FUSED, 2)
    assert code_of(dev.predictive)[0] == L.ERR_UNSUPPORTED                      # dim >= 5
    dev.close()
    T = 20
    model = cx.synth.ssm_chain(T, seed=92)
    dev = iterative_device(model, L.SCHED_FUSED, 5)
    cnt = (L.C.c_int64 * 4)()
    assert dev.lib.cx_predictive(dev.h, L.PREDICT_LOO, 0, None, None, None, None) == L.ERR_INVALID_ARGUMENT      # NULL counts4
    assert dev.lib.cx_predictive(dev.h, 2, 0, None, None, None, cnt) == L.ERR_INVALID_ARGUMENT                   # unknown mode
    code, msg = code_of(lambda: dev.predictive("loo", factor_ids=[2 * T + 1, 999]))
    assert code == L.ERR_NOT_FOUND and "999" in msg
    code, msg = code_of(lambda: dev.predictive("loo", factor_ids=[2 * T + 1, 3 * T + 1]))                          # a transition: no observed end
    assert code == L.ERR_UNSUPPORTED and f"factor {3 * T + 1}" in msg
    # a stream under capture (relaxed mode: the refusal's own runtime queries do not void the capture)
    hip = L.C.CDLL([ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln][0])      # the runtime the library itself loaded
    stream, graph = L.C.c_void_p(), L.C.c_void_p()
    assert hip.hipStreamCreate(L.C.byref(stream)) == 0
    dev.set_stream(stream.value)
    assert hip.hipStreamBeginCapture(stream, 2) == 0
    rc = dev.lib.cx_predictive(dev.h, L.PREDICT_LOO, 0, None, None, None, cnt)
    assert hip.hipStreamEndCapture(stream, L.C.byref(graph)) == 0
    if graph.value:
        hip.hipGraphDestroy(graph)
    dev.set_stream(None)
    assert hip.hipStreamDestroy(stream) == 0
    assert rc == L.ERR_STATE
    assert dev.predictive("loo")["counts"]["rows"] == T                       # and the handle works on
    dev.halo_configure([1], [2 * T + 1], [], [])                              # a halo list: a partitioned handle
    assert code_of(dev.predictive)[0] == L.ERR_UNSUPPORTED
    dev.close()
    model = cx.synth.ssm_chain(10, seed=93, q=0.0)
    dev = cx.DeviceGraph(schedule=L.SCHED_TREE)
    cx.synth.load_into_device(model, dev)
    code, msg = code_of(dev.predictive)
    assert code == L.ERR_UNSUPPORTED and "factor 31" in msg                   # zero noise: the first transition (ids 3T + 1 ..)
    dev.close()
    # a factor with two observed ends, and a CX_FACTOR_GAUSS_LINEAR whose IN end is the observed one
    model = cx.synth.ssm_chain_linear(6, seed=94)
    dev = cx.DeviceGraph(schedule=L.SCHED_TREE)
    cx.synth.load_into_device(model, dev)
    dev.set_messages([1], [3 * 6 + 1], L.TO_FACTOR, L.FORM_POINT, [0.3])      # x_1 observed: likelihood 2T + 1 now has two observed ends
    code, msg = code_of(lambda: dev.predictive("loo", factor_ids=[2 * 6 + 1]))
    assert code == L.ERR_UNSUPPORTED and "factor 13" in msg
    code, msg = code_of(lambda: dev.predictive("loo", factor_ids=[3 * 6 + 1]))   # x_2 = a x_1 + b + noise with x_1 (IN) observed
    assert code == L.ERR_UNSUPPORTED and "factor 19" in msg
    assert list(dev.predictive_rows()) == list(range(2 * 6 + 2, 3 * 6 + 1))    # the other likelihoods
    dev.close()


def test_hip_processor_predictive(hip_lib):
    n = 60
    rng = np.random.default_rng(5)
    data = [2 * i + rng.standard_normal() for i in range(1, n + 1)]
    y = np.asarray(data).reshape(n, 1)
    want = E.kalman_log_lik(np.ones(n - 1), np.zeros(n - 1), np.ones(n - 1), np.ones(n), y)
    for proc in (cx.HipProcessor(mode="sweep", n_sweeps=1, schedule=L.SCHED_TREE), cx.HipProcessor(mode="reference")):
        engine, x, yv, likelihood, _tr = make_ssm(n, proc, trace=False)
        for i in range(n):
            proc.set_value(engine.get_connection_message_to_factor(yv[i], likelihood[i]), data[i])
        update_marginals(engine, x)
        get_value(get_variable_marginal(engine.get_variable(x[0])))
        cau = proc.predictive("causal")
        assert cau["counts"] == {"rows": n, "scored": n - 1, "undefined": 0, "improper": 1}
        assert abs(cau["total"] - want) <= EXACT * abs(want), (proc.mode, cau["total"], want)
        ev, _ = proc.log_evidence()
        assert abs(cau["total"] - ev) <= EXACT * abs(ev)
        loo = proc.predictive("loo")
        assert loo["counts"]["scored"] == n and np.all(loo["cov"] > 1.0)          # S = the cavity's variance + r, r = 1
        short = proc.predictive("loo", rows=False)
        assert short["mean"] is None and short["total"] == loo["total"] and short["counts"] == loo["counts"]


def test_cpp_host_class_predictive(hip_lib, tmp_path):
    out_lines = run_demo("predictive_demo", tmp_path)
    lines = [line.split() for line in out_lines]
    T = 50
    model = cx.synth.ssm_chain(T, seed=1)
    model.data_y = np.array([0.5 * t + (7 * t) % 5 for t in range(1, T + 1)], dtype=np.float64)
    dev = iterative_device(model, L.SCHED_CHAIN_SCAN)
    for mode in ("loo", "causal"):
        want = dev.predictive(mode)
        tot = [l for l in lines if l[0] == mode + "_total"][0]
        assert abs(float(tot[1]) - want["total"]) <= 1e-12 * abs(want["total"])
        assert [int(v) for v in tot[2:]] == list(want["counts"].values())
        rows = np.array([[float(v) for v in l[2:]] for l in lines if l[0] == mode], dtype=np.float64)
        got = {"factor_ids": np.array([int(l[1]) for l in lines if l[0] == mode]), "mean": rows[:, :1], "cov": rows[:, 1:2].reshape(T, 1, 1),
               "log_density": rows[:, 2], "mahalanobis": rows[:, 3]}
        P.assert_rows_close(got, want, 1e-12, "c++ " + mode)
    want = E.kalman_of_chain(model)
    tot = [l for l in lines if l[0] == "causal_total"][0]
    assert abs(float(tot[1]) - want) <= EXACT * abs(want)
    dev.close()
