"""-m gpu: cx_causal_marginals — the predicted, filtered and fixed-lag-smoothed marginals of the states from the stored messages
 — against the dense solve of the model without the data a mode leaves out, the Kalman filter, and the numpy restatement
of the definition (tests/causal_support.py, pinned by tests/test_causal_checker.py).

Tolerances: those of tests/test_gpu_predictive.py, the same arithmetic class — EXACT = 1e-9 against exact solves, PARITY = 1e-10 against
the restatement on the device's own messages — compared by its scaled_err / assert_rows_close.  The oracle-against-oracle floor measured
in tests/test_causal_checker.py (Kalman filter against the dense solve, both f64) is 3e-14 on these shapes: 1e-9 is far above 100 x it,
no case needs more.

At d = 1 the models are the scalar counterparts of the anisotropic builders, which name parameter sets and have no dim-1 form
(test_causal_checker.chain_of / tree_of): synth.ssm_chain_linear (CX_FACTOR_GAUSS_LINEAR with b != 0) and causal_support.scalar_tree."""
import copy

import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from tests import anisotropic as AN
from tests import causal_support as CS
from tests import evidence_support as E
from tests import missing_data as MD
from tests import predictive_support as P
from tests.test_causal_checker import chain_of, tree_of
from tests.test_gpu_kary_mv import _kary_tree, _load as _load_kary
from tests.gpu_support import code_of

pytestmark = pytest.mark.gpu
EXACT, PARITY = 1e-9, 1e-10
T = 12
MODES = (("predicted", 0, CS.PREDICTED), ("filtered", 0, CS.FILTERED), ("filtered", 1, CS.FILTERED), ("filtered", 3, CS.FILTERED), ("filtered", T, CS.FILTERED))


def _dev(model, schedule, sweeps=1, seed_variance=None):
    dev = cx.DeviceGraph(dim=model.dim, schedule=schedule)
    MD.load(model, dev)
    if seed_variance is not None:
        dev.seed_messages(L.TO_VARIABLE, 0.0, seed_variance)
    dev.sweep(sweeps)
    return dev


def _against_dense(model, dev, what, modes=MODES):
    gm = E.gmodel(model)
    for mode, lag, m in modes:
        got = dev.causal_marginals(mode, lag)
        want = CS.dense_causal_all(gm, m, lag)
        assert np.array_equal(got["variable_ids"] if got["variable_ids"] is not None else gm.var_ids, gm.var_ids)
        got["variable_ids"] = gm.var_ids
        assert got["counts"] == want["counts"], (what, mode, lag, got["counts"], want["counts"])
        print(what, mode, lag, CS.assert_close(got, want, EXACT, f"{what} {mode} lag {lag}"))
    return gm


def _smoothed_equals_marginals(model, dev, lag, what):
    d = model.dim
    got = dev.causal_marginals("filtered", lag, model.x_ids)
    marg = dev.get_marginals(model.x_ids)
    assert got["counts"]["finite"] == len(model.x_ids)
    assert P.scaled_err(got["mean"], marg[:, :d]) <= EXACT and P.scaled_err(got["cov"], marg[:, d:].reshape(-1, d, d)) <= EXACT, what


@pytest.mark.parametrize("schedule", [L.SCHED_CHAIN_SCAN, L.SCHED_TREE], ids=["scan", "tree"])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_chains(hip_lib, d, schedule):
    model = chain_of(d)
    dev = _dev(model, schedule)
    _against_dense(model, dev, f"chain d {d} schedule {schedule}")
    _smoothed_equals_marginals(model, dev, T, f"chain d {d}")
    dev.close()


@pytest.mark.parametrize("schedule", [L.SCHED_CHAIN_SCAN, L.SCHED_TREE], ids=["scan", "tree"])
def test_additive_chain_runs_backwards_in_time(hip_lib, schedule):
    model = cx.synth.ssm_chain(T, seed=5, random_variances=True)
    dev = _dev(model, schedule)
    _against_dense(model, dev, f"ssm_chain schedule {schedule}")
    _smoothed_equals_marginals(model, dev, T, "ssm_chain")
    pre = dev.causal_marginals("predicted", 0, model.x_ids)
    assert np.isnan(pre["mean"][-1]).all() and not np.isnan(pre["mean"][:-1]).any()      # the LAST state is the one without a prediction
    dev.close()


@pytest.mark.parametrize("d", [1, 3])
def test_two_slices_and_more_than_one_block_against_the_kalman_filter(hip_lib, d):
    n = 300
    model = chain_of(d, n)
    s = MD.chain_spec(model)
    f = MD.kalman_filter(s["A"], s["b"], s["Q"], s["H"], s["R"], s["y"], s["keep"])
    dev = _dev(model, L.SCHED_CHAIN_SCAN)
    pre, flt = dev.causal_marginals("predicted", 0, model.x_ids), dev.causal_marginals("filtered", 0, model.x_ids)
    assert pre["counts"] == {"rows": n, "finite": n - 1, "undefined": 0, "improper": 1} and flt["counts"]["finite"] == n
    assert np.isnan(pre["mean"][0]).all() and np.isnan(pre["cov"][0]).all()
    errs = (P.scaled_err(pre["mean"][1:], f["mp"][1:]), P.scaled_err(pre["cov"][1:], f["Pp"][1:]), P.scaled_err(flt["mean"], f["mf"]), P.scaled_err(flt["cov"], f["Pf"]))
    print(d, "kalman", errs)
    assert max(errs) <= EXACT, errs
    full = dev.causal_marginals("filtered", 0)        # every variable: the data rows too
    assert full["counts"] == {"rows": 2 * n, "finite": 2 * n, "undefined": 0, "improper": 0}
    sm = MD.kalman_missing(model)
    lagged = dev.causal_marginals("filtered", n, model.x_ids)
    assert P.scaled_err(lagged["mean"], sm["mean"]) <= EXACT and P.scaled_err(lagged["cov"], sm["cov"]) <= EXACT
    dev.close()


@pytest.mark.parametrize("family,d", [("lin", 1), ("gen", 2)])
def test_missing_data_and_a_forecast_tail(hip_lib, family, d):
    n, h = 16, 4
    model = MD.make(family, n, d, "run(5,9)", h=h)
    dev = _dev(model, L.SCHED_TREE)
    _against_dense(model, dev, f"{family} d {d} gap and tail", MODES[:4])
    pre, flt = dev.causal_marginals("predicted", 0, model.x_ids), dev.causal_marginals("filtered", 0, model.x_ids)
    gap = np.arange(5, 10)
    assert flt["mean"][gap].tobytes() == pre["mean"][gap].tobytes() and flt["cov"][gap].tobytes() == pre["cov"][gap].tobytes()      # no datum: nothing is added
    marg = dev.get_marginals(model.x_ids[n:])
    assert P.scaled_err(flt["mean"][n:], marg[:, :d]) <= EXACT and P.scaled_err(flt["cov"][n:], marg[:, d:].reshape(-1, d, d)) <= EXACT
    s = MD.chain_spec(model)
    f = MD.kalman_filter(s["A"], s["b"], s["Q"], s["H"], s["R"], s["y"], s["keep"])
    assert P.scaled_err(flt["mean"], f["mf"]) <= EXACT and P.scaled_err(flt["cov"], f["Pf"]) <= EXACT
    dev.close()


@pytest.mark.parametrize("shape", ["comb", "branching"])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_trees(hip_lib, d, shape):
    model = tree_of(shape, d)
    dev = _dev(model, L.SCHED_TREE)
    _against_dense(model, dev, f"{shape} d {d}", MODES[:4] + (("filtered", 15, CS.FILTERED),))
    _smoothed_equals_marginals(model, dev, 15, f"{shape} d {d}")
    dev.close()


@pytest.mark.parametrize("d", [2, 4])
def test_a_hub_in_the_csr_tail(hip_lib, d):
    model = AN.multi_sensor(6, d, sensors=12)         # twelve O-class messages into every state: degree 13 or 14
    dev = _dev(model, L.SCHED_TREE)
    assert dev.stats()["n_big_variables"] == 6
    _against_dense(model, dev, f"multi-sensor d {d}", MODES[:4])
    dev.close()


@pytest.mark.parametrize("d", [2, 4])
def test_loopy_parity_with_the_definition(hip_lib, d):
    model = AN.loopy(10, d)
    dev = _dev(model, L.SCHED_FUSED, 300, seed_variance=AN.LOOPY_SEED_VARIANCE)
    dev.residual()
    dev.sweep(2)
    assert dev.residual() <= 1e-12
    gm = E.gmodel(model)
    f2v, opq = E.device_messages(gm, dev)
    for mode, lag, m in (("predicted", 0, CS.PREDICTED), ("filtered", 0, CS.FILTERED), ("filtered", 2, CS.FILTERED)):
        got, want = dev.causal_marginals(mode, lag), CS.causal_from_messages(gm, f2v, opq, m, lag)
        got["variable_ids"] = gm.var_ids
        assert got["counts"] == want["counts"] and want["counts"]["finite"] >= 2 * 10 - 1
        print("loopy", d, mode, lag, CS.assert_close(got, want, PARITY, f"loopy d {d} {mode} lag {lag}"))
    dev.close()


@pytest.mark.parametrize("d", [1, 3])
def test_agreement_with_cx_predictive(hip_lib, d):
    """the PREDICTED row of x_t pushed through its observation factor, ŷ = H μ + b, S = H Σ H' + R, is the CX_PREDICT_CAUSAL row of that factor"""
    model = chain_of(d)
    dev = _dev(model, L.SCHED_CHAIN_SCAN)
    pre = dev.causal_marginals("predicted", 0, model.x_ids)
    cau = dev.predictive("causal", factor_ids=model.data_fac)
    s = MD.chain_spec(model)
    H, R = s["H"], s["R"]
    yh = np.einsum("ij,nj->ni", H, pre["mean"])
    S = np.einsum("ij,njk,lk->nil", H, pre["cov"], H) + R
    assert np.isnan(cau["mean"][0]).all() and np.isnan(yh[0]).all()
    assert P.scaled_err(yh, cau["mean"]) <= EXACT and P.scaled_err(S, cau["cov"]) <= EXACT
    dev.close()


def test_statuses(hip_lib):
    model = cx.synth.ssm_chain_linear(20, seed=81)
    dev = cx.DeviceGraph(schedule=L.SCHED_TREE)
    cx.synth.load_into_device(model, dev)
    res = dev.causal_marginals("filtered")            # before any sweep: every free row read an undefined message
    assert res["counts"] == {"rows": 40, "finite": 20, "undefined": 20, "improper": 0}, res["counts"]
    free = np.isin(np.arange(1, 41), model.x_ids)
    assert np.isnan(res["mean"][free]).all() and np.isnan(res["cov"][free]).all()
    assert np.array_equal(res["mean"][~free, 0], model.data_y) and not res["cov"][~free].any()      # an observed row: its datum and zeros
    dev.sweep(1)
    pre, flt = dev.causal_marginals("predicted"), dev.causal_marginals("filtered")
    assert pre["counts"] == {"rows": 40, "finite": 39, "undefined": 0, "improper": 1}, pre["counts"]      # no prior: the first state has no prediction
    assert np.isnan(pre["mean"][0]).all() and not np.isnan(flt["mean"]).any() and flt["counts"]["finite"] == 40
    for r in (pre, flt):
        assert r["counts"]["finite"] + r["counts"]["undefined"] + r["counts"]["improper"] == r["counts"]["rows"]
    dev.close()


def _bits(r):
    return r["mean"].tobytes() + r["cov"].tobytes()


@pytest.mark.parametrize("d,schedule", [(1, L.SCHED_TREE), (4, L.SCHED_CHAIN_SCAN)])
def test_independence_and_purity(hip_lib, d, schedule):
    model = chain_of(d, 40)
    dev = _dev(model, schedule)
    dev.causal_marginals("filtered", 2)               # (chain scan, dim 2..4: the chain messages go to their slots on the first read-out)
    blob = dev.export_state()
    for mode, lag in (("predicted", 0), ("filtered", 0), ("filtered", 5)):
        full, again = dev.causal_marginals(mode, lag), dev.causal_marginals(mode, lag)
        assert _bits(full) == _bits(again) and full["counts"] == again["counts"]
        pick = np.random.default_rng(3).permutation(80)[:23]
        sub = dev.causal_marginals(mode, lag, np.arange(1, 81)[pick])
        assert sub["mean"].tobytes() == full["mean"][pick].tobytes() and sub["cov"].tobytes() == full["cov"][pick].tobytes(), (mode, lag)
        assert sub["counts"]["rows"] == 23
    assert np.array_equal(blob, dev.export_state())
    twin = _dev(model, schedule)
    dev.sweep(1); twin.sweep(1)
    assert np.array_equal(dev.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE), twin.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE), equal_nan=True)
    assert np.array_equal(dev.get_marginals(model.x_ids), twin.get_marginals(model.x_ids), equal_nan=True)
    dev.close(); twin.close()


def test_cache_rules(hip_lib):
    model = chain_of(2, 20)
    dev = _dev(model, L.SCHED_CHAIN_SCAN)
    dev.causal_marginals("filtered", 3)
    other = MD.with_data(model, np.asarray(model.data_y) * 0.5 + 1.0)
    dev.set_messages(other.data_var, other.data_fac, L.TO_FACTOR, L.FORM_POINT, other.data_y)
    dev.sweep(1)
    fresh = _dev(other, L.SCHED_CHAIN_SCAN)
    for mode, lag in (("predicted", 0), ("filtered", 3)):
        assert _bits(dev.causal_marginals(mode, lag)) == _bits(fresh.causal_marginals(mode, lag)), (mode, lag)
    dev.close(); fresh.close()
    # a state's datum that arrives later: free (flat) when the plan is first built, observed afterwards — the plan follows the observed flags
    n = 16
    full = MD.make("gen", n, 2)
    thin = copy.copy(full)
    keep = np.ones(n, bool); keep[6] = False
    thin.data_var, thin.data_fac, thin.data_y = full.data_var[keep], full.data_fac[keep], np.asarray(full.data_y)[keep]
    dev = cx.DeviceGraph(dim=2, schedule=L.SCHED_TREE)
    cx.synth.load_into_device(thin, dev)
    dev.set_messages(full.data_var[~keep], full.data_fac[~keep], L.TO_FACTOR, L.FORM_NATURAL, np.zeros((1, 2 + 4)))      # flat: no datum yet
    dev.sweep(1)
    before = dev.causal_marginals("filtered", 0, full.x_ids)
    gap = dev.causal_marginals("predicted", 0, full.x_ids)
    assert before["counts"]["finite"] == n and before["mean"][6].tobytes() == gap["mean"][6].tobytes()
    dev.set_messages(full.data_var[~keep], full.data_fac[~keep], L.TO_FACTOR, L.FORM_POINT, np.asarray(full.data_y)[~keep])
    dev.sweep(1)
    _against_dense(full, dev, "after the datum arrived", MODES[:4])
    dev.close()


def test_refusals(hip_lib):
    dev = cx.DeviceGraph()
    assert code_of(dev.causal_marginals)[0] == L.ERR_STATE                      # no graph
    dev.close()
    dev = cx.DeviceGraph(family=L.FAMILY_NATURAL2)
    assert code_of(dev.causal_marginals)[0] == L.ERR_UNSUPPORTED
    dev.close()
    m16 = cx.synth.lgssm_chain(4, d=16, seed=91)
    dev = cx.DeviceGraph(dim=16, schedule=L.SCHED_FUSED)
    cx.synth.load_into_device(m16, dev, seed_variance=1e6)
    dev.sweep(2)
    assert code_of(dev.causal_marginals)[0] == L.ERR_UNSUPPORTED                # dim >= 5
    dev.close()
    n = 20
    model = cx.synth.ssm_chain(n, seed=92)
    dev = _dev(model, L.SCHED_FUSED, 5, seed_variance=1e6)
    cnt = (L.C.c_int64 * 4)()
    out = np.zeros((2 * n, 2))
    po = out.ctypes.data_as(L.C.POINTER(L.C.c_double))
    call = dev.lib.cx_causal_marginals
    assert call(dev.h, L.CAUSAL_FILTERED, 0, 0, None, po, cnt) == L.OK and cnt[0] == 2 * n
    assert call(dev.h, 2, 0, 0, None, po, cnt) == L.ERR_INVALID_ARGUMENT                      # unknown mode
    assert call(dev.h, L.CAUSAL_FILTERED, -1, 0, None, po, cnt) == L.ERR_INVALID_ARGUMENT     # negative lag
    assert call(dev.h, L.CAUSAL_PREDICTED, 1, 0, None, po, cnt) == L.ERR_INVALID_ARGUMENT     # a lag with PREDICTED
    assert call(dev.h, L.CAUSAL_FILTERED, 0, 0, None, None, cnt) == L.ERR_INVALID_ARGUMENT    # NULL out
    assert call(dev.h, L.CAUSAL_FILTERED, 0, 0, None, po, None) == L.ERR_INVALID_ARGUMENT     # NULL counts4
    ids = np.array([1, 2], np.int64)
    assert call(dev.h, L.CAUSAL_FILTERED, 0, -1, ids.ctypes.data_as(L.C.POINTER(L.C.c_int64)), po, cnt) == L.ERR_INVALID_ARGUMENT
    code, msg = code_of(lambda: dev.causal_marginals("filtered", 0, [1, 999]))
    assert code == L.ERR_NOT_FOUND and "999" in msg
    assert dev.causal_marginals("filtered", 2, [3, 1])["counts"]["finite"] == 2               # and the handle works on
    dev.halo_configure([1], [2 * n + 1], [], [])                                              # a halo list: a partitioned handle
    assert code_of(dev.causal_marginals)[0] == L.ERR_UNSUPPORTED
    dev.close()
    model = cx.synth.ssm_chain(10, seed=93, q=0.0)
    dev = cx.DeviceGraph(schedule=L.SCHED_TREE)
    cx.synth.load_into_device(model, dev)
    code, msg = code_of(dev.causal_marginals)
    assert code == L.ERR_UNSUPPORTED and "factor 31" in msg                   # zero noise: the first transition (ids 3T + 1 ..)
    dev.close()


def test_transitions_of_three_or_more_variables(hip_lib):
    d = 2
    model, prior, facs, fid, sets, _mean, _cov = _kary_tree(8, d, 52, k_choices=(2, 3))
    n = len(model.x_ids)
    edge_sets = {(int(model.x_ids[i]), int(f)): s for f, (_o, ins, ss, _q) in zip(fid, facs) for i, s in zip(ins, ss)}
    gm = E.gmodel(model, edge_sets=edge_sets, opaque=(model.x_ids, model.x_ids + n, prior[0], prior[1]))
    dev = _load_kary(model, prior, facs, fid, sets, L.SCHED_TREE)
    dev.sweep(1)
    code, msg = code_of(lambda: dev.causal_marginals("filtered", 1))
    assert code == L.ERR_UNSUPPORTED and f"factor {int(fid[0])}" in msg, msg
    f2v, opq = E.device_messages(gm, dev)
    for mode, m in (("predicted", CS.PREDICTED), ("filtered", CS.FILTERED)):                  # lag 0: such factors are simply classified
        got, want = dev.causal_marginals(mode), CS.causal_from_messages(gm, f2v, opq, m)
        got["variable_ids"] = gm.var_ids
        assert got["counts"] == want["counts"] and want["counts"]["finite"] == n
        print("k-ary", mode, CS.assert_close(got, want, PARITY, f"k-ary {mode}"))
    dev.close()
