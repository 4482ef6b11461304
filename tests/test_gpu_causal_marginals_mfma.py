"""-m gpu: cx_causal_marginals_mfma — the predicted, filtered and fixed-lag-smoothed states at the matrix-core dims (cx_create dim
5 .. 64) — against the dense solve without the data a mode leaves out, the Kalman filter, the fixed-lag smoother as L
Rauch-Tung-Striebel steps back from the filtered state at t + L, and the numpy restatement of the definition on the device's own
messages (tests/causal_support.py, tests/causal_mfma_support.py; the models are those of tests/predictive_mfma_support.py; the
references are pinned against each other on the CPU by tests/test_causal_mfma_checker.py: at most 2.3e-14 apart).

Tolerances: TOL = 1e-9 against the exact references, the project's tolerance for this arithmetic class (tests/test_gpu_predictive_mfma.py,
tests/test_gpu_causal_marginals.py) and more than 1e4 times the floor above; 1e-12 between tile sizes.  Rows are compared by
predictive_support.assert_rows_close (vectors and matrices scaled by their largest entry; the NaN patterns must agree)."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from tests import causal_mfma_support as CM
from tests import causal_support as CS
from tests import evidence_mfma_support as S
from tests import evidence_support as E
from tests import missing_data as MD
from tests import predictive_mfma_support as PM
from tests import predictive_support as P
from tests.gpu_support import (HANDLE_CASES, STREAM_CASES, assert_reader_refusals, code_of, demo_chain, missing_data_device, run_demo,
                               swept_device, under_capture, with_sets)

pytestmark = pytest.mark.gpu
TOL = 1e-9
WHO = "cx_causal_marginals_mfma"


def _all(dev, gm, mode, lag):
    """every variable of the handle, labelled as the references label them"""
    got = dev.causal_marginals_mfma(mode, lag)
    assert got["variable_ids"] is None and len(got["mean"]) == len(gm.var_ids)
    got["variable_ids"] = gm.var_ids
    return got


def _close(got, want, what, tol=TOL, pick=None):
    errs = CS.assert_close(got, want, tol, what, pick)
    print(what, errs)
    return errs


def _bits(r):
    return r["mean"].tobytes() + r["cov"].tobytes()


def _x(gm, model):
    return np.searchsorted(gm.var_ids, np.asarray(model.x_ids))


def _definition(gm, dev, m, lag):
    f2v, opq = E.device_messages(gm, dev)
    return CS.causal_from_messages(gm, f2v, opq, m, lag)


def _against_kalman(dev, model, what, lags=(2,)):
    """the states of a chain: predicted and filtered against the Kalman filter, the lags against the RTS form"""
    s, f = CM.kalman(model)
    n = len(model.x_ids)
    pre, flt = dev.causal_marginals_mfma("predicted", 0, model.x_ids), dev.causal_marginals_mfma("filtered", 0, model.x_ids)
    assert pre["counts"] == {"rows": n, "finite": n - 1, "undefined": 0, "improper": 1} and np.isnan(pre["mean"][0]).all() and np.isnan(pre["cov"][0]).all(), pre["counts"]
    assert flt["counts"] == {"rows": n, "finite": n, "undefined": 0, "improper": 0}, flt["counts"]
    _close(pre, CM.rows(f["mp"], f["Pp"], model.x_ids), what + " predicted vs Kalman", pick=slice(1, None))
    _close(flt, CM.rows(f["mf"], f["Pf"], model.x_ids), what + " filtered vs Kalman")
    for lag in lags:
        got = dev.causal_marginals_mfma("filtered", lag, model.x_ids)
        assert got["counts"]["finite"] == n
        _close(got, CM.rows(*CM.rts_lag(s, f, lag), model.x_ids), f"{what} lag {lag} vs RTS")


# ---- 1. chains and combs after every schedule ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["chain", "comb"])
@pytest.mark.parametrize("d", PM.SCHEDULE_DIMS)
def test_chains_and_combs_after_every_schedule(hip_lib, d, shape):
    model = PM.chain(d) if shape == "chain" else PM.comb(d)
    gm = E.gmodel(model)
    dense = {(mode, lag): CS.dense_causal_all(gm, m, lag) for mode, lag, m in CM.MODES}
    x = _x(gm, model)
    for s in [L.SCHED_TREE, L.SCHED_REFERENCE, L.SCHED_FUSED] + ([L.SCHED_CHAIN_SCAN] if shape == "chain" else []):
        what = f"d {d} {shape} schedule {s}"
        dev = swept_device(model, s)      # (fused: seed variance 1e6 and 60 sweeps, the diameter is under 20)
        for mode, lag, _m in CM.MODES:
            got, want = _all(dev, gm, mode, lag), dense[(mode, lag)]
            assert got["counts"] == want["counts"], (what, mode, lag, got["counts"], want["counts"])
            _close(got, want, f"{what} {mode} lag {lag} vs dense")
        assert CM.status_of(_all(dev, gm, "predicted", 0))[x].tolist() == [2] + [0] * (len(x) - 1)      # exactly the first state has no prediction
        if shape == "chain":
            _against_kalman(dev, model, what, lags=())
        lagged, marg = dev.causal_marginals_mfma("filtered", 12, model.x_ids), dev.get_marginals(model.x_ids)
        _close(lagged, CM.rows(marg[:, :d], marg[:, d:].reshape(-1, d, d), model.x_ids), what + " lag 12 vs get_marginals")
        dev.close()


# ---- 2. gaps and a forecast tail ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", PM.GEN_DIMS)
def test_gaps_and_a_forecast_tail(hip_lib, d):
    model = PM.gen(d)
    gm = E.gmodel(model)
    dev = missing_data_device(model)
    for mode, lag, m in CM.MODES:
        got, want = _all(dev, gm, mode, lag), CS.dense_causal_all(gm, m, lag)
        assert got["counts"] == want["counts"], (mode, lag, got["counts"], want["counts"])
        _close(got, want, f"gen d {d} {mode} lag {lag} vs dense")
    # from the last datum on nothing downstream has been seen: β is exactly zero, so a lag changes no bit
    last = int(np.flatnonzero(MD.chain_spec(model)["keep"]).max())
    assert last < len(model.x_ids) - 1
    behind = np.asarray(model.x_ids)[last:]
    assert _bits(dev.causal_marginals_mfma("filtered", 3, behind)) == _bits(dev.causal_marginals_mfma("filtered", 0, behind))
    dev.close()


# ---- 3. a leading gap: the flat-pivot rule ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", PM.GEN_DIMS)
def test_a_leading_gap(hip_lib, d):
    model = PM.leading_gap(d)
    gm = E.gmodel(model)
    x = _x(gm, model)
    dev = missing_data_device(model)
    pattern = {("predicted", 0): [2, 2, 0, 0, 0], ("filtered", 0): [2, 0, 0, 0, 0]}      # lag >= 1: none
    for mode, lag, m in CM.MODES:
        got = _all(dev, gm, mode, lag)
        st = pattern.get((mode, lag), [0] * 5)
        assert CM.status_of(got)[x].tolist() == st, (d, mode, lag, CM.status_of(got)[x])
        assert got["counts"] == {"rows": len(gm.var_ids), "finite": len(gm.var_ids) - sum(st) // 2, "undefined": 0, "improper": sum(st) // 2}, got["counts"]
        # values: the definition on the device's own messages, on the rows the rule lets through (the reference has no flat-pivot
        # rule: on a message that is the rounding of a difference its Cholesky may pass or not)
        _close(got, _definition(gm, dev, m, lag), f"leading gap d {d} {mode} lag {lag} vs the definition on the device's messages", pick=~np.isnan(got["mean"]).any(axis=1))
    dev.close()


# ---- 4. a proper opaque prior ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", PM.PRIOR_DIMS)
def test_an_opaque_prior_gives_every_state_a_prediction(hip_lib, d):
    model, opq = S.prior_chain(d)
    gm = E.gmodel(model, opaque=opq)
    dev = cx.DeviceGraph(dim=d, schedule=L.SCHED_TREE)
    cx.synth.load_into_device(model, dev)
    S.set_opaque(dev, opq)
    dev.sweep(1)
    for mode, lag, m in CM.MODES:
        got, want = _all(dev, gm, mode, lag), CS.dense_causal_all(gm, m, lag)
        assert got["counts"] == want["counts"] and got["counts"]["finite"] == len(gm.var_ids), (mode, lag, got["counts"])
        _close(got, want, f"prior d {d} {mode} lag {lag} vs dense")
    dev.close()


# ---- 5. a clamped state in the middle --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", PM.CLAMPED_DIMS)
def test_a_clamped_state_in_the_middle(hip_lib, d):
    model = S.clamped_middle(d)
    gm = E.gmodel(model)
    x = _x(gm, model)
    c = x[model.meta["clamped_state"]]
    dev = swept_device(model, L.SCHED_TREE)
    for mode, lag, m in CM.MODES:
        got, want = _all(dev, gm, mode, lag), _definition(gm, dev, m, lag)
        assert got["counts"] == want["counts"], (mode, lag, got["counts"], want["counts"])
        _close(got, want, f"clamped middle d {d} {mode} lag {lag} vs the definition on the device's messages")
        assert np.array_equal(got["mean"][c], gm.y[c]) and not got["cov"][c].any()      # its datum and zeros
    dev.close()


# ---- 6. a loop -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", S.RING_DIMS)
def test_a_loop_matches_the_definition_on_the_device_messages(hip_lib, d):
    model = S.ring(d)
    gm = E.gmodel(model)
    dev = swept_device(model, L.SCHED_FUSED, S.RING_SWEEPS)
    for mode, lag, m in (("predicted", 0, CS.PREDICTED), ("filtered", 0, CS.FILTERED), ("filtered", 1, CS.FILTERED), ("filtered", 3, CS.FILTERED)):
        got, again = _all(dev, gm, mode, lag), _all(dev, gm, mode, lag)
        want = _definition(gm, dev, m, lag)
        assert got["counts"] == want["counts"] and got["counts"]["undefined"] == 0 and got["counts"]["improper"] == 0, (mode, lag, got["counts"], want["counts"])
        _close(got, want, f"ring d {d} {mode} lag {lag}")
        assert _bits(got) == _bits(again) and got["counts"] == again["counts"]      # two calls on one state: bit-identical
    dev.close()


# ---- 7. embedded dims ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [8, 20])
def test_embedded_dims_give_the_real_models_rows_at_any_tile_size(hip_lib, d, monkeypatch):
    model = cx.synth.lgssm_chain(5, d=d, seed=90 + d)
    dev = swept_device(model, L.SCHED_TREE)
    native = {lag: dev.causal_marginals_mfma("filtered", lag) for lag in (0, 2)}
    dev.close()
    monkeypatch.setenv("CX_MFMA_DIM", "64")
    dev = swept_device(model, L.SCHED_TREE)
    monkeypatch.delenv("CX_MFMA_DIM")
    for lag in (0, 2):
        forced = dev.causal_marginals_mfma("filtered", lag)
        _close(forced, native[lag], f"d {d} lag {lag}: 4 x 4 tiles against the native tile", tol=1e-12)
        assert forced["counts"] == native[lag]["counts"] and forced["counts"]["finite"] == 10
    dev.close()


# ---- 8. undefined inputs; new parameters -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [8, 32])
def test_undefined_then_exact_then_new_parameters(hip_lib, d):
    T = 7
    model = cx.synth.lgssm_chain(T, d=d, seed=81 + d)
    gm = E.gmodel(model)
    dev = cx.DeviceGraph(dim=d, schedule=L.SCHED_TREE)
    cx.synth.load_into_device(model, dev)
    for mode, lag in (("predicted", 0), ("filtered", 0), ("filtered", 2)):      # before any sweep
        r = _all(dev, gm, mode, lag)
        assert r["counts"] == {"rows": 2 * T, "finite": T, "undefined": T, "improper": 0}, (mode, lag, r["counts"])
        assert np.isnan(r["mean"][~gm.obs]).all() and np.isnan(r["cov"][~gm.obs]).all()
        assert np.array_equal(r["mean"][gm.obs], gm.y[gm.obs]) and not r["cov"][gm.obs].any()      # an observed row: its datum and zeros
    psets = dict(model.psets)
    first = None
    for step in ("old (A, Q)", "new (A, 2 Q)", "new (H, 2 R)"):
        if step == "new (A, 2 Q)":
            psets[0] = (psets[0][0], 2.0 * np.asarray(psets[0][1]))
            dev.set_factor_matrices(0, *psets[0])
        if step == "new (H, 2 R)":
            psets[1] = (psets[1][0], 2.0 * np.asarray(psets[1][1]))
            dev.set_factor_matrices(1, *psets[1])
        dev.sweep(1)
        _against_kalman(dev, with_sets(model, psets), f"d {d} {step}")      # the rule tables are read by every call
        lag2 = dev.causal_marginals_mfma("filtered", 2, model.x_ids)
        if first is not None:
            assert np.abs(lag2["cov"][1] - first["cov"][1]).max() > 1e-3
        first = lag2
    dev.close()


# ---- 9. named rows -----------------------------------------------------------------------------------------------------------------------
def test_named_rows_in_the_callers_order(hip_lib):
    d, T = 16, 9
    model = cx.synth.lgssm_chain(T, d=d, seed=83)
    gm = E.gmodel(model)
    dev = swept_device(model, L.SCHED_TREE)
    for mode, lag, m in (("predicted", 0, CS.PREDICTED), ("filtered", 0, CS.FILTERED), ("filtered", 2, CS.FILTERED)):
        full = _all(dev, gm, mode, lag)
        want = CS.dense_causal_all(gm, m, lag)
        for pick in ([7, 2, 16, 5, 0], [1, 8, 12]):       # (the second list: another request, the plan is rebuilt; 16, 12: observed variables)
            sub = dev.causal_marginals_mfma(mode, lag, gm.var_ids[pick])
            assert np.array_equal(sub["variable_ids"], gm.var_ids[pick]) and sub["counts"]["rows"] == len(pick)
            assert sub["mean"].tobytes() == full["mean"][pick].tobytes() and sub["cov"].tobytes() == full["cov"][pick].tobytes(), (mode, lag, pick)
            _close(sub, {k: want[k][pick] for k in ("variable_ids", "mean", "cov")}, f"named rows {mode} lag {lag} {pick} vs dense")
    # clamping a state between two calls: the plan follows the observed flags
    i = 4
    x = model.x_ids[i]
    facs = np.asarray(model.edge_fac)[np.asarray(model.edge_var) == x]
    value = np.random.default_rng(84).standard_normal(d)
    before = dev.causal_marginals_mfma("filtered", 2, model.x_ids)
    dev.set_messages(np.full(len(facs), x), facs, L.TO_FACTOR, L.FORM_POINT, np.tile(value, (len(facs), 1)))
    dev.sweep(1)
    clamped = dataclasses.replace(model, data_var=np.concatenate([model.data_var, np.full(len(facs), x)]), data_fac=np.concatenate([model.data_fac, facs]),
                                  data_y=np.vstack([model.data_y, np.tile(value, (len(facs), 1))]))
    gc = E.gmodel(clamped)
    for mode, lag, m in (("predicted", 0, CS.PREDICTED), ("filtered", 2, CS.FILTERED)):
        got = dev.causal_marginals_mfma(mode, lag, model.x_ids)
        want = _definition(gc, dev, m, lag)
        _close(got, {k: want[k][_x(gc, model)] for k in ("variable_ids", "mean", "cov")}, f"after the clamp {mode} lag {lag} vs the definition on the device's messages")
        assert np.array_equal(got["mean"][i], value) and not got["cov"][i].any()
    assert np.abs(got["mean"][i - 1] - before["mean"][i - 1]).max() > 1e-3
    dev.close()


# ---- 10. more rows than resident waves and than one payload chunk -------------------------------------------------------------------------
@pytest.mark.parametrize("T,d", [(2500, 64), (20000, 16)])
def test_long_chains_against_the_kalman_filter(hip_lib, T, d):
    model = cx.synth.lgssm_chain(T, d=d, seed=33)
    assert T * (d + d * d) * 8 > 32 << 20      # more than one chunk of the payload
    dev = swept_device(model, L.SCHED_CHAIN_SCAN)
    _against_kalman(dev, model, f"d = {d}, T = {T}, chain scan")
    dev.close()


# ---- 11. agreement with predictive_mfma("causal") ------------------------------------------------------------------------------------------
def test_agreement_with_predictive_mfma(hip_lib):
    """the PREDICTED row of x_t pushed through its observation factor, ŷ = H μ, S = H Σ H' + R, is the CX_PREDICT_CAUSAL row of that factor"""
    model = PM.gen(16)
    dev = missing_data_device(model)
    s = MD.chain_spec(model)
    steps = np.flatnonzero(s["keep"])
    pre = dev.causal_marginals_mfma("predicted", 0, np.asarray(model.x_ids)[steps])
    cau = dev.predictive_mfma("causal", factor_ids=s["lik"][steps])
    H = s["H"]
    yh = np.einsum("ij,nj->ni", H, pre["mean"])
    Sm = np.einsum("ij,njk,lk->nil", H, pre["cov"], H) + s["R"][steps]
    assert np.isnan(cau["mean"][0]).all() and np.isnan(yh[0]).all() and not np.isnan(yh[1:]).any()
    errs = (P.scaled_err(yh, cau["mean"]), P.scaled_err(Sm, cau["cov"]))
    print("agreement with predictive_mfma", errs)
    assert max(errs) <= TOL, errs
    dev.close()


# ---- 12. moves nothing -------------------------------------------------------------------------------------------------------------------
def test_moves_nothing(hip_lib):
    model = cx.synth.lgssm_chain(8, d=16, seed=72)
    for s in (L.SCHED_CHAIN_SCAN, L.SCHED_REFERENCE, L.SCHED_TREE):
        dev = swept_device(model, s)
        if s == L.SCHED_CHAIN_SCAN:      # (another reader first: every reader of the messages brings them to their slots)
            dev.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE)
        blob, marg = dev.export_state(), dev.get_marginals(model.x_ids)
        dev.causal_marginals_mfma("filtered", 3)      # the FIRST call: it builds the rows and allocates β
        assert np.array_equal(blob, dev.export_state())
        assert np.array_equal(marg, dev.get_marginals(model.x_ids))
        dev.causal_marginals_mfma("predicted")
        assert np.array_equal(blob, dev.export_state())
        dev.close()
    # fused: the next sweeps are those of a twin handle that never called it, bit for bit
    a, b = swept_device(model, L.SCHED_FUSED, 5), swept_device(model, L.SCHED_FUSED, 5)
    assert a.residual() == b.residual()      # (the first call takes the snapshot the next one measures against)
    a.causal_marginals_mfma("predicted"); a.causal_marginals_mfma("filtered", 2)
    a.sweep(3); b.sweep(3)
    ra, rb = a.residual(), b.residual()
    assert math.isfinite(ra) and ra == rb, (ra, rb)
    assert np.array_equal(a.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE), b.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE),
                          equal_nan=True)      # (the messages into the observed variables are never computed)
    assert np.array_equal(a.get_marginals(model.x_ids), b.get_marginals(model.x_ids))
    a.close(); b.close()


# ---- 13. refusals ------------------------------------------------------------------------------------------------------------------------
def _raw(dev, out):
    """the filtered states at lag 1 of every variable through the C ABI, into out [n_variables, d + d d]; the status"""
    return dev.lib.cx_causal_marginals_mfma(dev.h, L.CAUSAL_FILTERED, 1, 0, None, out.ctypes.data_as(C.POINTER(C.c_double)), (C.c_int64 * 4)())


_COMMON = dict(who=WHO, small="cx_causal_marginals", call=lambda dev: dev.causal_marginals_mfma(), small_call=lambda dev: dev.causal_marginals(),
               raw=lambda dev: _raw(dev, np.zeros((8, 16 + 256))))      # what assert_reader_refusals asks of this reader


def test_refusals(hip_lib):
    assert_reader_refusals(**_COMMON, cases=HANDLE_CASES)
    m16 = cx.synth.lgssm_chain(4, d=16, seed=92)
    dev = swept_device(m16, L.SCHED_FUSED, 2)
    code, msg = code_of(dev.causal_marginals)
    assert code == L.ERR_UNSUPPORTED and "cx_causal_marginals" in msg and WHO not in msg      # the old call refuses under its own name
    n = 8
    out, c4 = np.zeros((n, 16 + 256)), (C.c_int64 * 4)()
    po = out.ctypes.data_as(C.POINTER(C.c_double))
    ids = (C.c_int64 * 1)(int(m16.x_ids[0]))
    call = dev.lib.cx_causal_marginals_mfma
    assert call(dev.h, L.CAUSAL_FILTERED, 0, 0, None, po, c4) == L.OK and list(c4) == [n, n, 0, 0]
    for args, text in (((2, 0, 0, None, po, c4), "mode is"), ((L.CAUSAL_FILTERED, -1, 0, None, po, c4), "negative lag"),
                       ((L.CAUSAL_PREDICTED, 1, 0, None, po, c4), "a lag goes with CX_CAUSAL_FILTERED"), ((L.CAUSAL_FILTERED, 0, 0, None, None, c4), "null argument"),
                       ((L.CAUSAL_FILTERED, 0, 0, None, po, None), "null argument"), ((L.CAUSAL_FILTERED, 0, -1, ids, po, c4), "negative count")):
        assert call(dev.h, *args) == L.ERR_INVALID_ARGUMENT, args
        assert dev.lib.cx_last_error(dev.h).decode().startswith(WHO) and text in dev.lib.cx_last_error(dev.h).decode()
    code, msg = code_of(dev.causal_marginals_mfma, "filtered", 0, [int(m16.x_ids[0]), 10 ** 9])
    assert code == L.ERR_NOT_FOUND and msg.startswith(WHO) and str(10 ** 9) in msg
    assert dev.causal_marginals_mfma("filtered", 2, [int(m16.x_ids[2]), int(m16.x_ids[0])])["counts"]["finite"] == 2      # and the handle works on
    dev.close()


def test_no_factor_of_another_kind_enters_a_handle_of_these_dims(hip_lib):
    """The issue's refusal of "any other factor kind" (prm::checked_pairs under this function's name) is a guard: cx_graph_create admits
    nothing but two-variable CX_FACTOR_GAUSS_LINEAR factors and opaque ones at dim 5 .. 64, so no graph reaches it through the API."""
    m = cx.synth.lgssm_chain(3, d=16, seed=94)
    three = (np.array([1, 2, 3], np.int64), np.array([99, 99, 99], np.int64), np.array([L.ROLE_IN, L.ROLE_IN, L.ROLE_OUT], np.int32))
    two = (np.array([1, 3], np.int64), np.array([99, 99], np.int64), np.array([L.ROLE_IN, L.ROLE_OUT], np.int32))
    for kind, (ev, ef, er) in ((L.FACTOR_GAUSS_LINEAR_N, three), (L.FACTOR_GAUSS_LINEAR, three), (L.FACTOR_GAUSS_ADDITIVE, two), (L.FACTOR_NORMAL_PRECISION, three)):
        dev = cx.DeviceGraph(dim=16, schedule=L.SCHED_TREE)
        for k, (A, Q) in m.psets.items():
            dev.set_factor_matrices(k, A, Q)
        code, msg = code_of(dev.graph_create, np.concatenate([m.edge_var, ev]), np.concatenate([m.edge_fac, ef]), np.concatenate([m.factor_ids, [99]]),
                          np.concatenate([m.factor_kind, [kind]]).astype(np.int32), np.concatenate([m.factor_var, [0.0]]),
                          edge_role=np.concatenate([m.edge_role, er]).astype(np.int32))
        assert code == L.ERR_UNSUPPORTED and msg.startswith("cx_graph_create"), (kind, code, msg)
        dev.close()


def test_refusals_of_a_captured_stream_and_of_parameter_sets_never_set(hip_lib):
    assert_reader_refusals(**_COMMON, cases=STREAM_CASES)
    d = 16
    model = cx.synth.lgssm_chain(5, d=d, seed=93)
    dev = swept_device(model, L.SCHED_TREE)
    want = dev.causal_marginals_mfma("filtered", 1)
    out = np.zeros((10, d + d * d))
    rc, msg = under_capture(dev, lambda: _raw(dev, out))
    assert rc == L.ERR_STATE and msg.startswith(WHO) and "captured" in msg, (rc, msg)
    assert not out.any()                                       # nothing was written
    got = dev.causal_marginals_mfma("filtered", 1)             # and the handle works on, bit for bit
    assert _bits(got) == _bits(want) and got["counts"] == want["counts"]
    dev.close()


# ---- 14. the C++ host class --------------------------------------------------------------------------------------------------------------
def test_cpp_host_class_causal_marginals_mfma(hip_lib, tmp_path):
    lines = [line.split() for line in run_demo("causal_mfma_demo", tmp_path)]
    head = {ln[0]: ln[1:] for ln in lines if ln[0] != "row"}
    rows = [[float(v) for v in ln[2:]] for ln in lines if ln[0] == "row"]
    T, d = 12, 16
    A, Q, R, y = demo_chain(T, d)
    s = dict(A=np.broadcast_to(A, (T - 1, d, d)), b=np.zeros((T - 1, d)), Q=np.broadcast_to(Q, (T - 1, d, d)), H=np.eye(d),
             R=np.broadcast_to(R, (T, d, d)), y=y, keep=np.ones(T, bool))
    f = MD.kalman_filter(s["A"], s["b"], s["Q"], s["H"], s["R"], s["y"], s["keep"])
    ms, Ps = CM.rts_lag(s, f, 2)
    assert head["before"] == [str(T), "0", str(T), "0"] and head["all"] == [str(2 * T)] * 2 + ["0", "0"]
    assert head["predicted"] == [str(T), str(T - 1), "0", "1"] and head["filtered"] == [str(T), str(T), "0", "0"] and head["lag2"] == head["filtered"]
    assert len(rows) == T and all(math.isnan(v) for v in rows[0][:5])
    for t in range(T):
        want = [w for m, Pm in ((f["mp"], f["Pp"]), (f["mf"], f["Pf"]), (ms, Ps)) for w in (m[t][0], m[t][d - 1], Pm[t][0, 0], Pm[t][1, 0], Pm[t][d - 1, d - 1])]
        for k, (g, w) in enumerate(zip(rows[t], want)):
            assert (t == 0 and k < 5) or abs(g - w) <= TOL * max(abs(w), 1.0), (t, k, g, w)


# ---- 15. more than three sources: the summed record ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", CM.BRANCH_DIMS)
def test_a_state_with_four_sources_goes_through_the_summed_record(hip_lib, d):
    """the three states below the root have their datum and three transitions onward: the rule towards the root takes their sum from the
    scratch record (k_cmm_presum); from lag 2 on that sum reads the β of the other buffer"""
    model = CM.branching(d)
    gm = E.gmodel(model)
    dev = swept_device(model, L.SCHED_TREE)
    for mode, lag, m in CM.BRANCH_MODES:
        got, want = _all(dev, gm, mode, lag), CS.dense_causal_all(gm, m, lag)
        assert got["counts"] == want["counts"] and got["counts"]["finite"] == len(gm.var_ids), (d, mode, lag, got["counts"], want["counts"])
        _close(got, want, f"branching d {d} {mode} lag {lag} vs dense")
    sub, full = dev.causal_marginals_mfma("filtered", 2, model.x_ids[:1]), dev.causal_marginals_mfma("filtered", 2, model.x_ids)
    assert sub["mean"].tobytes() == full["mean"][:1].tobytes() and sub["cov"].tobytes() == full["cov"][:1].tobytes()      # the root alone: every transition is still walked
    dev.close()


@pytest.mark.parametrize("d", [16, 64])
def test_two_transitions_out_of_one_state_share_its_summed_record(hip_lib, d):
    """a state with two parents is the OUT end of two transitions, whose entries name ONE summed record; the reference is the definition on
    the device's own messages (causal_mfma_support.two_parents says why the dense solve is none)"""
    model = CM.two_parents(d)
    gm = E.gmodel(model)
    dev = swept_device(model, L.SCHED_TREE)
    for mode, lag, m in CM.BRANCH_MODES:
        got, want = _all(dev, gm, mode, lag), _definition(gm, dev, m, lag)
        assert got["counts"] == want["counts"] and got["counts"]["finite"] == len(gm.var_ids), (d, mode, lag, got["counts"], want["counts"])
        _close(got, want, f"two parents d {d} {mode} lag {lag} vs the definition on the device's messages")
    dev.close()
