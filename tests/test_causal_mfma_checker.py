"""CPU: the references of tests/test_gpu_causal_marginals_mfma.py agree with each other on the models those tests run.  On every forest
of predictive_mfma_support.forest_cases() the definition (causal_support.causal_from_messages on functional_support.forest_bp's exact
messages) and the dense solve without the data a mode leaves out (causal_support.dense_causal_all) agree to 1e-10 in assert_rows_close's
measure with equal statuses — measured: at most 2.3e-14 — for the predicted and filtered states and lags 1, 3 and 12, so that the GPU
tests can hold every row to the plain 1e-9; so do the Kalman filter and the fixed-lag smoother written as L Rauch-Tung-Striebel steps
back from the filtered state at t + L (causal_mfma_support.rts_lag; measured: 5e-15).

Known, and not to be "fixed": on clamped_middle the dense solve and the definition differ at lag 0 — causal_support.left_out does not
model the clamp.  Predicted: the first state's status differs; filtered: the means differ by about 0.5.  For that model the only
reference is the definition on the device's own messages; the difference is pinned below (from lag 1 on the two agree)."""
import numpy as np
import pytest

from tests import causal_mfma_support as CM
from tests import causal_support as CS
from tests import evidence_support as E
from tests import functional_support as F
from tests import predictive_mfma_support as PM

CASES = PM.forest_cases()
TOL = 1e-10


def _messages(name):
    model, opq = CASES[name]()
    gm = E.gmodel(model) if opq is None else E.gmodel(model, opaque=opq)
    return model, gm, F.forest_bp(gm)


def _free_status(gm, res):
    """the statuses of the states (the non-observed variables), in ascending id"""
    return res["status"][~gm.obs].tolist()


@pytest.mark.parametrize("name", sorted(CASES))
def test_definition_agrees_with_the_dense_solve(name):
    model, gm, f2v = _messages(name)
    n = int((~gm.obs).sum())
    for mode, lag, m in CM.MODES:
        what = f"{name} {mode} lag {lag}"
        got, dense = CS.causal_from_messages(gm, f2v, None, m, lag), CS.dense_causal_all(gm, m, lag)
        st = _free_status(gm, got)
        if name.startswith("clamped") and lag == 0:
            if m == CS.PREDICTED:      # the first state: no prediction by the definition, a proper marginal in the dense model
                assert st == [2] + [0] * (n - 1) and _free_status(gm, dense) == [0] * n, (what, st)
            else:
                with pytest.raises(AssertionError):
                    CS.assert_close(got, dense, 1e-3, what)
            continue
        assert np.array_equal(got["status"], dense["status"]) and got["counts"] == dense["counts"], (what, got["status"], dense["status"])
        print(what, CS.assert_close(got, dense, TOL, what))
        # the status patterns the GPU tests assert
        if name.startswith(("chain", "comb", "gen")):
            assert st == ([2] if m == CS.PREDICTED else [0]) + [0] * (n - 1), (what, st)
        elif name.startswith("leading gap"):
            assert st == ([2, 2, 0, 0, 0] if m == CS.PREDICTED else [2, 0, 0, 0, 0] if lag == 0 else [0] * 5), (what, st)
        else:
            assert st == [0] * n, (what, st)


@pytest.mark.parametrize("name", [k for k in sorted(CASES) if k.startswith(("chain", "gen"))])
def test_definition_agrees_with_the_kalman_filter_and_the_rts_form_of_the_lag(name):
    model, gm, f2v = _messages(name)
    s, f = CM.kalman(model)
    x = np.searchsorted(gm.var_ids, np.asarray(model.x_ids))
    pre = CS.causal_from_messages(gm, f2v, None, CS.PREDICTED, 0)
    assert np.isnan(pre["mean"][x[0]]).all()
    print(name, "predicted", CS.assert_close(CM.rows(pre["mean"][x[1:]], pre["cov"][x[1:]]), CM.rows(f["mp"][1:], f["Pp"][1:]), TOL, name + " predicted vs Kalman"))
    for lag in (0, 1, 2, 3, 12):
        got = CS.causal_from_messages(gm, f2v, None, CS.FILTERED, lag)
        ms, Ps = CM.rts_lag(s, f, lag)
        print(name, "lag", lag, CS.assert_close(CM.rows(got["mean"][x], got["cov"][x]), CM.rows(ms, Ps), TOL, f"{name} lag {lag} vs RTS"))


@pytest.mark.parametrize("d", CM.BRANCH_DIMS)
def test_a_state_with_four_sources_definition_agrees_with_the_dense_solve(d):
    model = CM.branching(d)
    gm = E.gmodel(model)
    f2v = F.forest_bp(gm)
    U, O, T = CS.classes(gm)
    x = np.searchsorted(gm.var_ids, np.asarray(model.x_ids))
    assert [len(O[v]) + len(T[v]) for v in x[1:4]] == [4, 4, 4] and all(len(U[v]) == 1 for v in x[1:4])      # the OUT ends of the root's transitions
    for mode, lag, m in CM.BRANCH_MODES:
        what = f"branching d {d} {mode} lag {lag}"
        got, dense = CS.causal_from_messages(gm, f2v, None, m, lag), CS.dense_causal_all(gm, m, lag)
        assert got["counts"] == dense["counts"] and got["counts"]["finite"] == len(gm.var_ids), (what, got["counts"], dense["counts"])
        print(what, CS.assert_close(got, dense, TOL, what))


def test_a_state_with_two_parents_is_the_out_end_of_two_transitions():
    model = CM.two_parents(16)
    gm = E.gmodel(model)
    U, O, T = CS.classes(gm)
    x = np.searchsorted(gm.var_ids, np.asarray(model.x_ids))
    assert len(U[x[1]]) == 2 and len(O[x[1]]) + len(T[x[1]]) == 4 and len(T[x[0]]) == 3 and len(T[x[13]]) == 1
    got = CS.causal_from_messages(gm, F.forest_bp(gm), None, CS.FILTERED, 3)
    assert got["counts"]["finite"] == len(gm.var_ids)
