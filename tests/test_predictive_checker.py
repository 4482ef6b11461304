"""CPU checks of the statements the predictive-score tests compare cx_predictive against (tests/predictive_support.py): the numpy
restatement of the formula from messages is proved against the dense leave-one-out solve and against the Kalman innovations, on exact
messages from evidence_support.numpy_bp.  They pin the helpers before any GPU run."""
import numpy as np
import pytest

import cortex.jl_amd as cx
from tests import evidence_support as E
from tests import predictive_support as P

CHAINS = [("ssm_chain", lambda: cx.synth.ssm_chain(14, seed=3, random_variances=True)),
          ("ssm_chain_linear", lambda: cx.synth.ssm_chain_linear(14, seed=5)),
          ("lgssm_d2", lambda: cx.synth.lgssm_chain(10, d=2, seed=6)),
          ("lgssm_d3", lambda: cx.synth.lgssm_chain(9, d=3, seed=7)),
          ("lgssm_d4", lambda: cx.synth.lgssm_chain(8, d=4, seed=8))]


@pytest.mark.parametrize("name,make", CHAINS, ids=[c[0] for c in CHAINS])
def test_chains_loo_is_the_dense_solve_and_causal_is_the_kalman_filter(name, make):
    model = make()
    T = model.meta["T"]
    gm = E.gmodel(model)
    f2v = E.numpy_bp(gm)
    loo = P.predictive_from_messages(gm, f2v, mode=P.LOO)
    assert loo["counts"] == {"rows": T, "scored": T, "undefined": 0, "improper": 0}
    P.assert_rows_close(loo, P.dense_loo_all(gm), 1e-10, name + " loo")
    cau = P.predictive_from_messages(gm, f2v, mode=P.CAUSAL)
    assert cau["counts"] == {"rows": T, "scored": T - 1, "undefined": 0, "improper": 1}
    yh, S, term, maha = P.innovations_of_chain(model)
    kal = {"factor_ids": cau["factor_ids"], "mean": yh, "cov": S, "log_density": term, "mahalanobis": maha}
    P.assert_rows_close(cau, kal, 1e-10, name + " causal")
    want = E.kalman_of_chain(model)
    assert abs(np.nansum(term) - want) <= 1e-12 * abs(want)                 # the innovations are those of kalman_log_lik's recursion
    assert abs(cau["total"] - want) <= 1e-10 * abs(want)
    assert abs(cau["total"] - E.dense_log_z(gm)) <= 1e-10 * abs(want)


def test_tree_with_observed_kary_factors_loo_is_the_dense_solve():
    model = cx.synth.tree_model(120, seed=23, k_choices=(1, 2, 3, 5, 6), observe=0.25)
    gm = E.gmodel(model)
    rows = P.rows_of(gm)
    assert sum(1 for r in rows if r[1] == 2) >= 2 and sum(1 for r in rows if r[1] > 2) >= 2, rows      # pairwise and k-ary rows
    loo = P.predictive_from_messages(gm, E.numpy_bp(gm), mode=P.LOO)
    assert loo["counts"]["scored"] == len(rows)
    P.assert_rows_close(loo, P.dense_loo_all(gm), 1e-10, "tree loo")


@pytest.mark.parametrize("d", [2, 4])
def test_comb_loo_is_the_dense_solve_and_causal_conditions_on_ancestors(d):
    model = cx.synth.lgssm_comb(5, d=d, teeth=1, seed=40 + d)
    gm = E.gmodel(model)
    f2v = E.numpy_bp(gm)
    loo = P.predictive_from_messages(gm, f2v, mode=P.LOO)
    assert loo["counts"]["scored"] == loo["counts"]["rows"] == 10
    P.assert_rows_close(loo, P.dense_loo_all(gm), 1e-10, "comb loo")
    # a branching graph: every row conditions on the data of its state's ancestors only; the root's row is improper and the sum
    # is not the evidence (the teeth's data are never conditioned on by the spine)
    cau = P.predictive_from_messages(gm, f2v, mode=P.CAUSAL)
    assert cau["counts"]["improper"] == 1 and cau["counts"]["scored"] == 9
    assert abs(cau["total"] - E.dense_log_z(gm)) > 1e-3


def test_undefined_and_improper_rows_are_told_apart():
    model = cx.synth.ssm_chain(10, seed=1)
    gm = E.gmodel(model)
    res = P.predictive_from_messages(gm, E.numpy_bp(gm, max_iter=2), mode=P.LOO)      # the middle of the chain is not reached yet
    assert res["counts"]["undefined"] > 0 and res["counts"]["improper"] == 0
    assert np.isnan(res["log_density"][res["status"] == 1]).all()
    one = cx.synth.ssm_chain(1, seed=2)                                              # one state, no prior: nothing else to predict from
    g1 = E.gmodel(one)
    res = P.predictive_from_messages(g1, E.numpy_bp(g1), mode=P.LOO)
    assert res["counts"] == {"rows": 1, "scored": 0, "undefined": 0, "improper": 1}
    assert P.dense_loo(g1, int(res["factor_ids"][0])) is None


@pytest.mark.parametrize("seed", [3, 6, 10, 13, 17])
def test_a_cavity_with_no_message_left_is_improper_by_structure(seed):
    # on these chains (M - m_lik) - m_transition at x_1 rounds to a tiny POSITIVE precision, not to 0: the first causal row is improper
    # because no message is left in its cavity, not because a difference happens to vanish
    model = cx.synth.ssm_chain_linear(6, seed=seed)
    gm = E.gmodel(model)
    f2v = E.numpy_bp(gm)
    v = int(np.searchsorted(gm.var_ids, 1))
    lam = [f2v[2][1][fi, j, 0, 0] for fi in range(len(gm.groups[2]["fid"])) for j in range(2) if gm.groups[2]["vars"][fi, j] == v]
    assert len(lam) == 2 and max((lam[0] + lam[1]) - lam[0] - lam[1], (lam[0] + lam[1]) - lam[1] - lam[0]) > 0
    cau = P.predictive_from_messages(gm, f2v, mode=P.CAUSAL)
    assert cau["counts"] == {"rows": 6, "scored": 5, "undefined": 0, "improper": 1} and cau["status"][0] == 2
    want = E.kalman_of_chain(model)
    assert abs(cau["total"] - want) <= 1e-10 * abs(want)
