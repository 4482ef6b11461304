"""CPU: the inputs of tests/test_gpu_predictive_mfma.py are what those tests take them for.  On every forest of
predictive_mfma_support.forest_cases() the message formula (predictive_support.predictive_from_messages on functional_support.forest_bp's
exact messages) agrees with the independent references — the dense leave-one-out solve, the Kalman filters — to 1e-10 in
assert_rows_close's measure with equal statuses, so that every row of the GPU tests can be held to the plain 1e-9; and the status
patterns the GPU tests assert are those of the references.  (The long chains of the GPU file's test 10 are lgssm_chain models like the
six-state ones here; their dense leave-one-out reference would be O(T) solves of a T d system and is not run.)"""
import numpy as np
import pytest

from tests import evidence_support as E
from tests import functional_support as F
from tests import predictive_mfma_support as PM
from tests import predictive_support as P

CASES = PM.forest_cases()
TOL = 1e-10


def _both(name):
    model, opq = CASES[name]()
    gm = E.gmodel(model) if opq is None else E.gmodel(model, opaque=opq)
    f2v = F.forest_bp(gm)
    return model, gm, P.predictive_from_messages(gm, f2v, mode=P.LOO), P.predictive_from_messages(gm, f2v, mode=P.CAUSAL)


@pytest.mark.parametrize("name", sorted(CASES))
def test_message_formula_agrees_with_the_independent_references(name):
    model, gm, loo, cau = _both(name)
    dense = P.dense_loo_all(gm)
    errs = P.assert_rows_close(loo, dense, TOL, name + " loo")
    assert np.array_equal(loo["status"], dense["status"]), (name, loo["status"], dense["status"])
    print(name, "loo", errs)
    n = len(cau["status"])
    if name.startswith("chain"):
        want = PM.innovations_rows(model)
        print(name, "causal", P.assert_rows_close(cau, want, TOL, name + " causal"))
        assert np.array_equal(cau["status"], want["status"]) and cau["status"].tolist() == [2] + [0] * (n - 1)
        assert abs(cau["total"] - E.kalman_of_chain(model)) <= TOL * abs(cau["total"])      # H = I: the improper row's share is 0
    elif name.startswith("gen"):
        want, log_first = PM.kalman_rows(model)
        print(name, "causal", P.assert_rows_close(cau, want, TOL, name + " causal"))
        assert np.array_equal(cau["status"], want["status"]) and cau["status"].tolist() == [2] + [0] * (n - 1)
        assert np.array_equal(np.sort(cau["factor_ids"]), np.sort(np.asarray(model.data_fac)))      # the rows are exactly the observed steps
        z = E.dense_log_z(gm)
        assert abs(cau["total"] + log_first - z) <= TOL * abs(z), (name, cau["total"], log_first, z)
    elif name.startswith("comb"):
        assert cau["status"].tolist() == [2] + [0] * (n - 1), (name, cau["status"])
    elif name.startswith("leading gap"):
        # the first transition's message into x_2 carries no information: on exact messages its precision is the rounding of a difference
        assert n == 4 and cau["status"].tolist() == [2, 0, 0, 0] and loo["status"].tolist() == [0, 0, 0, 0], (name, cau["status"], loo["status"])
    elif name.startswith("prior"):
        z = E.dense_log_z(gm)
        assert not cau["status"].any() and not loo["status"].any()
        assert abs(cau["total"] - z) <= TOL * abs(z), (name, cau["total"], z)
    else:
        assert name.startswith("clamped")
        # five rows: four likelihoods of free states and the transition into the clamped state
        assert n == 5 and cau["status"].tolist() == [2, 0, 0, 0, 0] and not loo["status"].any(), (name, cau["status"], loo["status"])
