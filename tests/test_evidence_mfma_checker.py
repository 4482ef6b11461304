"""CPU: the inputs of tests/test_gpu_evidence_mfma.py's loop and forecast-tail cases are what those tests take them for, so that the GPU
tests cannot pass on a degenerate input — the ring's belief propagation has a fixed point that 150 iterations reach, its Bethe value is
not the exact one, and the forecast-tail model has a finite exact value that the tail does not change."""
import math

import numpy as np
import pytest

from tests import evidence_mfma_support as S
from tests import evidence_support as E


@pytest.mark.parametrize("d", S.RING_DIMS)
def test_ring_bp_converges_within_150_iterations_and_bethe_is_not_exact(d):
    gm = E.gmodel(S.ring(d))
    a = E.numpy_bp(gm, max_iter=S.RING_SWEEPS, tol=0.0, seed_precision=1e-6)
    b = E.numpy_bp(gm, max_iter=S.RING_SWEEPS + 20, tol=0.0, seed_precision=1e-6)
    for k in a:
        for x, y in zip(a[k], b[k]):
            assert np.all(np.isfinite(x)) and np.max(np.abs(x - y)) <= 1e-12 * np.max(np.abs(y)), (d, k, np.max(np.abs(x - y)))
    bethe, exact = E.bethe_log_z(gm, a), E.dense_log_z(gm)
    assert math.isfinite(bethe) and math.isfinite(exact)
    assert abs(bethe - exact) > 1e-6 * abs(exact), (d, bethe, exact)
    assert abs(bethe - exact) < 0.1 * abs(exact), (d, bethe, exact)


@pytest.mark.parametrize("d", S.OPAQUE_DIMS)
def test_opaque_models_carry_a_proper_prior_and_a_flat_end_that_change_the_value_as_they_should(d):
    # a proper prior: positive definite, and its constant c_o and its pull on x_1 both show in the value
    model, opq = S.prior_chain(d)
    assert np.sum(np.asarray(model.factor_kind) == 0) == 1 and np.linalg.eigvalsh(opq[3][0])[0] > 0.4 and np.abs(opq[2]).max() > 0.5
    gm = E.gmodel(model, opaque=opq)
    with_prior = E.dense_log_z(gm)
    bare = E.dense_log_z(E.gmodel(model, opaque=(opq[0][:0], opq[1][:0], opq[2][:0], opq[3][:0])))
    c_o = 0.5 * np.linalg.slogdet(opq[3][0])[1] - 0.5 * opq[2][0] @ np.linalg.solve(opq[3][0], opq[2][0]) - 0.5 * d * math.log(2 * math.pi)
    assert math.isfinite(with_prior) and abs(with_prior - bare) > 1e-3 * abs(bare) and abs(with_prior - bare - c_o) > 1e-3 * abs(bare)
    assert abs(E.bethe_log_z(gm, E.numpy_bp(gm, max_iter=40)) - with_prior) <= 1e-10 * abs(with_prior)
    # a flat opaque end: natural zeros, no constant, and the tail behind the last datum still comes out 0 net
    model, opq = S.flat_opaque_tail(d)
    assert np.sum(np.asarray(model.factor_kind) == 0) == 2 and not opq[3][1].any() and not opq[2][1].any()
    gm = E.gmodel(model, opaque=opq)
    value = E.dense_log_z(gm)
    _, thin = S.forecast_chain(d)
    prior_only = E.dense_log_z(E.gmodel(S._with_opaque(thin, thin.x_ids[:1])[0], opaque=(opq[0][:1], opq[1][:1], opq[2][:1], opq[3][:1])))
    assert math.isfinite(value) and abs(value - prior_only) <= 1e-11 * abs(value), (value, prior_only)
    assert abs(E.bethe_log_z(gm, E.numpy_bp(gm, max_iter=40)) - value) <= 1e-10 * abs(value)


def test_clamped_middle_model_has_the_three_kinds_of_observed_factor():
    model = S.clamped_middle(16)
    gm = E.gmodel(model)
    n_obs = gm.obs[gm.groups[2]["vars"]].sum(axis=1)
    assert sorted(np.bincount(n_obs, minlength=3).tolist()) == [1, 2, 6] and np.bincount(n_obs, minlength=3)[2] == 1      # 2 free-free, 6 one end, 1 both
    assert math.isfinite(E.dense_log_z(gm))


@pytest.mark.parametrize("d", S.FORECAST_DIMS)
def test_forecast_tail_model_has_a_finite_value_that_the_tail_does_not_change(d):
    model, thin = S.forecast_chain(d)
    assert len(model.x_ids) == len(thin.x_ids) + 3 and int(np.sum(thin.meta["keep"])) < len(thin.x_ids)
    with_tail, without = E.dense_log_z(E.gmodel(model)), E.dense_log_z(E.gmodel(thin))
    assert math.isfinite(with_tail) and abs(with_tail - without) <= 1e-11 * abs(without), (d, with_tail, without)
    # exact messages on this tree give the same number through the formula the device evaluates
    gm = E.gmodel(model)
    assert abs(E.bethe_log_z(gm, E.numpy_bp(gm, max_iter=40)) - with_tail) <= 1e-10 * abs(with_tail)
