"""CPU checks of the three statements of log p(data) that the log-evidence tests compare cx_log_evidence against
(tests/evidence_support.py): the dense joint, the Kalman filter's prediction-error decomposition and the numpy restatement of the
formula from messages.  They pin the helpers before any GPU run."""
import math

import numpy as np
import pytest

import cortex.jl_amd as cx
from tests import evidence_support as E


@pytest.mark.parametrize("make", [lambda: cx.synth.ssm_chain(60, seed=3), lambda: cx.synth.ssm_chain(40, seed=4, random_variances=True),
                                  lambda: cx.synth.ssm_chain_linear(60, seed=5), lambda: cx.synth.lgssm_chain(40, d=2, seed=6),
                                  lambda: cx.synth.lgssm_chain(30, d=4, seed=7)])
def test_dense_equals_kalman_on_chains(make):
    m = make()
    dense, kal = E.dense_log_z(E.gmodel(m)), E.kalman_of_chain(m)
    assert abs(dense - kal) <= 1e-10 * abs(kal), (dense, kal)


def test_one_variable_model_is_a_normal_density():
    y, r = 1.7, 0.6
    want = -0.5 * math.log(2 * math.pi * (1 + r)) - 0.5 * y * y / (1 + r)
    gm = E.gmodel(E.one_variable_model(y, r))
    assert abs(E.dense_log_z(gm) - want) <= 1e-13
    assert abs(E.bethe_log_z(gm, E.numpy_bp(gm)) - want) <= 1e-13


@pytest.mark.parametrize("make", [lambda: cx.synth.tree_model(30, seed=11, k_choices=(1, 2, 3, 5, 6), observe=0.2),
                                  lambda: cx.synth.tree_model(24, seed=12, k_choices=(1, 1, 2), observe=0.3, components=3),
                                  lambda: cx.synth.kary_model(15, seed=13, observe=0.3),
                                  lambda: cx.synth.ssm_chain_linear(25, seed=14)])
def test_restatement_with_exact_tree_messages_equals_dense(make):
    gm = E.gmodel(make())
    dense = E.dense_log_z(gm)
    bethe = E.bethe_log_z(gm, E.numpy_bp(gm))
    assert abs(bethe - dense) <= 1e-10 * abs(dense), (bethe, dense)


def test_restatement_at_d4_on_a_chain_equals_dense():
    gm = E.gmodel(cx.synth.lgssm_chain(12, d=4, seed=15))
    dense = E.dense_log_z(gm)
    assert abs(E.bethe_log_z(gm, E.numpy_bp(gm)) - dense) <= 1e-10 * abs(dense)


def test_restatement_is_not_exact_on_a_loopy_grid():
    gm = E.gmodel(cx.synth.gaussian_grid(4, 5, seed=2))
    dense = E.dense_log_z(gm)
    bethe = E.bethe_log_z(gm, E.numpy_bp(gm, seed_precision=1e-6))
    assert np.isfinite(bethe) and abs(bethe - dense) > 1e-4 * abs(dense), (bethe, dense)


def test_restatement_is_nan_on_undefined_messages():
    gm = E.gmodel(cx.synth.ssm_chain(10, seed=1))
    f2v = E.numpy_bp(gm, max_iter=2)        # the middle of the chain is not reached yet
    assert math.isnan(E.bethe_log_z(gm, f2v))
