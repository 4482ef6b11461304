"""CPU: the two statements of the smoothed disturbances in tests/disturbances_mfma_support.py (the dense joint posterior and the
restatement of the kernel's algebra on given messages) pinned against each other, against the RTS smoother and against the trace
identity Σ_f tr(Q_f⁻¹ Cov(r_f)) = the number of latent scalar components, before any GPU run; and learn.auxiliary_residuals against its
definition."""
import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import learn
from tests import anisotropic as AN
from tests import disturbances_mfma_support as D
from tests import evidence_mfma_support as EM
from tests import evidence_support as E
from tests import learn_mfma_support as M
from tests import offsets_support as O

KEYS = ("mean", "cov", "expected_mahalanobis", "mahalanobis")


def _close(got, want, tol, what):
    err = float(np.max(np.abs(np.asarray(got) - np.asarray(want)))) if np.size(want) else 0.0
    assert np.all(np.isfinite(got)) and err <= tol, (what, err, tol)


def _same_rows(a, b, what):
    assert np.array_equal(a["factor_ids"], b["factor_ids"])
    for k in KEYS:
        _close(a[k], b[k], 1e-9 * max(1.0, float(np.max(np.abs(b[k])))), f"{what} {k}")


@pytest.mark.parametrize("d", (5, 16, 20))
def test_dense_is_the_restatement_on_exact_messages(d):
    for name, model, _ in M.small_models(d):
        gm = E.gmodel(model)
        _same_rows(D.restated(gm, E.numpy_bp(gm, max_iter=60)), D.dense(model), f"d {d} {name}")


@pytest.mark.parametrize("d", EM.OPAQUE_DIMS)
def test_dense_takes_an_opaque_prior(d):
    model, opq = EM.prior_chain(d)
    gm = E.gmodel(model, opaque=opq)
    _same_rows(D.restated(gm, E.numpy_bp(gm, max_iter=60)), D.dense(model, opaque=opq), f"prior chain d {d}")


@pytest.mark.parametrize("d", (5, 16))
def test_dense_is_the_rts_smoother_on_a_chain(d):
    model = cx.synth.lgssm_chain(9, d=d, seed=12 + d)
    got = D.dense(model)
    mom = M.rts_factor_moments(model)      # {set: (E[r], E[x], E[r r'], ...)}: transitions, then likelihoods, both in time order
    sets = dict(zip(np.asarray(model.factor_ids).tolist(), np.asarray(model.factor_var).astype(int).tolist()))
    at = {0: 0, 1: 0}
    for i, f in enumerate(got["factor_ids"].tolist()):      # (ids ascend in time within a set)
        s = sets[f]
        er, err = mom[s][0][at[s]], mom[s][2][at[s]]
        at[s] += 1
        _close(got["mean"][i], er, 1e-9, f"d {d} factor {f} mean")
        _close(got["cov"][i], err - np.outer(er, er), 1e-9 * max(1.0, float(np.max(np.abs(err)))), f"d {d} factor {f} covariance")


CASES = {"chain": lambda: AN.chain(7, 5), "comb": lambda: AN.comb(4, 6, teeth=2), "loopy": lambda: AN.loopy(8, 5)}


@pytest.mark.parametrize("name", CASES)
def test_trace_identity_and_q_minus_cov_is_positive_semidefinite(name):
    """Σ_f (t_f - q_f) = tr(J S) = the number of latent scalar components whenever the joint precision J is the sum of the factors' own
    terms (no opaque message); the offsets move the means alone.  And Q - Cov(r | data) = Var(E[r | data]) is positive semi-definite."""
    model = CASES[name]()
    n = D.latent_dims(model)
    for b in (None, O.with_offsets(model, 3)):
        rows = D.dense(model, b)
        got = float(np.sum(rows["expected_mahalanobis"] - rows["mahalanobis"]))
        assert abs(got - n) <= 1e-9 * n, (name, got, n)
        Q = D.factor_Q(model, rows["factor_ids"])
        low = np.linalg.eigvalsh(Q - rows["cov"])[:, 0]
        assert np.all(low >= -1e-10 * np.max(np.abs(Q))), (name, low.min())
        t, q, _ = D.scores(rows["mean"], rows["cov"], Q)
        _close(t, rows["expected_mahalanobis"], 1e-10 * max(1.0, float(np.max(t))), name + " t")
        _close(q, rows["mahalanobis"], 1e-10 * max(1.0, float(np.max(q))), name + " q")
    with_b, without = D.dense(model, O.with_offsets(model, 3)), D.dense(model)
    _close(with_b["cov"], without["cov"], 1e-12 * float(np.max(np.abs(without["cov"]))), name + ": the offsets leave the covariances")
    assert np.max(np.abs(with_b["mean"] - without["mean"])) > 1e-3


def test_auxiliary_residuals_match_their_definition_and_are_nan_on_a_forecast_tail():
    d = 8
    model, _ = EM.forecast_chain(d)
    rows = D.dense(model)
    Q = D.factor_Q(model, rows["factor_ids"])
    z = learn.auxiliary_residuals(rows, Q)
    assert z.shape == (len(rows["factor_ids"]), d)
    var = np.diagonal(Q - rows["cov"], axis1=1, axis2=2)
    flat = var <= 64 * d * np.finfo(float).eps * np.diagonal(Q, axis1=1, axis2=2)
    assert np.array_equal(np.isnan(z), flat)
    _close(z[~flat], (rows["mean"] / np.sqrt(np.where(flat, 1.0, var)))[~flat], 0.0, "z")
    # the transitions behind the last datum say nothing about their disturbances: Cov(r) = Q, every entry NaN; the others are all defined
    tail = flat.all(axis=1)
    assert 1 <= tail.sum() < len(tail) and not flat[~tail].any()
    last = int(np.argmax(rows["factor_ids"]))
    assert tail[last]
    _close(rows["cov"][last], Q[last], 1e-12 * float(np.max(np.abs(Q[last]))), "Cov(r) = Q behind the flat leaf")
    # one Q for every row is taken as given
    tr = np.array([np.array_equal(q, Q[last]) for q in Q])
    one = learn.auxiliary_residuals({"mean": rows["mean"][tr], "cov": rows["cov"][tr]}, Q[last])
    assert np.array_equal(one, z[tr], equal_nan=True)
