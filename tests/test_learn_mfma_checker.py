"""CPU: the numpy restatement of the algebra of cx_factor_beliefs_mfma / cx_factor_statistics_mfma (tests/learn_mfma_support.py,
DESIGN.md §4n) on exact CPU messages against the dense posterior, the dense residual statistics and the RTS smoother, at every model and
dim of tests/test_gpu_learn_mfma.py; and every factorisation of those models is positive definite, so that no GPU test hides a case
behind the NaN rule."""
import numpy as np
import pytest

import cortex.jl_amd as cx
from tests import evidence_mfma_support as EM
from tests import evidence_support as E
from tests import learn_mfma_support as M
from tests import learning_support as S


def _close(got, want, tol, what):
    err = float(np.max(np.abs(np.asarray(got) - np.asarray(want)))) if np.size(want) else 0.0
    assert err <= tol, (what, err, tol)


def _check(model, what, opaque=None):
    gm = E.gmodel(model, opaque=opaque)
    f2v = E.numpy_bp(gm, max_iter=60)
    fids = gm.groups[2]["fid"]
    means, covs, status = M.beliefs(gm, f2v)
    assert np.all(status == M.OK), (what, status)
    want_m, want_c = S.dense_factor_beliefs(gm, fids)
    _close(means, want_m, 1e-9, what + " means")
    _close(covs, want_c, 1e-9 * max(1.0, float(np.max(np.abs(want_c)))), what + " covariances")
    sets = {int(f): int(s) for f, s in zip(*S.pset_groups(model))}
    groups = np.array([sets[int(f)] for f in fids])
    got, cnt = M.statistics(gm, f2v, fids, groups, 2)
    want = S.grouped_statistics(gm, fids, groups, 2)
    assert cnt["undefined"] == 0 and cnt["not_positive_definite"] == 0 and cnt["factors"] == len(fids)
    for k in S.KEYS:
        _close(got[k], want[k], 1e-9 * max(1.0, float(np.max(np.abs(want[k])))), f"{what} {k}")
    return gm, f2v, got


@pytest.mark.parametrize("d", M.DIMS)
def test_restatement_matches_the_dense_posterior_on_the_small_models(d):
    for name, model, chain in M.small_models(d):
        _, _, got = _check(model, f"d {d} {name}")
        if chain:      # the lag-one covariances of the smoother, through the statistics they enter
            want = M.rts_statistics(model)
            for k in S.KEYS:
                _close(got[k], want[k], 1e-9 * max(1.0, float(np.max(np.abs(want[k])))), f"d {d} rts {k}")


@pytest.mark.parametrize("d", M.OBSERVED_DIMS)
def test_observed_ends(d):
    model = EM.clamped_middle(d)
    gm, _, _ = _check(model, f"clamped middle d {d}")
    n_obs = gm.obs[gm.groups[2]["vars"]].sum(axis=1)
    assert set(n_obs.tolist()) == {0, 1, 2}      # free-free, one end observed (both kinds: see test_evidence_mfma_checker), both observed


@pytest.mark.parametrize("d", EM.FORECAST_DIMS)
def test_forecast_tail_and_its_flat_leaf(d):
    model, _ = EM.forecast_chain(d)
    gm, f2v, _ = _check(model, f"forecast d {d}")
    rows = M.restate(gm, f2v, stats=True)
    last = int(np.argmax(gm.groups[2]["fid"]))      # the last transition: its OUT end is the latent leaf
    Q = gm.groups[2]["Q"][last]
    assert not gm.obs[gm.groups[2]["vars"][last]].any()
    _close(rows[last][2], Q, 1e-13 * float(np.max(np.abs(Q))), "Cov(r) = Q behind a flat leaf")
    _close(rows[last][3], 0.0, 0.0, "Cov(r, x_in) = 0 behind a flat leaf")


@pytest.mark.parametrize("d", EM.OPAQUE_DIMS)
def test_opaque_prior(d):
    model, opq = EM.prior_chain(d)
    _check(model, f"prior chain d {d}", opaque=opq)


@pytest.mark.parametrize("d", EM.RING_DIMS)
def test_ring_beliefs_are_defined_and_are_not_the_exact_ones(d):
    gm = E.gmodel(EM.ring(d))
    f2v = E.numpy_bp(gm, max_iter=EM.RING_SWEEPS, tol=0.0, seed_precision=1e-6)
    means, covs, status = M.beliefs(gm, f2v)
    assert np.all(status == M.OK)
    want_m, want_c = S.dense_factor_beliefs(gm, gm.groups[2]["fid"])
    assert np.max(np.abs(covs - want_c)) > 1e-6 * np.max(np.abs(want_c))


def test_the_long_chains_and_the_em_models_are_positive_definite_throughout():
    for T, d in M.LONG + ((200, 8), (200, 16), M.MANY):
        model = cx.synth.lgssm_chain(T, d=d, seed=33)
        A, Q, R = model.meta["A"], model.meta["Q"], model.meta["R"]
        ll, ms, Ps, Pc = S.rts(A, Q, np.eye(d), R, np.asarray(model.data_y).reshape(T, d))
        assert np.isfinite(ll) and np.all(np.linalg.eigvalsh(Ps)[:, 0] > 0)


def test_numpy_m_step_is_learn_m_step():
    model = cx.synth.lgssm_chain(40, d=5, seed=3)
    st = {k: v[0] for k, v in M.rts_statistics(model).items()}
    A = model.meta["A"]
    got = cx.learn.m_step(st, A)
    wantA, wantQ = M.numpy_m_step(st, A)
    _close(got["A"], wantA, 1e-12, "A")
    _close(got["Q"], wantQ, 1e-12, "Q")


def test_many_groups_make_more_partials_than_waves_and_regroup_the_same_sums():
    T, d = M.MANY
    groups, n_groups = M.many_groups(T)
    per = -(-(2 * T - 1) // 2048)      # factors per partial at 1 x 1 tiles (cx_learn_mfma.hip: max_waves)
    sizes = np.concatenate([np.bincount(groups[0]), np.bincount(groups[1])[int(groups[0].max()) + 1:]])
    assert per == 2 and int(np.sum(-(-sizes // per))) > 2048 and n_groups == len(sizes) == 2101
    model = cx.synth.lgssm_chain(T, d=d, seed=33)
    fine, coarse = M.rts_statistics(model, groups, n_groups), M.rts_statistics(model)
    n_tr = int(groups[0].max()) + 1
    for k in S.KEYS:
        _close(fine[k][:n_tr].sum(0), coarse[k][0], 1e-10 * max(1.0, float(np.max(np.abs(coarse[k][0])))), k + " transitions")
        _close(fine[k][n_tr:].sum(0), coarse[k][1], 1e-10 * max(1.0, float(np.max(np.abs(coarse[k][1])))), k + " likelihoods")
