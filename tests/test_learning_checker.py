"""CPU checks of the statements the factor-statistics tests compare cx_factor_beliefs / cx_factor_statistics and learn.em against
(tests/learning_support.py): the dense factor beliefs against the RTS smoother, the Kalman log-likelihood with a general observation
matrix against the dense joint, Shumway–Stoffer EM, and learn.m_step against the raw-moment M-step."""
import math
from fractions import Fraction

import numpy as np

import cortex.jl_amd as cx
from cortex.jl_amd import learn
from tests import evidence_support as E
from tests import learning_support as S


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def test_dense_factor_beliefs_equal_the_rts_smoother():
    T, d = 30, 3
    m = cx.synth.lgssm_chain(T, d=d, seed=101)
    gm = E.gmodel(m)
    y = np.asarray(m.data_y).reshape(T, d)
    ll, ms, Ps, Pc = S.rts(m.meta["A"], m.meta["Q"], np.eye(d), m.meta["R"], y)
    tr = np.arange(3 * T + 1, 4 * T)
    means, covs = S.dense_factor_beliefs(gm, tr)
    want_m = np.concatenate([ms[1:], ms[:-1]], axis=1)                   # (out, in) = (x_{t+1}, x_t)
    want_c = np.block([[Ps[1:], Pc], [np.transpose(Pc, (0, 2, 1)), Ps[:-1]]])
    assert _rel(means, want_m) < 1e-10 and _rel(covs, want_c) < 1e-10
    lik = np.arange(2 * T + 1, 3 * T + 1)
    means, covs = S.dense_factor_beliefs(gm, lik)                         # (out, in) = (y_t observed, x_t)
    assert _rel(means, np.concatenate([y, ms], axis=1)) < 1e-10
    assert np.all(covs[:, :d, :] == 0) and np.all(covs[:, :, :d] == 0) and _rel(covs[:, d:, d:], Ps) < 1e-10
    assert abs(ll - E.kalman_of_chain(m)) <= 1e-10 * abs(ll)


def test_kalman_with_an_observation_matrix_equals_the_dense_joint():
    T, d = 25, 2
    m = cx.synth.lgssm_chain(T, d=d, seed=102)
    Cm, R = np.array([[1.2, 0.3], [-0.2, 0.9]]), np.array([[0.8, 0.1], [0.1, 0.5]])
    psets = dict(m.psets)
    psets[1] = (Cm, R)
    dense = E.dense_log_z(E.gmodel(m, psets=psets))
    kal = S.kalman_log_lik_c(m.meta["A"], m.meta["Q"], Cm, R, np.asarray(m.data_y).reshape(T, d))
    assert abs(dense - kal) <= 1e-10 * abs(dense), (dense, kal)


def _perturbed(m, d, rng):
    A = m.meta["A"] + 0.05 * rng.standard_normal((d, d))
    return A, 2.0 * m.meta["Q"], np.eye(d) + 0.05 * rng.standard_normal((d, d)), 0.5 * m.meta["R"]


def test_numpy_em_is_non_decreasing():
    T, d = 300, 2
    m = cx.synth.lgssm_chain(T, d=d, seed=103)
    trace, params = S.ss_em(np.asarray(m.data_y).reshape(T, d), *_perturbed(m, d, np.random.default_rng(1)), n_iter=12)
    steps = np.diff(trace)
    assert np.all(steps >= -1e-9 * abs(trace[-1])), steps
    assert trace[-1] > trace[0] + 1.0


def test_m_step_of_the_grouped_statistics_equals_shumway_stoffer():
    # O(1) data: the residual form (learn.m_step) and the raw moments (ss_m_step) agree
    T, d = 40, 2
    m = cx.synth.lgssm_chain(T, d=d, seed=104)
    A0, Q0, C0, R0 = _perturbed(m, d, np.random.default_rng(2))
    psets = {0: (A0, Q0), 1: (C0, R0)}
    gm = E.gmodel(m, psets=psets)
    fids, groups = S.pset_groups(m)
    st = S.grouped_statistics(gm, fids, groups, 2)
    y = np.asarray(m.data_y).reshape(T, d)
    _ll, ms, Ps, Pc = S.rts(A0, Q0, C0, R0, y)
    A, Q, C, R = S.ss_m_step(y, ms, Ps, Pc, params=(A0, Q0, C0, R0))
    tr, ob = learn.m_step(learn.group(st, 0), A0), learn.m_step(learn.group(st, 1), C0)
    for got, want in ((tr["A"], A), (tr["Q"], Q), (ob["A"], C), (ob["Q"], R)):
        assert _rel(got, want) < 1e-9, (got, want)
    # a Q-only step is S_rr / n; the raw textbook form agrees on this data
    q_only = learn.m_step(learn.group(st, 0), A0, learn=("Q",))
    assert np.array_equal(q_only["A"], A0) and _rel(q_only["Q"], st["S_rr"][0] / (T - 1)) < 1e-15
    Exx = Ps + ms[:, :, None] * ms[:, None, :]
    A_raw, _ = S.raw_m_step(Exx[1:].sum(0), (Pc + ms[1:, :, None] * ms[:-1, None, :]).sum(0), Exx[:-1].sum(0), T - 1)
    assert _rel(tr["A"], A_raw) < 1e-9


def test_m_step_learns_b_at_dim_1_by_regression_on_x_and_1():
    rng = np.random.default_rng(3)
    x = rng.standard_normal(500) * 3
    a, b, noise = 0.7, -1.3, 0.2 * rng.standard_normal(500)
    out = a * x + b + noise
    a0, b0 = 1.0, 0.0
    r = out - a0 * x - b0
    st = {"n": 500.0, "sum_r": [r.sum()], "sum_x": [x.sum()], "S_rr": [[r @ r]], "S_rx": [[r @ x]], "S_xx": [[x @ x]]}
    new = learn.m_step(st, [[a0]], [b0], learn=("A", "b", "Q"))
    Z = np.stack([x, np.ones_like(x)], axis=1)
    coef, *_ = np.linalg.lstsq(Z, out, rcond=None)
    res = out - Z @ coef
    assert abs(new["A"][0, 0] - coef[0]) < 1e-12 and abs(new["b"][0] - coef[1]) < 1e-12
    assert abs(new["Q"][0, 0] - res @ res / 500) < 1e-12


def _scalar_rts(y, q, r):
    """ssm_chain (x_{t+1} = x_t + N(0, q), y = x + N(0, r), flat prior on x_1) in plain floats: smoothed means, variances, lag-one"""
    T = len(y)
    mf, Pf, Pp = [0.0] * T, [0.0] * T, [0.0] * T
    mf[0], Pf[0] = y[0], r
    for t in range(1, T):
        Pp[t] = Pf[t - 1] + q
        K = Pp[t] / (Pp[t] + r)
        mf[t] = mf[t - 1] + K * (y[t] - mf[t - 1])
        Pf[t] = (1.0 - K) * Pp[t]
    ms, Ps, Pc = mf[:], Pf[:], [0.0] * (T - 1)
    for t in range(T - 2, -1, -1):
        G = Pf[t] / Pp[t + 1]
        ms[t] = mf[t] + G * (ms[t + 1] - mf[t])
        Ps[t] = Pf[t] + G * G * (Ps[t + 1] - Pp[t + 1])
        Pc[t] = Ps[t + 1] * G
    return ms, Ps, Pc


def test_m_step_keeps_q_on_a_drifting_chain_where_the_raw_form_does_not():
    # the C2-size chain: data grow as 2t up to 5e5.  The transitions' Q-only update from residual statistics against the same
    # update from raw second moments; the truth is the exact (rational) sum of the smoother's terms.
    T = 250_001
    m = cx.synth.ssm_chain(T, seed=105)
    ms, Ps, Pc = _scalar_rts(np.asarray(m.data_y, float).tolist(), 1.0, 1.0)
    n = T - 1
    # ADDITIVE transition (x_t, x_{t+1}): out = x_t (the lower id), in = x_{t+1}; r = x_t - x_{t+1}
    er = [ms[t] - ms[t + 1] for t in range(n)]
    vr = [Ps[t] + Ps[t + 1] - 2.0 * Pc[t] for t in range(n)]
    S_rr = math.fsum(e * e + v for e, v in zip(er, vr))
    exact = sum((Fraction(ms[t]) - Fraction(ms[t + 1])) ** 2 + Fraction(Ps[t]) + Fraction(Ps[t + 1]) - 2 * Fraction(Pc[t]) for t in range(n)) / n
    st = {"n": n, "sum_r": [sum(er)], "sum_x": [sum(ms[1:])], "S_rr": [[S_rr]], "S_rx": [[0.0]], "S_xx": [[1.0]]}
    q_res = learn.m_step(st, [[1.0]], learn=("Q",))["Q"][0, 0]
    m_ = np.asarray(ms)
    raw = (np.sum(m_[:-1] ** 2 + Ps[:-1]) - 2.0 * np.sum(m_[:-1] * m_[1:] + np.asarray(Pc)) + np.sum(m_[1:] ** 2 + Ps[1:])) / n
    err_res, err_raw = abs(q_res - float(exact)) / float(exact), abs(raw - float(exact)) / float(exact)
    assert err_res < 1e-13, err_res
    assert err_raw > 1e3 * max(err_res, 1e-16), (err_raw, err_res)
