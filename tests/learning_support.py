"""Shared by the factor-statistics tests: independent statements of what cx_factor_beliefs / cx_factor_statistics return and of EM.

  dense_factor_beliefs     the joint posterior of every two-variable factor of an evidence_support.GModel from the dense joint
                           (mean J⁻¹h, covariance J⁻¹ of the non-observed variables; observed entries: the datum, zero covariance)
  grouped_statistics       the residual statistics of those beliefs (r = x_out - A x_in - b), summed per group, in the layout of
                           DeviceGraph.factor_statistics
  rts / kalman_log_lik_c   a Kalman filter with a flat prior on x_1 and a general observation matrix C, the RTS smoother with the
                           lag-one covariances, for synth.lgssm_chain / ssm_chain
  ss_em                    Shumway–Stoffer EM on raw moments (A, Q, C, R)
"""
from __future__ import annotations

import math

import numpy as np

from tests import evidence_support as E

LOG2PI = math.log(2.0 * math.pi)
KEYS = ("n", "sum_r", "sum_x", "S_rr", "S_rx", "S_xx")


def assert_rel_close(got, want, rtol, what=""):
    """every entry within rtol of want's, relative to max(|want|, 1)"""
    got, want = np.asarray(got, float), np.asarray(want, float)
    err = float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1.0))) if got.size else 0.0
    assert err <= rtol, (what, err)


# ---- dense ----------------------------------------------------------------------------------------------------------------------
def dense_posterior(gm: E.GModel):
    """(mean [nv, d] — the datum on observed variables —, covariance [nv, nv, d, d] — zero on observed ones —) of the whole model"""
    d = gm.d
    free = np.flatnonzero(~gm.obs)
    fpos = -np.ones(len(gm.var_ids), np.int64)
    fpos[free] = np.arange(len(free))
    n = len(free) * d
    J, h = np.zeros((n, n)), np.zeros(n)
    for g in gm.groups.values():
        for vs, C, b, Q in zip(g["vars"], g["C"], g["b"], g["Q"]):
            Qi = np.linalg.inv(Q)
            bp = b - sum(C[j] @ gm.y[v] for j, v in enumerate(vs) if gm.obs[v])
            fr = [(j, fpos[v]) for j, v in enumerate(vs) if not gm.obs[v]]
            for j, a in fr:
                h[a * d:(a + 1) * d] += C[j].T @ Qi @ bp
                for l, c in fr:
                    J[a * d:(a + 1) * d, c * d:(c + 1) * d] += C[j].T @ Qi @ C[l]
    for v, eta, lam in zip(gm.opq_var, gm.opq_eta, gm.opq_lam):
        if gm.obs[v]:
            continue
        a = fpos[v]
        J[a * d:(a + 1) * d, a * d:(a + 1) * d] += lam
        h[a * d:(a + 1) * d] += eta
    S = np.linalg.inv(J)
    m = S @ h
    mean = gm.y.copy()
    mean[free] = m.reshape(len(free), d)
    return mean, S, fpos


def dense_factor_beliefs(gm: E.GModel, fids=None):
    """(means [n, 2d], covariances [n, 2d, 2d]) of the two-variable factors `fids` (default: all of them, in GModel order), (out, in)"""
    d = gm.d
    g = gm.groups[2]
    mean, S, fpos = dense_posterior(gm)
    where = {int(f): i for i, f in enumerate(g["fid"])}
    fids = g["fid"] if fids is None else np.asarray(fids)
    means, covs = np.zeros((len(fids), 2 * d)), np.zeros((len(fids), 2 * d, 2 * d))
    for r, f in enumerate(fids):
        vs = g["vars"][where[int(f)]]
        means[r] = np.concatenate([mean[vs[0]], mean[vs[1]]])
        for a in range(2):
            for c in range(2):
                if fpos[vs[a]] >= 0 and fpos[vs[c]] >= 0:
                    pa, pc = fpos[vs[a]], fpos[vs[c]]
                    covs[r, a * d:(a + 1) * d, c * d:(c + 1) * d] = S[pa * d:(pa + 1) * d, pc * d:(pc + 1) * d]
    return means, covs


def factor_residual_moments(gm: E.GModel, means, covs, fids):
    """per factor: E[r], E[x_in], E[r r'], E[r x_in'], E[x_in x_in'] from its joint belief (means [n, 2d], covs [n, 2d, 2d])"""
    d = gm.d
    g = gm.groups[2]
    where = {int(f): i for i, f in enumerate(g["fid"])}
    idx = np.array([where[int(f)] for f in fids], np.int64)
    A, b = -g["C"][idx, 1], g["b"][idx]
    Cm = np.concatenate([np.broadcast_to(np.eye(d), A.shape), -A], axis=2)          # [n, d, 2d]
    er = np.einsum("nij,nj->ni", Cm, means) - b
    ex = means[:, d:]
    Crr = np.einsum("nij,njk,nlk->nil", Cm, covs, Cm)
    Crx = np.einsum("nij,njk->nik", Cm, covs[:, :, d:])
    Cxx = covs[:, d:, d:]
    return er, ex, Crr + er[:, :, None] * er[:, None, :], Crx + er[:, :, None] * ex[:, None, :], Cxx + ex[:, :, None] * ex[:, None, :]


def grouped_statistics(gm: E.GModel, fids, groups, n_groups, beliefs=None):
    """the layout of DeviceGraph.factor_statistics from the dense beliefs (or the given (means, covs) of `fids`); group -1: skipped"""
    d = gm.d
    fids, groups = np.asarray(fids, np.int64), np.asarray(groups, np.int64)
    means, covs = dense_factor_beliefs(gm, fids) if beliefs is None else beliefs
    er, ex, rr, rx, xx = factor_residual_moments(gm, means, covs, fids)
    out = {"n": np.zeros(n_groups), "sum_r": np.zeros((n_groups, d)), "sum_x": np.zeros((n_groups, d)),
           "S_rr": np.zeros((n_groups, d, d)), "S_rx": np.zeros((n_groups, d, d)), "S_xx": np.zeros((n_groups, d, d))}
    for k in range(n_groups):
        sel = groups == k
        out["n"][k] = sel.sum()
        for key, v in (("sum_r", er), ("sum_x", ex), ("S_rr", rr), ("S_rx", rx), ("S_xx", xx)):
            out[key][k] = np.array([math.fsum(c) for c in v[sel].reshape(int(sel.sum()), -1).T]).reshape(out[key][k].shape) if sel.any() else 0.0
    return out


def pset_groups(model):
    """(factor ids, groups) of the parameter-set grouping of a dim > 1 model: every two-variable factor, group = its set"""
    return np.asarray(model.factor_ids, np.int64), np.asarray(model.factor_var, float).reshape(len(model.factor_ids), -1)[:, 0].astype(np.int64)


# ---- Kalman / RTS with a general observation matrix ----------------------------------------------------------------------------------
def rts(A, Q, C, R, y):
    """x_{t+1} = A x_t + N(0, Q), y_t = C x_t + N(0, R), flat prior on x_1 (C invertible).  Returns (log p(y), smoothed means [T, d],
    covariances [T, d, d], lag-one covariances Cov(x_{t+1}, x_t | y) [T-1, d, d])."""
    y = np.asarray(y, float)
    T, d = y.shape
    A, Q, C, R = (np.asarray(z, float).reshape(d, d) for z in (A, Q, C, R))
    Ri = np.linalg.inv(R)
    mf, Pf, mp, Pp = np.zeros((T, d)), np.zeros((T, d, d)), np.zeros((T, d)), np.zeros((T, d, d))
    Pf[0] = np.linalg.inv(C.T @ Ri @ C)
    mf[0] = Pf[0] @ C.T @ Ri @ y[0]
    ll = -math.log(abs(np.linalg.det(C)))           # ∫ N(y_1; C x, R) dx = 1 / |det C|
    for t in range(1, T):
        mp[t] = A @ mf[t - 1]
        Pp[t] = A @ Pf[t - 1] @ A.T + Q
        S = C @ Pp[t] @ C.T + R
        e = y[t] - C @ mp[t]
        Ls = np.linalg.cholesky(S)
        z = np.linalg.solve(Ls, e)
        ll += -0.5 * d * LOG2PI - np.log(np.diag(Ls)).sum() - 0.5 * z @ z
        K = np.linalg.solve(S, C @ Pp[t]).T
        mf[t] = mp[t] + K @ e
        P = Pp[t] - K @ C @ Pp[t]
        Pf[t] = 0.5 * (P + P.T)
    ms, Ps, Pc = mf.copy(), Pf.copy(), np.zeros((max(T - 1, 0), d, d))
    for t in range(T - 2, -1, -1):
        G = np.linalg.solve(Pp[t + 1], A @ Pf[t]).T          # P_t A' Pp_{t+1}⁻¹
        ms[t] = mf[t] + G @ (ms[t + 1] - mp[t + 1])
        P = Pf[t] + G @ (Ps[t + 1] - Pp[t + 1]) @ G.T
        Ps[t] = 0.5 * (P + P.T)
        Pc[t] = Ps[t + 1] @ G.T
    return float(ll), ms, Ps, Pc


def kalman_log_lik_c(A, Q, C, R, y) -> float:
    return rts(A, Q, C, R, y)[0]


def ss_m_step(y, ms, Ps, Pc, learn=("A", "Q", "C", "R"), params=None):
    """Shumway–Stoffer on raw moments: A = S10 S00⁻¹, Q = (S11 - A S10') / (T-1), C = Syx Sxx⁻¹, R = (Syy - C Syx') / T"""
    T, d = y.shape
    A0, Q0, C0, R0 = params
    Exx = Ps + ms[:, :, None] * ms[:, None, :]
    S11, S00 = Exx[1:].sum(0), Exx[:-1].sum(0)
    S10 = (Pc + ms[1:, :, None] * ms[:-1, None, :]).sum(0)
    Syy = (y[:, :, None] * y[:, None, :]).sum(0)
    Syx = (y[:, :, None] * ms[:, None, :]).sum(0)
    Sxx = Exx.sum(0)
    A = S10 @ np.linalg.inv(S00) if "A" in learn else A0
    if "Q" in learn:
        Q = (S11 - A @ S10.T - S10 @ A.T + A @ S00 @ A.T) / (T - 1)
        Q = 0.5 * (Q + Q.T)
    else:
        Q = Q0
    C = Syx @ np.linalg.inv(Sxx) if "C" in learn else C0
    if "R" in learn:
        R = (Syy - C @ Syx.T - Syx @ C.T + C @ Sxx @ C.T) / T
        R = 0.5 * (R + R.T)
    else:
        R = R0
    return A, Q, C, R


def ss_em(y, A, Q, C, R, n_iter, learn=("A", "Q", "C", "R")):
    """n_iter EM iterations; returns (trace of n_iter + 1 log-likelihoods, the parameters of every iteration)"""
    params = [tuple(np.array(z, float) for z in (A, Q, C, R))]
    trace = []
    for it in range(n_iter + 1):
        ll, ms, Ps, Pc = rts(*params[-1], y)
        trace.append(ll)
        if it == n_iter:
            break
        params.append(ss_m_step(y, ms, Ps, Pc, learn, params[-1]))
    return trace, params


def raw_m_step(S11, S10, S00, n):
    """the textbook raw-moment update of one factor group, x_out ≈ A x_in: A = S10 S00⁻¹, Q = (S11 - A S10') / n"""
    A = S10 @ np.linalg.inv(S00)
    Q = (S11 - A @ S10.T) / n
    return A, 0.5 * (Q + Q.T)
