"""Shared by the cx_factor_beliefs_mfma / cx_factor_statistics_mfma tests (tests/test_gpu_learn_mfma.py, pinned on the CPU by
tests/test_learn_mfma_checker.py): a numpy restatement of the kernel's algebra on GIVEN factor→variable messages, and
the statistics of a chain from the RTS smoother.

  factor_moments   one factor: eliminate OUT (M = Λ_o + Q⁻¹ = U'U, W_M = U^-T, Yt = W_M Q⁻¹A), the marginal of IN (S = Λ_i + C - Yt'Yt),
                   then the pair (f, x_in) with f = x_out (beliefs) or f = r = x_out - A x_in formed directly (K = M⁻¹ Λ_o A)
  restate          every two-variable factor of a GModel from a message dict (evidence_support.numpy_bp or device_messages); the
                   leave-one-out messages are SUMS of the other messages, as on the device
  beliefs / statistics   the layouts of DeviceGraph.factor_beliefs_mfma / factor_statistics_mfma
  rts_statistics   the same statistics of a synth.lgssm_chain from learning_support.rts (smoothed and lag-one covariances)
"""
from __future__ import annotations

import numpy as np

from tests import evidence_support as E
from tests import learning_support as S

OK, UNDEFINED, NOT_PD = 0, 1, 2


def assert_within(got, want, tol, what):
    """every entry finite and within the absolute bound tol of want's; prints the largest error"""
    got, want = np.asarray(got, float), np.asarray(want, float)
    err = float(np.max(np.abs(got - want))) if want.size else 0.0
    print(f"{what}: max abs error {err:.3e} (bound {tol:.3e})")
    assert np.all(np.isfinite(got)), what
    assert err <= tol, (what, err, tol)


def bound_of(want):
    """the bound of covariances and statistics: 1e-9 max(1, max|want|)"""
    return 1e-9 * max(1.0, float(np.max(np.abs(want)))) if np.size(want) else 1e-9


def _winv(M):
    """W = U^-T for M = U'U (numpy's lower Cholesky factor is U'); raises LinAlgError when M is not positive definite"""
    return np.linalg.inv(np.linalg.cholesky(M))


def factor_moments(A, Q, lam_o, eta_o, lam_i, eta_i, y_o, y_i, stats):
    """(E[f], E[x_in], Cov(f), Cov(f, x_in), Cov(x_in), status).  y_o / y_i: the datum of an observed end, else None (then lam / eta
    is the leave-one-out message of that end)."""
    d = len(A)
    P = np.linalg.inv(Q)
    bt = P @ A                      # B' of the rule table towards IN, (P, B, C) = (Q⁻¹, A'Q⁻¹, A'Q⁻¹A)
    C = A.T @ bt
    nan = np.full(d, np.nan), np.full(d, np.nan), np.full((d, d), np.nan), np.full((d, d), np.nan), np.full((d, d), np.nan)
    ins = [z for z in (y_o, y_i) if z is not None] + ([lam_o, eta_o] if y_o is None else []) + ([lam_i, eta_i] if y_i is None else [])
    if any(np.isnan(z).any() for z in ins):
        return (*nan, UNDEFINED)
    try:
        if y_o is None:
            W = _winv(lam_o + P)
            z = W @ eta_o
            Yt = W @ bt
            Minv = W.T @ W
            m0 = W.T @ z
            lam_p, eta_p = C - Yt.T @ Yt, Yt.T @ z
            Jt = -(lam_o @ A).T @ Minv if stats else bt.T @ Minv
        else:
            Minv, m0 = np.zeros((d, d)), y_o
            lam_p, eta_p = C, bt.T @ y_o
            Jt = -A.T if stats else np.zeros((d, d))
        if y_i is None:
            Ws = _winv(lam_i + lam_p)
            Sii = Ws.T @ Ws
            mu = Ws.T @ (Ws @ (eta_i + eta_p))
        else:
            Sii, mu = np.zeros((d, d)), y_i
    except np.linalg.LinAlgError:
        return (*nan, NOT_PD)
    N = Sii @ Jt
    return m0 + Jt.T @ mu, mu, Minv + Jt.T @ N, N.T, Sii, OK


def restate(gm: E.GModel, f2v, opq_msgs=None, stats=False):
    """factor_moments of every two-variable factor of gm, in GModel order: a list of 6-tuples"""
    d = gm.d
    g = gm.groups[2]
    e, l = f2v[2]
    oe, ol = (gm.opq_eta, gm.opq_lam) if opq_msgs is None else opq_msgs
    into = {}                       # variable -> [(factor row or -1 - opaque index, eta, Lambda)]
    for fi, vs in enumerate(g["vars"]):
        for j in range(2):
            into.setdefault(int(vs[j]), []).append((fi, e[fi, j], l[fi, j]))
    for k, v in enumerate(gm.opq_var):
        into.setdefault(int(v), []).append((-1 - k, oe[k], ol[k]))

    def loo(v, fi):
        rest = [(ee, ll) for f, ee, ll in into[int(v)] if f != fi]
        return sum((ll for _, ll in rest), np.zeros((d, d))), sum((ee for ee, _ in rest), np.zeros(d))

    out = []
    for fi, vs in enumerate(g["vars"]):
        A, Q = -g["C"][fi, 1], g["Q"][fi]
        assert np.array_equal(g["C"][fi, 0], np.eye(d)) and not np.any(g["b"][fi])
        vo, vi = int(vs[0]), int(vs[1])
        lo, eo = (None, None) if gm.obs[vo] else loo(vo, fi)
        li, ei = (None, None) if gm.obs[vi] else loo(vi, fi)
        out.append(factor_moments(A, Q, lo, eo, li, ei, gm.y[vo] if gm.obs[vo] else None, gm.y[vi] if gm.obs[vi] else None, stats))
    return out


def beliefs(gm, f2v, opq_msgs=None, fids=None):
    """(means [n, 2d], covariances [n, 2d, 2d], status [n]) of `fids` (default: every two-variable factor in GModel order)"""
    rows = restate(gm, f2v, opq_msgs, stats=False)
    where = {int(f): i for i, f in enumerate(gm.groups[2]["fid"])}
    idx = range(len(rows)) if fids is None else [where[int(f)] for f in fids]
    means = np.array([np.concatenate([rows[i][0], rows[i][1]]) for i in idx])
    covs = np.array([np.block([[rows[i][2], rows[i][3]], [rows[i][3].T, rows[i][4]]]) for i in idx])
    return means, covs, np.array([rows[i][5] for i in idx])


def statistics(gm, f2v, fids, groups, n_groups, opq_msgs=None):
    """(the dict of DeviceGraph.factor_statistics_mfma, counts) from the restatement; a group with a failed factor is NaN (n excepted)"""
    d = gm.d
    rows = restate(gm, f2v, opq_msgs, stats=True)
    where = {int(f): i for i, f in enumerate(gm.groups[2]["fid"])}
    out = {"n": np.zeros(n_groups), "sum_r": np.zeros((n_groups, d)), "sum_x": np.zeros((n_groups, d)), "S_rr": np.zeros((n_groups, d, d)),
           "S_rx": np.zeros((n_groups, d, d)), "S_xx": np.zeros((n_groups, d, d))}
    cnt = {"factors": 0, "groups": 0, "undefined": 0, "not_positive_definite": 0}
    for f, k in zip(np.asarray(fids), np.asarray(groups)):
        if k < 0:
            continue
        er, ex, crr, crx, cxx, st = rows[where[int(f)]]
        out["n"][k] += 1
        cnt["factors"] += 1
        cnt["undefined"] += st == UNDEFINED
        cnt["not_positive_definite"] += st == NOT_PD
        out["sum_r"][k] += er
        out["sum_x"][k] += ex
        out["S_rr"][k] += crr + np.outer(er, er)
        out["S_rx"][k] += crx + np.outer(er, ex)
        out["S_xx"][k] += cxx + np.outer(ex, ex)
    cnt["groups"] = int((out["n"] > 0).sum())
    return out, cnt


def rts_factor_moments(model):
    """per factor of a synth.lgssm_chain, from the RTS smoother (smoothed and lag-one covariances): {set: (E[r], E[x_in], E[r r'],
    E[r x_in'], E[x_in x_in'])}, set 0 the T - 1 transitions and set 1 the T likelihoods (H = I), both in time order"""
    T, d = model.meta["T"], model.dim
    A, Q, R = model.meta["A"], model.meta["Q"], model.meta["R"]
    y = np.asarray(model.data_y, float).reshape(T, d)
    _, ms, Ps, Pc = S.rts(A, Q, np.eye(d), R, y)
    er = ms[1:] - ms[:-1] @ A.T
    crx = Pc - A @ Ps[:-1]                                        # Cov(x_{t+1} - A x_t, x_t)
    crr = Ps[1:] - A @ np.swapaxes(Pc, 1, 2) - Pc @ A.T + A @ Ps[:-1] @ A.T
    el = y - ms
    outer = lambda a, b: a[:, :, None] * b[:, None, :]
    return {0: (er, ms[:-1], crr + outer(er, er), crx + outer(er, ms[:-1]), Ps[:-1] + outer(ms[:-1], ms[:-1])),
            1: (el, ms, Ps + outer(el, el), -Ps + outer(el, ms), Ps + outer(ms, ms))}


def rts_statistics(model, groups=None, n_groups=2):
    """the statistics of a synth.lgssm_chain from the RTS smoother, in the layout of DeviceGraph.factor_statistics_mfma.  groups: {set:
    the group of every factor of that set in time order, -1 skipped}; default: one group per parameter set"""
    T, d = model.meta["T"], model.dim
    mom = rts_factor_moments(model)
    groups = {0: np.zeros(T - 1, np.int64), 1: np.ones(T, np.int64)} if groups is None else groups
    out = {"n": np.zeros(n_groups), "sum_r": np.zeros((n_groups, d)), "sum_x": np.zeros((n_groups, d)), "S_rr": np.zeros((n_groups, d, d)),
           "S_rx": np.zeros((n_groups, d, d)), "S_xx": np.zeros((n_groups, d, d))}
    for s in (0, 1):
        g = np.asarray(groups[s])
        keep = g >= 0
        np.add.at(out["n"], g[keep], 1.0)
        for key, v in zip(KEYS_SUMS, mom[s]):
            np.add.at(out[key], g[keep], v[keep])
    return out


KEYS_SUMS = ("sum_r", "sum_x", "S_rr", "S_rx", "S_xx")


def numpy_m_step(st, A, learn=("A", "Q")):
    """the M-step of one group from its residual statistics, written out: ΔA = S_rx S_xx⁻¹, Q' = (S_rr - ΔA S_rx') / n"""
    dA = st["S_rx"] @ np.linalg.inv(st["S_xx"]) if "A" in learn else np.zeros_like(A)
    Qn = (st["S_rr"] - dA @ st["S_rx"].T) / st["n"]
    return A + dA, 0.5 * (Qn + Qn.T)


# ---- the models of the GPU tests (both files read them from here) -------------------------------------------------------------------
DIMS = (5, 16, 20, 32, 40, 64)      # 5: the least; 20, 40: embedded in the 32- and 64-tile; 16, 32, 64: native
OBSERVED_DIMS = (16, 40)
LONG = ((3000, 16), (600, 64))      # more factors than one partial holds, at 1 x 1 and 4 x 4 tiles
MANY = (1500, 16)                   # with many_groups: more partials than waves of one launch


def many_groups(T):
    """{set: groups in time order}, n_groups for a chain of T states: the first 500 transitions one group, every other transition a
    group of its own, the first 400 likelihoods one group, every other likelihood a group of its own — T = 1500: 2,999 factors in
    2,101 groups, cut into 250 + 999 + 200 + 1,100 = 2,549 partials of at most two factors, more than the 2,048 waves of a launch at 1 x 1
    tiles: waves walk several partials, and partials hold several factors"""
    tr = np.where(np.arange(T - 1) < 500, 0, np.arange(T - 1) - 499)
    n_tr = int(tr.max()) + 1
    lik = np.where(np.arange(T) < 400, n_tr, n_tr + 1 + np.arange(T) - 400)
    return {0: tr, 1: lik}, int(lik.max()) + 1


def small_models(d):
    """[(name, model, is a chain)]: lgssm_chain(6, d) and the comb of tests/test_gpu_evidence_mfma.py"""
    import cortex.jl_amd as cx

    return [("chain", cx.synth.lgssm_chain(6, d=d, seed=30 + d), True), ("comb", cx.synth.lgssm_comb(4, d=d, teeth=1, seed=40 + d), False)]
