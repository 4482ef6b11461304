"""Shared by the predictive-score tests: three independent statements of what cx_predictive returns, over the GModel and
the message arrays of tests/evidence_support.py.

  predictive_from_messages   the formula of cx_predictive from arrays of factor→variable messages, in the same centred coordinates
  dense_loo                  the dense joint solve of the model with ONE factor (and its datum) removed, pushed through (A, b, Q)
  kalman_innovations         ŷ_t, S_t and the per-step term of the prediction-error decomposition (flat prior on the first state)

A GModel states every rule factor as  Σ_e C_e x_e - b ~ N(0, Q)  with entry 0 the CX_ROLE_OUT end (C_0 = I) and the others CX_ROLE_IN
(CX_FACTOR_GAUSS_ADDITIVE: the lower variable id first, C = (1, -1), b = 0).  A row is a factor whose entry 0 is its only observed
variable, or a scalar additive factor — recognised here by k = 2, C = (1, -1), b = 0 — with either entry the only observed one.
"""
from __future__ import annotations

import math

import numpy as np

from tests import evidence_support as E

LOG2PI = E.LOG2PI
LOO, CAUSAL = 0, 1


def rows_of(gm):
    """[(factor id, arity, index in its group, position of the datum)] in ascending factor id"""
    out = []
    for k, g in gm.groups.items():
        for fi, (fid, V, C, b) in enumerate(zip(g["fid"], g["vars"], g["C"], g["b"])):
            ob = gm.obs[V]
            if ob.sum() != 1:
                continue
            o = int(np.flatnonzero(ob)[0])
            additive = gm.d == 1 and k == 2 and C[0, 0, 0] == 1.0 and C[1, 0, 0] == -1.0 and b[0] == 0.0
            if o == 0 or additive:
                out.append((int(fid), k, fi, o))
    return sorted(out)


def _affine(g, fi, o):
    """y = Σ_j A_j x_j + b' + N(0, Q) of the factor's datum entry o: {j: A_j}, b', Q"""
    C, b, Q = g["C"][fi], g["b"][fi], g["Q"][fi]
    s = C[o][0, 0]                                   # C_o = ± I
    return {j: -s * C[j] for j in range(len(C)) if j != o}, s * b, Q


def _score(y, yh, S):
    d = len(y)
    try:
        Ls = np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        return None
    z = np.linalg.solve(Ls, y - yh)
    maha = float(z @ z)
    return -0.5 * (d * LOG2PI + 2.0 * np.log(np.diag(Ls)).sum() + maha), maha


def _result(fids, d):
    n = len(fids)
    return {"factor_ids": np.asarray(fids, np.int64), "mean": np.full((n, d), np.nan), "cov": np.full((n, d, d), np.nan),
            "log_density": np.full(n, np.nan), "mahalanobis": np.full(n, np.nan), "status": np.zeros(n, np.int64)}


def _finish(res):
    st = res["status"]
    res["total"] = math.fsum(res["log_density"][st == 0].tolist())
    res["counts"] = {"rows": len(st), "scored": int((st == 0).sum()), "undefined": int((st == 1).sum()), "improper": int((st == 2).sum())}
    return res


def predictive_from_messages(gm, f2v, opq=None, mode=LOO):
    """f2v, opq: as evidence_support.bethe_log_z takes them (device_messages / numpy_bp).  Every row of rows_of(gm), ascending factor id:
    {"factor_ids", "mean", "cov", "log_density", "mahalanobis", "status" (0 scored, 1 an undefined input, 2 improper), "total", "counts"}"""
    d, nv = gm.d, len(gm.var_ids)
    oe, ol = (gm.opq_eta, gm.opq_lam) if opq is None else opq
    M_eta, M_lam = np.zeros((nv, d)), np.zeros((nv, d, d))
    into_in = {}                                     # variable -> [(k, fi, j)]: the messages into it from factors on which it is an IN entry
    for k, g in gm.groups.items():
        e, l = f2v[k]
        for j in range(k):
            np.add.at(M_eta, g["vars"][:, j], e[:, j])
            np.add.at(M_lam, g["vars"][:, j], l[:, j])
            if j >= 1:
                for fi, v in enumerate(g["vars"][:, j]):
                    into_in.setdefault(int(v), []).append((k, fi, j))
    np.add.at(M_eta, gm.opq_var, oe)
    np.add.at(M_lam, gm.opq_var, ol)
    n_msgs = np.bincount(gm.opq_var, minlength=nv)       # messages into every variable, the opaque ones included
    for k, g in gm.groups.items():
        n_msgs = n_msgs + np.bincount(g["vars"].reshape(-1), minlength=nv)
    pd = E._pd(M_lam)
    mu = np.zeros((nv, d))
    if pd.any():
        mu[pd] = np.linalg.solve(M_lam[pd], M_eta[pd][..., None])[..., 0]
    eta_c = np.where(pd[:, None], 0.0, M_eta)
    rows = rows_of(gm)
    res = _result([r[0] for r in rows], d)
    for r, (_fid, k, fi, o) in enumerate(rows):
        g = gm.groups[k]
        A, b, Q = _affine(g, fi, o)
        e, l = f2v[k]
        yh, S, status = b.astype(float).copy(), np.array(Q, float), 0
        for j, Aj in A.items():
            v = int(g["vars"][fi, j])
            out = [(k, fi, j)] + ([t for t in into_in.get(v, []) if t != (k, fi, j)] if mode == CAUSAL else [])
            lt, et = M_lam[v].copy(), eta_c[v].copy()
            for (k2, f2, j2) in out:
                e2, l2 = f2v[k2][0][f2, j2], f2v[k2][1][f2, j2]
                lt = lt - l2
                et = et - (e2 - l2 @ mu[v])
            if np.isnan(lt).any() or np.isnan(et).any():
                status = 1
                continue
            if len(out) == n_msgs[v]:                    # nothing is left: flat by structure (M - its own terms need not round to 0)
                status = status or 2
                continue
            try:
                Lc = np.linalg.cholesky(lt)
            except np.linalg.LinAlgError:
                status = status or 2
                continue
            # what is left is a DIFFERENCE: a pivot below 64 ulp of the belief's own entry is the rounding of a flat remainder (the flat
            # message behind a forecast's end), of either sign — improper, as cx_predictive has it
            if not np.all(np.diag(Lc) ** 2 > 64 * np.finfo(float).eps * np.maximum(np.diag(M_lam[v]), 0.0)):
                status = status or 2
                continue
            Sc = np.linalg.inv(lt)
            yh = yh + Aj @ (mu[v] + Sc @ et)
            S = S + Aj @ (0.5 * (Sc + Sc.T)) @ Aj.T
        sc = _score(gm.y[g["vars"][fi, o]], yh, S) if status == 0 else None
        if status == 0 and sc is None:
            status = 2
        res["status"][r] = status
        if status == 0:
            res["mean"][r], res["cov"][r], res["log_density"][r], res["mahalanobis"][r] = yh, S, sc[0], sc[1]
    return _finish(res)


def dense_loo(gm, fid):
    """p(y_a | all other data) of row `fid` from the dense joint of the model WITHOUT that factor: (mean, cov, log_density, mahalanobis), or
    None when the joint precision of what is left is not positive definite (an improper predictive)"""
    row = [r for r in rows_of(gm) if r[0] == int(fid)]
    assert row, f"factor {fid} is not a row"
    _, k0, fi0, o0 = row[0]
    d = gm.d
    free = np.flatnonzero(~gm.obs)
    fpos = -np.ones(len(gm.var_ids), np.int64)
    fpos[free] = np.arange(len(free))
    n = len(free) * d
    J, h = np.zeros((n, n)), np.zeros(n)
    for k, g in gm.groups.items():
        for fi, (vs, C, b, Q) in enumerate(zip(g["vars"], g["C"], g["b"], g["Q"])):
            if k == k0 and fi == fi0:
                continue
            Qi = np.linalg.inv(Q)
            bp = b - sum(C[j] @ gm.y[v] for j, v in enumerate(vs) if gm.obs[v])
            fr = [(j, fpos[v]) for j, v in enumerate(vs) if not gm.obs[v]]
            for j, a in fr:
                h[a * d:(a + 1) * d] += C[j].T @ Qi @ bp
                for l, c in fr:
                    J[a * d:(a + 1) * d, c * d:(c + 1) * d] += C[j].T @ Qi @ C[l]
    for v, eta, lam in zip(gm.opq_var, gm.opq_eta, gm.opq_lam):
        if gm.obs[v] or np.isnan(eta).any() or np.isnan(lam).any():
            continue
        a = fpos[v]
        J[a * d:(a + 1) * d, a * d:(a + 1) * d] += lam
        h[a * d:(a + 1) * d] += eta
    try:
        np.linalg.cholesky(J)
    except np.linalg.LinAlgError:
        return None
    Sig = np.linalg.inv(J)
    Sig = 0.5 * (Sig + Sig.T)
    m = Sig @ h
    g = gm.groups[k0]
    A, b, Q = _affine(g, fi0, o0)
    yh, S = b.astype(float).copy(), np.array(Q, float)
    pos = {j: int(fpos[g["vars"][fi0, j]]) for j in A}
    for j, Aj in A.items():
        a = pos[j]
        yh = yh + Aj @ m[a * d:(a + 1) * d]
        for l, Al in A.items():
            c = pos[l]
            S = S + Aj @ Sig[a * d:(a + 1) * d, c * d:(c + 1) * d] @ Al.T
    sc = _score(gm.y[g["vars"][fi0, o0]], yh, 0.5 * (S + S.T))
    return None if sc is None else (yh, S, sc[0], sc[1])


def dense_loo_all(gm):
    """dense_loo of every row, in the layout of predictive_from_messages"""
    rows = rows_of(gm)
    res = _result([r[0] for r in rows], gm.d)
    for r, row in enumerate(rows):
        got = dense_loo(gm, row[0])
        if got is None:
            res["status"][r] = 2
        else:
            res["mean"][r], res["cov"][r], res["log_density"][r], res["mahalanobis"][r] = got
    return _finish(res)


# ---- Kalman ----------------------------------------------------------------------------------------------------------------------
def kalman_innovations(A, b, Q, R, y):
    """the recursion of evidence_support.kalman_log_lik, keeping its innovations: (ŷ [T, d], S [T, d, d], term [T], maha [T]) with row 0 NaN
    (flat prior on x_1: no proper prediction of y_1); Σ term[1:] is kalman_log_lik"""
    T, d = y.shape
    A, b, Q, R = (np.asarray(z, float) for z in (A, b, Q, R))
    A, Q, R, b = A.reshape(T - 1, d, d), Q.reshape(T - 1, d, d), R.reshape(T, d, d), b.reshape(T - 1, d)
    yh, S, term, maha = np.full((T, d), np.nan), np.full((T, d, d), np.nan), np.full(T, np.nan), np.full(T, np.nan)
    m, P = y[0].astype(float).copy(), R[0].copy()
    for t in range(1, T):
        mp = A[t - 1] @ m + b[t - 1]
        Pp = A[t - 1] @ P @ A[t - 1].T + Q[t - 1]
        St = Pp + R[t]
        yh[t], S[t] = mp, St
        term[t], maha[t] = _score(y[t], mp, St)
        K = np.linalg.solve(St, Pp).T
        m = mp + K @ (y[t] - mp)
        P = Pp - K @ Pp
        P = 0.5 * (P + P.T)
    return yh, S, term, maha


def innovations_of_chain(model):
    """the rows CX_PREDICT_CAUSAL gives on a synth.ssm_chain / ssm_chain_linear / lgssm_chain model, in the order of its likelihood factors
    (time).  ssm_chain's transitions are CX_FACTOR_GAUSS_ADDITIVE, whose `in` end is the LATER state: there the causal rows are those of
    the reverse-time filter, p(y_t | y_>t), the same recursion on the reversed series."""
    kind, T, d = model.meta["kind"], model.meta["T"], model.dim
    y = np.asarray(model.data_y, float).reshape(T, d)
    if kind == "ssm_chain":
        r, q = np.broadcast_to(model.meta["r"], (T,)), np.broadcast_to(model.meta["q"], (T - 1,))
        out = kalman_innovations(np.ones(T - 1), np.zeros(T - 1), q[::-1].copy(), r[::-1].copy(), y[::-1].copy())
        return tuple(z[::-1].copy() for z in out)
    if kind == "ssm_chain_linear":
        return kalman_innovations(model.meta["a"], model.meta["b"], model.meta["q"], np.full(T, model.meta["r"]), y)
    A, Q, R = model.meta["A"], model.meta["Q"], model.meta["R"]
    return kalman_innovations(np.broadcast_to(A, (T - 1, d, d)), np.zeros((T - 1, d)), np.broadcast_to(Q, (T - 1, d, d)),
                              np.broadcast_to(R, (T, d, d)), y)


# ---- comparison ------------------------------------------------------------------------------------------------------------------
def scaled_err(a, b):
    """max |a - b| over max |b| (matrices are scaled by their largest entry); NaN patterns must agree"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)), "shape or NaN pattern differs"
    if a.ndim <= 1:
        ok = ~np.isnan(b)
        return float(np.max(np.abs(a[ok] - b[ok]) / np.maximum(np.abs(b[ok]), 1e-300), initial=0.0))
    worst = 0.0
    for x, y in zip(a, b):
        if np.isnan(y).any():
            continue
        worst = max(worst, float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-300)))
    return worst


def assert_rows_close(got, want, tol, what=""):
    """mean, cov, log_density and mahalanobis of two results, row by row: vectors and matrices scaled by their largest entry"""
    assert np.array_equal(np.asarray(got["factor_ids"]), np.asarray(want["factor_ids"])), what
    errs = {k: scaled_err(got[k], want[k]) for k in ("mean", "cov", "log_density")}
    # the squared residual of a datum that sits on its prediction is a difference of equal numbers: scaled by 1 + its value
    ok = ~np.isnan(np.asarray(want["mahalanobis"]))
    errs["mahalanobis"] = float(np.max(np.abs(got["mahalanobis"][ok] - want["mahalanobis"][ok]) / (1.0 + np.abs(want["mahalanobis"][ok])), initial=0.0))
    assert np.array_equal(np.isnan(got["mahalanobis"]), ~ok), what
    assert all(e <= tol for e in errs.values()), (what, errs)
    return errs
