"""Shared by the missing-data tests: chains and combs whose states are NOT all observed, and chains with a forecast horizon.

Every model of synth.py and tests/anisotropic.py hangs a likelihood (or a unary prior) on every latent variable.  Here the same graphs
lose some of them:

  thin(model, keep)     the likelihood factor and the observation variable of every state with keep[i] false are removed (edges, roles,
                        factor rows, data rows; ids are NOT renumbered): a latent variable of degree 2 whose side sum is exactly zero
  tail(model, h)        h more states behind the last one, transitions only; the last new state has degree 1, and its variable→factor
                        message is the caller's — natural-form zeros, the flat message, leaves the rest of the model untouched
  load(model, dev)      synth.load_into_device, then the flat message on every degree-1 latent variable (flat_ends=False: left unset)
  alt / run / sparse / random_keep      patterns of keep; the first and the last state are always kept (a proper posterior, and every path
                        starts and ends at an observed state)
  kalman_missing(model) a covariance-form Kalman filter and RTS smoother with a flat prior on x_1 that skips the update at an unobserved
                        step: smoothed moments, lag-one covariances, the innovations of the observed steps, their sum, and for a tail the
                        plain forecast recursion.  It shares nothing with the dense references (evidence_support.gmodel and what is built
                        on it), which take these models unchanged.
  gpu_models()          name -> builder of every case tests/test_gpu_missing_data.py runs; tests/test_missing_data_checkers.py walks it
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from tests import anisotropic as AN

LOG2PI = math.log(2.0 * math.pi)


# ---- patterns ----------------------------------------------------------------------------------------------------------------------
def _ends(keep):
    keep[0] = keep[-1] = True
    return keep


def alt(n):
    """every second state observed"""
    return _ends(np.arange(n) % 2 == 0)


def run(n, a, b):
    """states a..b (0-based, inclusive) unobserved"""
    assert 0 < a <= b < n - 1
    keep = np.ones(n, bool)
    keep[a:b + 1] = False
    return keep


def sparse(n):
    """only the first, the middle and the last state observed"""
    keep = np.zeros(n, bool)
    keep[n // 2] = True
    return _ends(keep)


def random_keep(n, p, seed):
    """every state observed with probability p"""
    return _ends(np.random.default_rng([seed, n, 81]).random(n) < p)


def comb_alt(n_spine, teeth=1):
    """a comb's every second spine state and every second tooth unobserved (x order: the spine, then the teeth); an unobserved tooth at
    the end of its path is a latent leaf of degree 1"""
    keep = np.ones(n_spine * (1 + teeth), bool)
    keep[1:n_spine - 1:2] = False
    keep[n_spine::2] = False
    return keep


# ---- builders ----------------------------------------------------------------------------------------------------------------------
def n_states(model):
    return len(model.x_ids)


def thin(model, keep):
    """`model` without the likelihood of the states whose keep is false.  keep: one bool per entry of model.x_ids.  Every state of the
    models this takes carries one likelihood factor, row i of the data arrays that of x_ids[i] (checked)."""
    keep = np.asarray(keep, bool)
    n = len(model.x_ids)
    assert keep.shape == (n,) and len(model.data_fac) == n and "keep" not in model.meta
    ev, ef = np.asarray(model.edge_var), np.asarray(model.edge_fac)
    for i in np.flatnonzero(~keep):
        assert sorted(ev[ef == model.data_fac[i]].tolist()) == sorted([int(model.x_ids[i]), int(model.data_var[i])]), "row i is not the likelihood of state i"
    gone = np.asarray(model.data_fac)[~keep]
    e_on = ~np.isin(ef, gone)
    f_on = ~np.isin(np.asarray(model.factor_ids), gone)
    d = model.dim
    y = np.asarray(model.data_y, float).reshape(n, d)[keep]
    return dataclasses.replace(
        model, edge_var=ev[e_on], edge_fac=ef[e_on], edge_role=None if model.edge_role is None else np.asarray(model.edge_role)[e_on],
        factor_ids=np.asarray(model.factor_ids)[f_on], factor_kind=np.asarray(model.factor_kind)[f_on], factor_var=np.asarray(model.factor_var)[f_on],
        data_var=np.asarray(model.data_var)[keep], data_fac=np.asarray(model.data_fac)[keep], data_y=y if d > 1 else y[:, 0],
        meta={**model.meta, "keep": keep, "lik_of_state": np.where(keep, np.asarray(model.data_fac), -1)})


def _transitions(model):
    """(factor ids, rows of factor_var) of a chain's transitions in time order: the factors that are no likelihood"""
    lik = set(np.asarray(model.meta.get("lik_of_state", model.data_fac)).tolist()) | set(np.asarray(model.data_fac).tolist())
    rows = [i for i, f in enumerate(np.asarray(model.factor_ids).tolist()) if f not in lik]
    return np.asarray(model.factor_ids)[rows], np.asarray(model.factor_var)[rows]


def tail(model, h):
    """`model` (a chain, thinned or not) with h more states behind the last one.  Tail transition k takes the parameters of the chain's
    own transition k mod (T - 1) (the scalar chains have per-factor parameters), the ids follow the largest id in use."""
    assert h >= 1 and model.meta["kind"] in ("ssm_chain", "ssm_chain_linear", "lgssm_chain") and "tail" not in model.meta
    T = len(model.x_ids)
    top = int(max(np.max(model.edge_var), np.max(model.edge_fac)))
    xs = top + 1 + np.arange(h, dtype=np.int64)
    fs = top + h + 1 + np.arange(h, dtype=np.int64)
    prev = np.concatenate([model.x_ids[-1:], xs[:-1]])
    _, par = _transitions(model)
    assert len(par) == T - 1
    new_par = par[np.arange(h) % (T - 1)]
    role = None
    if model.edge_role is not None:
        role = np.concatenate([model.edge_role, np.full(h, L.ROLE_IN), np.full(h, L.ROLE_OUT)]).astype(np.int32)
    kind = L.FACTOR_GAUSS_ADDITIVE if model.meta["kind"] == "ssm_chain" else L.FACTOR_GAUSS_LINEAR
    meta = {**model.meta, "tail": h, "tail_par": new_par}
    if "keep" not in meta:
        meta["keep"] = np.ones(T, bool)
        meta["lik_of_state"] = np.asarray(model.data_fac).copy()
    return dataclasses.replace(
        model, edge_var=np.concatenate([model.edge_var, prev, xs]), edge_fac=np.concatenate([model.edge_fac, fs, fs]), edge_role=role,
        factor_ids=np.concatenate([model.factor_ids, fs]), factor_kind=np.concatenate([model.factor_kind, np.full(h, kind, np.int32)]).astype(np.int32),
        factor_var=np.concatenate([model.factor_var, new_par]), x_ids=np.concatenate([model.x_ids, xs]), meta=meta)


def flat_end_edges(model):
    """(variable ids, factor ids) of the one edge of every latent variable of degree 1"""
    ev, ef = np.asarray(model.edge_var), np.asarray(model.edge_fac)
    ids, first, count = np.unique(ev, return_index=True, return_counts=True)
    leaf = (count == 1) & ~np.isin(ids, np.asarray(model.data_var))
    return ids[leaf], ef[first[leaf]]


def load(model, dev, flat_ends=True):
    cx.synth.load_into_device(model, dev)
    v, f = flat_end_edges(model)
    if flat_ends and len(v):
        d = model.dim
        dev.set_messages(v, f, L.TO_FACTOR, L.FORM_NATURAL, np.zeros((len(v), 2 if d == 1 else d + d * d)))
    return dev


def with_data(model, y):
    """the same model with other data (rows as model.data_var)"""
    return dataclasses.replace(model, data_y=np.asarray(y, float).reshape(np.shape(model.data_y)))


# ---- the Kalman reference ----------------------------------------------------------------------------------------------------------
def chain_spec(model):
    """a chain of this module as the arrays of a time-varying state-space model, read from the model's META (the graph arrays go to the
    dense references): A [n-1, d, d], b [n-1, d], Q [n-1, d, d], H [d, d], R [n, d, d], y [n, d] (NaN where there is none), keep [n],
    lik [n] (factor id of the step's likelihood, -1 where there is none), T (states before the tail), h, and `reverse`: ssm_chain's
    transitions are CX_FACTOR_GAUSS_ADDITIVE, whose out end is the LOWER id, so the device's causal order runs backwards in time there"""
    m, d = model.meta, model.dim
    kind = m["kind"]
    h = int(m.get("tail", 0))
    n = len(model.x_ids)
    T = n - h
    keep = np.concatenate([np.asarray(m.get("keep", np.ones(T, bool))), np.zeros(h, bool)])
    lik = np.concatenate([np.asarray(m.get("lik_of_state", model.data_fac)), np.full(h, -1)])
    y = np.full((n, d), np.nan)
    y[keep] = np.asarray(model.data_y, float).reshape(-1, d)
    tp = np.asarray(m.get("tail_par", np.zeros((0,) + np.shape(model.factor_var)[1:])), float)
    eye = np.eye(d)
    if kind == "ssm_chain":
        q = np.concatenate([np.broadcast_to(m["q"], (T - 1,)), tp.reshape(-1)])
        A, b, Q = np.ones((n - 1, 1, 1)), np.zeros((n - 1, 1)), q.reshape(n - 1, 1, 1)
        H, R = eye, np.concatenate([np.broadcast_to(m["r"], (T,)), np.ones(h)]).reshape(n, 1, 1)
    elif kind == "ssm_chain_linear":
        tp = tp.reshape(-1, 3)
        A = np.concatenate([m["a"], tp[:, 1]]).reshape(n - 1, 1, 1)
        b = np.concatenate([m["b"], tp[:, 2]]).reshape(n - 1, 1)
        Q = np.concatenate([m["q"], tp[:, 0]]).reshape(n - 1, 1, 1)
        H, R = eye, np.full((n, 1, 1), float(m["r"]))
    else:
        assert kind == "lgssm_chain"
        A = np.broadcast_to(np.asarray(m["A"], float), (n - 1, d, d))
        b = np.zeros((n - 1, d))
        Q = np.broadcast_to(np.asarray(m["Q"], float), (n - 1, d, d))
        H, R = np.asarray(m.get("H", eye), float), np.broadcast_to(np.asarray(m["R"], float), (n, d, d))
    return dict(A=A, b=b, Q=Q, H=H, R=R, y=y, keep=keep, lik=lik, T=T, h=h, d=d, reverse=kind == "ssm_chain")


def _score(y, yh, S):
    Ls = np.linalg.cholesky(S)
    z = np.linalg.solve(Ls, y - yh)
    maha = float(z @ z)
    return -0.5 * (len(y) * LOG2PI + 2.0 * np.log(np.diag(Ls)).sum() + maha), maha


def kalman_filter(A, b, Q, H, R, y, keep, carry_gap=True):
    """x_{t+1} = A_t x_t + b_t + N(0, Q_t), y_t = H x_t + N(0, R_t) where keep[t]; flat prior on x_0, keep[0] true, H invertible.  At a
    step without a datum the update is skipped: the prediction is carried on.  Returns the filtered and predicted moments and, per
    observed step, (ŷ, S, log score, squared residual) — NaN at step 0, whose predictive is improper; log_first is its share of
    log p(y), -log|det H|.
    carry_gap=False is the WRONG filter of tests/test_missing_data_checkers.py: across a gap it predicts from the last filtered state with
    ONE transition, dropping the A P A' + Q accumulated over the gap."""
    n, d = y.shape
    assert keep[0]
    mf, Pf, mp, Pp = np.zeros((n, d)), np.zeros((n, d, d)), np.zeros((n, d)), np.zeros((n, d, d))
    yh, S, term, maha = np.full((n, d), np.nan), np.full((n, d, d), np.nan), np.full(n, np.nan), np.full(n, np.nan)
    Ri = np.linalg.inv(R[0])
    Pf[0] = np.linalg.inv(H.T @ Ri @ H)
    mf[0] = Pf[0] @ H.T @ Ri @ y[0]
    last = 0
    for t in range(1, n):
        src = t - 1 if carry_gap else last
        mp[t] = A[t - 1] @ mf[src] + b[t - 1]
        Pp[t] = A[t - 1] @ Pf[src] @ A[t - 1].T + Q[t - 1]
        Pp[t] = 0.5 * (Pp[t] + Pp[t].T)
        if not keep[t]:
            mf[t], Pf[t] = mp[t], Pp[t]
            continue
        last = t
        St = H @ Pp[t] @ H.T + R[t]
        St = 0.5 * (St + St.T)
        yh[t], S[t] = H @ mp[t], St
        term[t], maha[t] = _score(y[t], yh[t], St)
        K = np.linalg.solve(St, H @ Pp[t]).T
        mf[t] = mp[t] + K @ (y[t] - yh[t])
        P = Pp[t] - K @ H @ Pp[t]
        Pf[t] = 0.5 * (P + P.T)
    return dict(mf=mf, Pf=Pf, mp=mp, Pp=Pp, yhat=yh, S=S, term=term, maha=maha, log_first=-math.log(abs(np.linalg.det(H))))


def rts_smoother(A, f):
    """the RTS pass over kalman_filter's result: (means, covariances, lag-one covariances Cov(x_{t+1}, x_t | y))"""
    mf, Pf, mp, Pp = f["mf"], f["Pf"], f["mp"], f["Pp"]
    n, d = mf.shape
    ms, Ps, Pc = mf.copy(), Pf.copy(), np.zeros((n - 1, d, d))
    for t in range(n - 2, -1, -1):
        G = np.linalg.solve(Pp[t + 1], A[t] @ Pf[t]).T
        ms[t] = mf[t] + G @ (ms[t + 1] - mp[t + 1])
        P = Pf[t] + G @ (Ps[t + 1] - Pp[t + 1]) @ G.T
        Ps[t] = 0.5 * (P + P.T)
        Pc[t] = Ps[t + 1] @ G.T
    return ms, Ps, Pc


def kalman_missing(model, spec=None):
    """the filter and smoother of a chain of this module.  Returns {"mean" [n, d], "cov" [n, d, d], "lag_one" [n-1, d, d], "steps" (time
    index of the observed steps, in the order of their likelihood's factor id), "factor_ids", "yhat", "S", "log_density", "mahalanobis"
    (rows as steps; NaN for the one improper row), "log_first" (-log|det H|: what the improper row adds to log p(y)), "log_evidence",
    "forecast" ((mean [h, d], cov [h, d, d]) of the tail by m <- A m + b, P <- A P A' + Q from the smoothed last observed state, or None)}.
    The innovations run in the device's causal order: backwards in time on ssm_chain (chain_spec), where A = 1 makes the reversed
    series a chain of the same kind; the tail, which no datum follows, adds nothing to them."""
    s = chain_spec(model) if spec is None else spec
    A, b, Q, H, R, y, keep, T, h = (s[k] for k in ("A", "b", "Q", "H", "R", "y", "keep", "T", "h"))
    f = kalman_filter(A, b, Q, H, R, y, keep)
    ms, Ps, Pc = rts_smoother(A, f)
    if s["reverse"]:
        assert np.all(A == 1.0) and not np.any(b)
        r = kalman_filter(A[:T - 1][::-1], b[:T - 1][::-1], Q[:T - 1][::-1], H, R[:T][::-1], y[:T][::-1], keep[:T][::-1])
        inn = {k: np.concatenate([r[k][::-1], np.full((h,) + r[k].shape[1:], np.nan)]) for k in ("yhat", "S", "term", "maha")}
        assert abs(math.fsum(r["term"][keep[:T][::-1]][1:].tolist()) - math.fsum(f["term"][keep][1:].tolist())) <= 1e-9 * max(1.0, abs(np.nansum(f["term"])))
    else:
        inn = f
    steps = np.flatnonzero(keep)
    steps = steps[np.argsort(s["lik"][steps], kind="stable")]
    forecast = None
    if h:
        fm, fP = np.zeros((h, s["d"])), np.zeros((h, s["d"], s["d"]))
        m, P = ms[T - 1], Ps[T - 1]
        for k in range(h):
            m, P = A[T - 1 + k] @ m + b[T - 1 + k], A[T - 1 + k] @ P @ A[T - 1 + k].T + Q[T - 1 + k]
            fm[k], fP[k] = m, P
        forecast = (fm, fP)
    total = math.fsum(v for v in f["term"][keep].tolist() if not math.isnan(v))
    return {"mean": ms, "cov": Ps, "lag_one": Pc, "steps": steps, "factor_ids": s["lik"][steps], "yhat": inn["yhat"][steps], "S": inn["S"][steps],
            "log_density": inn["term"][steps], "mahalanobis": inn["maha"][steps], "log_first": f["log_first"],
            "log_evidence": total + f["log_first"], "forecast": forecast}


def ss_em_missing(model, A, Q, C, R, n_iter):
    """Shumway–Stoffer EM of a dim > 1 chain with missing observations (no tail), fed with kalman_missing's moments: the transition sums
    run over every step, the observation sums over the observed ones.  Returns (trace of n_iter + 1 log evidences, final (A, Q, C, R))."""
    s = chain_spec(model)
    n, d, keep, y = len(s["keep"]), s["d"], s["keep"], s["y"]
    assert s["h"] == 0
    par = tuple(np.array(z, float) for z in (A, Q, C, R))
    trace = []
    for it in range(n_iter + 1):
        A, Q, C, R = par
        sp = {**s, "A": np.broadcast_to(A, (n - 1, d, d)), "Q": np.broadcast_to(Q, (n - 1, d, d)), "H": C, "R": np.broadcast_to(R, (n, d, d))}
        k = kalman_missing(model, sp)
        trace.append(k["log_evidence"])
        if it == n_iter:
            break
        ms, Ps, Pc = k["mean"], k["cov"], k["lag_one"]
        Exx = Ps + ms[:, :, None] * ms[:, None, :]
        S11, S00 = Exx[1:].sum(0), Exx[:-1].sum(0)
        S10 = (Pc + ms[1:, :, None] * ms[:-1, None, :]).sum(0)
        yo = y[keep]
        Syy = (yo[:, :, None] * yo[:, None, :]).sum(0)
        Syx = (yo[:, :, None] * ms[keep][:, None, :]).sum(0)
        Sxx = Exx[keep].sum(0)
        A = S10 @ np.linalg.inv(S00)
        Q = (S11 - A @ S10.T - S10 @ A.T + A @ S00 @ A.T) / (n - 1)
        C = Syx @ np.linalg.inv(Sxx)
        R = (Syy - C @ Syx.T - Syx @ C.T + C @ Sxx @ C.T) / keep.sum()
        par = (A, 0.5 * (Q + Q.T), C, 0.5 * (R + R.T))
    return trace, par


def loo_reference_error(gm, dense_loo):
    """per leave-one-out row: how far the dense solve (predictive_support.dense_loo_all) and the message formula on exact messages
    (predictive_support.predictive_from_messages), two f64 computations of the same number that share no code, are apart — what the
    reference itself knows of that row (the scaled differences of predictive_support.assert_rows_close, the largest of the four)"""
    from tests import functional_support as F
    from tests import predictive_support as P

    msg = P.predictive_from_messages(gm, F.forest_bp(gm), mode=P.LOO)
    assert np.array_equal(msg["factor_ids"], dense_loo["factor_ids"]) and np.array_equal(msg["status"], dense_loo["status"])
    err = np.zeros(len(msg["factor_ids"]))
    for i in np.flatnonzero(msg["status"] == 0):
        for k in ("mean", "cov"):
            err[i] = max(err[i], float(np.max(np.abs(msg[k][i] - dense_loo[k][i])) / max(float(np.max(np.abs(dense_loo[k][i]))), 1e-300)))
        err[i] = max(err[i], abs(msg["log_density"][i] - dense_loo["log_density"][i]) / max(abs(dense_loo["log_density"][i]), 1e-300),
                     abs(msg["mahalanobis"][i] - dense_loo["mahalanobis"][i]) / (1.0 + abs(dense_loo["mahalanobis"][i])))
    return err


# ---- a plain chain pass in natural form (and a wrong one) -----------------------------------------------------------------------------
def chain_pass(model, empty_side_is_undefined=False):
    """forward and backward messages of a chain (no tail) in natural form, the side message of a state the likelihood's H' R^-1 H,
    H' R^-1 y — or NOTHING: the sum over no messages is (0, 0).  Returns the marginal (means, covariances).
    empty_side_is_undefined=True is the WRONG pass of tests/test_missing_data_checkers.py: it takes a state without a side message for
    one whose side message is not there YET (NaN, the marker of an undefined message), as a pass written for fully observed chains may."""
    s = chain_spec(model)
    A, b, Q, H, R, y, keep = (s[k] for k in ("A", "b", "Q", "H", "R", "y", "keep"))
    n, d = y.shape
    assert s["h"] == 0
    se, sl = np.zeros((n, d)), np.zeros((n, d, d))
    for t in range(n):
        if keep[t]:
            Ri = np.linalg.inv(R[t])
            se[t], sl[t] = H.T @ Ri @ y[t], H.T @ Ri @ H
        elif empty_side_is_undefined:
            se[t], sl[t] = np.nan, np.nan
    fe, fl, be, bl = np.zeros((n, d)), np.zeros((n, d, d)), np.zeros((n, d)), np.zeros((n, d, d))
    for t in range(n - 1):
        Qi = np.linalg.inv(Q[t])
        e, l = se[t] + fe[t], sl[t] + fl[t]
        J = l + A[t].T @ Qi @ A[t]
        G = Qi @ A[t] @ np.linalg.inv(J) if np.isfinite(J).all() else np.full((d, d), np.nan)
        fl[t + 1] = Qi - G @ A[t].T @ Qi
        fe[t + 1] = Qi @ b[t] + G @ (e - A[t].T @ Qi @ b[t])
    for t in range(n - 2, -1, -1):
        Qi = np.linalg.inv(Q[t])
        e, l = se[t + 1] + be[t + 1], sl[t + 1] + bl[t + 1]
        G = A[t].T @ Qi @ np.linalg.inv(l + Qi) if np.isfinite(l).all() else np.full((d, d), np.nan)
        bl[t] = A[t].T @ Qi @ A[t] - G @ Qi @ A[t]
        be[t] = -A[t].T @ Qi @ b[t] + G @ (e + Qi @ b[t])
    lam = sl + fl + bl
    eta = se + fe + be
    cov = np.full((n, d, d), np.nan)
    ok = np.isfinite(lam).all(axis=(1, 2))
    cov[ok] = np.linalg.inv(lam[ok])
    return np.einsum("nij,nj->ni", cov, eta), cov


# ---- the cases of the GPU tests --------------------------------------------------------------------------------------------------------
SCALAR_T, MV_T, CORE_T, READER_T = 3300, 700, 40, 40
SCALAR_RUN, MV_RUN, CORE_RUN = (600, 2900), (100, 650), (5, 30)
MV_K, CORE_K, CORE_FAN = (1, 5), 3, 2
CORE_DIMS = (7, 16, 20, 32, 64)
SCALAR_TILE, MV_LANES = 1024, 256


def base_chain(family, T, d=1):
    if family == "ssm":
        return cx.synth.ssm_chain(T, seed=41, random_variances=True)
    if family == "lin":
        return cx.synth.ssm_chain_linear(T, seed=42)
    if family == "iso":
        return cx.synth.lgssm_chain(T, d=d, seed=43)
    if family == "gen":
        return AN.chain(T, d)
    assert family == "genI"
    return AN.chain(T, d, general_h=False)


def pattern(name, n):
    if name == "alt":
        return alt(n)
    if name == "sparse":
        return sparse(n)
    if name.startswith("run"):
        a, b = (int(x) for x in name[4:-1].split(","))
        return run(n, a, b)
    if name.startswith("random"):
        return random_keep(n, float(name[7:-1]), 5)
    raise ValueError(name)


def make(family, T, d, pat=None, h=0):
    m = base_chain(family, T, d)
    if pat:
        m = thin(m, pattern(pat, T))
    return tail(m, h) if h else m


def thinned_comb(d, general=False):
    base = AN.comb(20, d, teeth=1) if general else cx.synth.lgssm_comb(20, d=d, teeth=1, seed=44)
    return thin(base, comb_alt(20, 1))


def _run_name(ab):
    return f"run({ab[0]},{ab[1]})"


def gpu_cases():
    """[(name, family, T, d, pattern or None, h)] of the chains, in the order of gpu_models()"""
    out = []
    for fam in ("ssm", "lin"):
        for pat in (_run_name(SCALAR_RUN), "alt", "sparse", "random(0.3)"):
            out.append((fam, SCALAR_T, 1, pat, 0))
        for h in (1, 5, 1500):
            out.append((fam, SCALAR_T, 1, None, h))
        for pat, h in (("alt", 0), ("sparse", 0), ("run(5,30)", 0), (None, 1), (None, 5), ("alt", 5)):
            out.append((fam, READER_T, 1, pat, h))
    for d in (2, 3, 4):
        for fam in ("iso", "gen", "genI"):
            for pat in (_run_name(MV_RUN), "alt", "sparse"):
                out.append((fam, MV_T, d, pat, 0))
        for fam in ("iso", "gen"):
            for pat, h in (("alt", 0), ("sparse", 0), ("run(5,30)", 0), (None, 1), (None, 5), ("alt", 5)):
                out.append((fam, READER_T, d, pat, h))
    for d in CORE_DIMS:
        for pat in (_run_name(CORE_RUN), "alt", "sparse"):
            out.append(("gen", CORE_T, d, pat, 0))
        for h in (1, 5):
            out.append(("gen", CORE_T, d, None, h))
    return [(case_name(*c),) + c for c in out]


def case_name(family, T, d, pat, h):
    return f"{family} T={T} d={d}" + (f" {pat}" if pat else "") + (f" tail={h}" if h else "")


def gpu_models():
    out = {name: (lambda f=f, T=T, d=d, p=p, h=h: make(f, T, d, p, h)) for name, f, T, d, p, h in gpu_cases()}
    for d in (2, 4, 16):
        out[f"comb 20 d={d} alt"] = lambda d=d: thinned_comb(d)
    for d in (2, 4):
        out[f"gen comb 20 d={d} alt"] = lambda d=d: thinned_comb(d, general=True)
    return out


def is_reader_size(model):
    """small enough for the O(rows n^3) dense leave-one-out reference"""
    return len(model.x_ids) <= 60 and model.dim <= 4
