"""Shared by the causal-marginal tests: two independent statements of what cx_causal_marginals returns, over the GModel
and the message arrays of tests/evidence_support.py.

  causal_from_messages   the definition — the classes U, O, T of the stored messages, the sums, the recursion for β — on arrays of
                         factor→variable messages (evidence_support.device_messages / numpy_bp)
  dense_causal           the marginal of x_i in the dense joint of the model in which the data the mode leaves out are made non-observed:
                         the data of i's descendants beyond the lag, and i's own for the predicted mode

A GModel states every rule factor as  Σ_e C_e x_e - b ~ N(0, Q)  with entry 0 the CX_ROLE_OUT end (C_0 = I) and the others CX_ROLE_IN
(CX_FACTOR_GAUSS_ADDITIVE: the lower variable id first, C = (1, -1), b = 0), as tests/predictive_support.py reads it.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from tests import evidence_support as E
from tests import predictive_support as P

PREDICTED, FILTERED = 0, 1


def scalar_tree(parent, seed=3):
    """a dim-1 tree with every transition pointing away from the root — x_c = a x_p + b + N(0, q) (CX_FACTOR_GAUSS_LINEAR, the parent on
    the CX_ROLE_IN end), parent[c] < c, parent[0] = -1 — and an additive likelihood on every state: the scalar counterpart of
    anisotropic.comb / branching, whose graphs name parameter sets and have no dim-1 form"""
    import cortex.jl_amd as cx
    from cortex.jl_amd import _lib as L

    parent = np.asarray(parent, np.int64)
    n = len(parent)
    assert parent[0] == -1 and np.all(parent[1:] < np.arange(1, n)) and np.all(parent[1:] >= 0)
    rng = np.random.default_rng([seed, n, 83])
    x = np.arange(1, n + 1, dtype=np.int64)
    y, lik, tr = x + n, x + 2 * n, 3 * n + np.arange(1, n, dtype=np.int64)
    at = 0.9 * rng.uniform(0.8, 1.2, n - 1) * rng.choice([1.0, -1.0], n - 1, p=[0.8, 0.2])
    bt, qt, r = 0.3 * rng.standard_normal(n - 1), 0.5 * rng.uniform(0.5, 2.0, n - 1), 0.7
    params = np.zeros((2 * n - 1, 3))
    params[:n, 0] = r
    params[n:, 0], params[n:, 1], params[n:, 2] = qt, at, bt
    state = np.empty(n)
    state[0] = rng.standard_normal()
    for c in range(1, n):
        state[c] = at[c - 1] * state[parent[c]] + bt[c - 1] + np.sqrt(qt[c - 1]) * rng.standard_normal()
    kind = np.concatenate([np.full(n, L.FACTOR_GAUSS_ADDITIVE), np.full(n - 1, L.FACTOR_GAUSS_LINEAR)]).astype(np.int32)
    return cx.synth.Model(edge_var=np.concatenate([y, x, x[parent[1:]], x[1:]]), edge_fac=np.concatenate([lik, lik, tr, tr]),
                          factor_ids=np.concatenate([lik, tr]), factor_kind=kind, factor_var=params, x_ids=x, data_var=y, data_fac=lik,
                          data_y=state + np.sqrt(r) * rng.standard_normal(n),
                          edge_role=np.concatenate([np.full(2 * n, L.ROLE_OUT), np.full(n - 1, L.ROLE_IN), np.full(n - 1, L.ROLE_OUT)]).astype(np.int32),
                          meta={"kind": "scalar_tree", "parent": parent})


def comb_parents(n_spine, teeth):
    """a spine with a path of `teeth` states hanging on every spine state"""
    par = [-1] + list(range(n_spine - 1))
    for s in range(n_spine):
        p = s
        for _ in range(teeth):
            par.append(p)
            p = len(par) - 1
    return par


def branching_parents(n, b):
    return [-1] + [(c - 1) // b for c in range(1, n)]


def _additive(gm, k, C, b):
    return gm.d == 1 and k == 2 and C[0, 0, 0] == 1.0 and C[1, 0, 0] == -1.0 and b[0] == 0.0


def classes(gm):
    """per variable index: lists U, O, T of (k, row in group k, entry) — the messages into it from rule factors, by class (the opaque
    messages are all U and are not listed)"""
    nv = len(gm.var_ids)
    U, O, T = ([[] for _ in range(nv)] for _ in range(3))
    for k, g in gm.groups.items():
        for fi, (V, C, b) in enumerate(zip(g["vars"], g["C"], g["b"])):
            for j in range(k):
                v = int(V[j])
                if gm.obs[v]:
                    continue
                if j == 0:
                    own = _additive(gm, k, C, b) and gm.obs[V[1]]
                    (O if own else U)[v].append((k, fi, j))
                else:
                    (O if gm.obs[V[0]] else T)[v].append((k, fi, j))
    return U, O, T


def _rule_to_in(g, fi, eta, lam):
    """the message of pair factor fi (entries: out, in) towards its `in` end, given the message (eta, lam) from its `out` end"""
    C, b, Q = g["C"][fi], g["b"][fi], g["Q"][fi]
    Qi = np.linalg.inv(Q)
    C1 = C[1]
    M = Qi + lam
    G = C1.T @ Qi
    l = G @ C1 - G @ np.linalg.solve(M, G.T)
    e = G @ b - G @ np.linalg.solve(M, Qi @ b + eta)
    return e, 0.5 * (l + l.T)


def _result(gm):
    nv, d = len(gm.var_ids), gm.d
    return {"variable_ids": gm.var_ids.copy(), "mean": np.full((nv, d), np.nan), "cov": np.full((nv, d, d), np.nan), "status": np.zeros(nv, np.int64)}


def _finish(res):
    st = res["status"]
    res["counts"] = {"rows": len(st), "finite": int((st == 0).sum()), "undefined": int((st == 1).sum()), "improper": int((st == 2).sum())}
    return res


def _moments(res, v, eta, lam):
    if np.isnan(eta).any() or np.isnan(lam).any():
        res["status"][v] = 1
        return
    try:
        np.linalg.cholesky(lam)
    except np.linalg.LinAlgError:
        res["status"][v] = 2
        return
    S = np.linalg.inv(lam)
    S = 0.5 * (S + S.T)
    res["mean"][v], res["cov"][v] = S @ eta, S


def causal_from_messages(gm, f2v, opq=None, mode=FILTERED, lag=0):
    """f2v, opq: as evidence_support.bethe_log_z takes them.  Every variable of gm in ascending id: {"variable_ids", "mean", "cov",
    "status" (0 finite, 1 an undefined input, 2 improper), "counts"}"""
    assert mode in (PREDICTED, FILTERED) and lag >= 0 and (lag == 0 or mode == FILTERED)
    d, nv = gm.d, len(gm.var_ids)
    oe, ol = (gm.opq_eta, gm.opq_lam) if opq is None else opq
    U, O, T = classes(gm)
    su_e, su_l, so_e, so_l = np.zeros((nv, d)), np.zeros((nv, d, d)), np.zeros((nv, d)), np.zeros((nv, d, d))
    np.add.at(su_e, gm.opq_var, oe)
    np.add.at(su_l, gm.opq_var, ol)
    for v in range(nv):
        for (k, fi, j) in U[v]:
            su_e[v] += f2v[k][0][fi, j]; su_l[v] += f2v[k][1][fi, j]
        for (k, fi, j) in O[v]:
            so_e[v] += f2v[k][0][fi, j]; so_l[v] += f2v[k][1][fi, j]
    beta = {}                                        # (k, fi, j) -> (eta, lam); absent: flat
    for _ in range(lag):
        new = {}
        for v in range(nv):
            for (k, fi, j) in T[v]:
                assert k == 2, "the recursion runs through factors of two variables"
                g = gm.groups[k]
                o = int(g["vars"][fi, 0])
                e, l = so_e[o].copy(), so_l[o].copy()
                for t in T[o]:
                    if t in beta:
                        e += beta[t][0]; l += beta[t][1]
                if not e.any() and not l.any():
                    continue                         # nothing downstream has been seen: flat
                new[(k, fi, j)] = _rule_to_in(g, fi, e, l)
        beta = new
    res = _result(gm)
    for v in range(nv):
        if gm.obs[v]:
            res["mean"][v], res["cov"][v] = gm.y[v], 0.0
            continue
        e, l = su_e[v].copy(), su_l[v].copy()
        if mode == FILTERED:
            e += so_e[v]; l += so_l[v]
        for t in T[v]:
            if t in beta:
                e += beta[t][0]; l += beta[t][1]
        _moments(res, v, e, l)
    return _finish(res)


def left_out(gm, i, mode, lag):
    """the observed variables whose data the mode leaves out of variable index i's estimate"""
    _U, O, T = classes(gm)
    dist, front = {int(i): 0}, [int(i)]
    while front:
        nxt = []
        for v in front:
            for (k, fi, _j) in T[v]:
                o = int(gm.groups[k]["vars"][fi, 0])
                if o not in dist:
                    dist[o] = dist[v] + 1
                    nxt.append(o)
        front = nxt
    out = set()
    for v, s in dist.items():
        if s > lag or (v == i and mode == PREDICTED):
            for (k, fi, j) in O[v]:
                out.update(int(u) for u in gm.groups[k]["vars"][fi] if gm.obs[u])
    return sorted(out)


def dense_causal(gm, i, mode=FILTERED, lag=0):
    """(mean, cov) of variable index i, or None where the joint precision of what is left is not positive definite"""
    obs = gm.obs.copy()
    obs[left_out(gm, i, mode, lag)] = False
    g2 = dataclasses.replace(gm, obs=obs)
    d = gm.d
    free = np.flatnonzero(~obs)
    fpos = -np.ones(len(gm.var_ids), np.int64)
    fpos[free] = np.arange(len(free))
    n = len(free) * d
    J, h = np.zeros((n, n)), np.zeros(n)
    for g in g2.groups.values():                     # (the J and h of evidence_support.dense_log_z)
        for vs, C, b, Q in zip(g["vars"], g["C"], g["b"], g["Q"]):
            Qi = np.linalg.inv(Q)
            bp = b - sum(C[j] @ gm.y[v] for j, v in enumerate(vs) if obs[v])
            fr = [(j, fpos[v]) for j, v in enumerate(vs) if not obs[v]]
            for j, a in fr:
                h[a * d:(a + 1) * d] += C[j].T @ Qi @ bp
                for l, c in fr:
                    J[a * d:(a + 1) * d, c * d:(c + 1) * d] += C[j].T @ Qi @ C[l]
    for v, eta, lam in zip(gm.opq_var, gm.opq_eta, gm.opq_lam):
        if obs[v] or np.isnan(eta).any() or np.isnan(lam).any():
            continue
        a = fpos[v]
        J[a * d:(a + 1) * d, a * d:(a + 1) * d] += lam
        h[a * d:(a + 1) * d] += eta
    ev = np.linalg.eigvalsh(J)
    if not ev[0] > 1e-12 * ev[-1]:
        return None
    S = np.linalg.inv(J)
    S = 0.5 * (S + S.T)
    a = fpos[i]
    return (S @ h)[a * d:(a + 1) * d], S[a * d:(a + 1) * d, a * d:(a + 1) * d]


def dense_causal_all(gm, mode=FILTERED, lag=0):
    """dense_causal of every variable, in the layout of causal_from_messages"""
    res = _result(gm)
    for v in range(len(gm.var_ids)):
        if gm.obs[v]:
            res["mean"][v], res["cov"][v] = gm.y[v], 0.0
            continue
        got = dense_causal(gm, v, mode, lag)
        if got is None:
            res["status"][v] = 2
        else:
            res["mean"][v], res["cov"][v] = got
    return _finish(res)


def as_rows(res, pick=None):
    """a result in the layout predictive_support.assert_rows_close compares (its two score columns: zeros)"""
    ids = np.asarray(res["variable_ids"] if res.get("variable_ids") is not None else np.arange(len(res["mean"])))
    sel = slice(None) if pick is None else pick
    n = len(ids[sel])
    return {"factor_ids": ids[sel], "mean": np.asarray(res["mean"])[sel], "cov": np.asarray(res["cov"])[sel], "log_density": np.zeros(n), "mahalanobis": np.zeros(n)}


def assert_close(got, want, tol, what="", pick=None):
    """mean and cov of two results row by row, by predictive_support.assert_rows_close (vectors and matrices scaled by their largest entry;
    the NaN patterns must agree)"""
    return P.assert_rows_close(as_rows(got, pick), as_rows(want, pick), tol, what)
