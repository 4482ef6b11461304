"""Shared by the log-evidence tests: three independent statements of log p(data) for a Gaussian synth.Model.

  dense_log_z       the joint information matrix of the non-observed variables (data folded in): ½ h'J⁻¹h - ½ log det J + (n/2) log 2π
                    plus the factors' and the opaque messages' constants
  bethe_log_z       the formula of cx_log_evidence from arrays of factor→variable messages, vectorised, in the same
                    centred coordinates
  kalman_log_lik    the prediction-error decomposition of a chain's data (flat prior on the first state)

plus a numpy Gaussian BP (flooding, lazy on undefined inputs) that gives exact messages on forests and the Bethe fixed point on loops.
A model is first turned into a GModel: every rule factor as a residual  Σ_e C_e x_e - b ~ N(0, Q)  over its variables, the opaque
(caller-set) messages in natural form, the data.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L

LOG2PI = math.log(2.0 * math.pi)


@dataclass
class GModel:
    d: int
    var_ids: np.ndarray                 # every variable that occurs, ascending
    obs: np.ndarray                     # [nv] bool
    y: np.ndarray                       # [nv, d] data (observed variables)
    groups: dict = field(default_factory=dict)   # arity k -> dict(fid [n], vars [n, k] (indices), C [n, k, d, d], b [n, d], Q [n, d, d])
    opq_var: np.ndarray = None          # [no] variable index of each opaque message
    opq_fac: np.ndarray = None          # [no] its factor id
    opq_eta: np.ndarray = None          # [no, d]
    opq_lam: np.ndarray = None          # [no, d, d]


def _row(p):
    p = np.atleast_1d(np.asarray(p, dtype=np.float64))
    return np.concatenate([p, np.zeros(4 - len(p))])


def gmodel(model, coef=None, edge_sets=None, opaque=None, psets=None) -> GModel:
    """model: synth.Model.  coef: {(var id, fac id): a} of LINEAR_N inputs (default: the model's meta, else 1).  edge_sets: {(var id, fac id):
    set} (dim > 1 LINEAR_N inputs).  opaque: (var ids, fac ids, eta [n, d], Lambda [n, d, d]) in place of the model's prior_* arrays.
    psets: {set: (A, Q)} in place of the model's."""
    d = model.dim
    psets = model.psets if psets is None else psets
    fast = _gmodel_additive(model) if d == 1 and coef is None and opaque is None else None
    if fast is not None:
        return fast
    var_ids = np.unique(model.edge_var)
    vpos = {int(v): i for i, v in enumerate(var_ids)}
    obs = np.zeros(len(var_ids), bool)
    y = np.zeros((len(var_ids), d))
    for v, yy in zip(model.data_var, np.asarray(model.data_y).reshape(len(model.data_var), d) if len(model.data_var) else []):
        obs[vpos[int(v)]] = True
        y[vpos[int(v)]] = yy
    if coef is None:
        coef = {}
        meta = model.meta
        if "all_coef" in meta:
            coef = {(int(v), int(f)): float(a) for v, f, a in zip(meta["all_coef_var"], meta["all_coef_fac"], meta["all_coef"])}
        elif "coef" in meta:
            coef = {(int(v), int(f)): float(a) for v, f, a in zip(meta["coef_var"], meta["coef_fac"], meta["coef"])}
    edge_sets = edge_sets or {}
    role = model.edge_role if model.edge_role is not None else np.full(len(model.edge_var), L.ROLE_OUT, np.int32)
    by_fac = {}
    for v, f, r in zip(model.edge_var, model.edge_fac, role):
        by_fac.setdefault(int(f), []).append((int(v), int(r)))
    groups = {}
    I = np.eye(d)
    for fi, (fid, kind) in enumerate(zip(model.factor_ids, model.factor_kind)):
        fid, kind = int(fid), int(kind)
        if kind == L.FACTOR_OPAQUE:
            continue
        p = _row(model.factor_var[fi])
        edges = sorted(by_fac[fid])
        if d == 1:
            if kind == L.FACTOR_GAUSS_ADDITIVE:
                vs, C, b, Q = [edges[0][0], edges[1][0]], [I, -I], np.zeros(1), p[0] * I
            elif kind == L.FACTOR_GAUSS_LINEAR:
                out = [v for v, r in edges if r == L.ROLE_OUT][0]
                inn = [v for v, r in edges if r == L.ROLE_IN][0]
                vs, C, b, Q = [out, inn], [I, -p[1] * I], np.array([p[2]]), p[0] * I
            else:
                out = [v for v, r in edges if r == L.ROLE_OUT][0]
                ins = [v for v, r in edges if r == L.ROLE_IN]
                vs = [out] + ins
                C = [I] + [-coef.get((v, fid), 1.0) * I for v in ins]
                b, Q = np.array([p[1]]), p[0] * I
        else:
            s0 = int(p[0])
            A0, Q = psets[s0]
            out = [v for v, r in edges if r == L.ROLE_OUT][0]
            ins = [v for v, r in edges if r == L.ROLE_IN]
            vs = [out] + ins
            C = [I] + [-np.asarray(psets[edge_sets.get((v, fid), s0)][0]) for v in ins]
            b = np.zeros(d)
        k = len(vs)
        g = groups.setdefault(k, {"fid": [], "vars": [], "C": [], "b": [], "Q": []})
        g["fid"].append(fid); g["vars"].append([vpos[v] for v in vs]); g["C"].append(np.stack(C)); g["b"].append(b); g["Q"].append(np.asarray(Q, float))
    for k, g in groups.items():
        groups[k] = {"fid": np.asarray(g["fid"], np.int64), "vars": np.asarray(g["vars"], np.int64), "C": np.asarray(g["C"]), "b": np.asarray(g["b"]),
                     "Q": np.asarray(g["Q"])}
    if opaque is None:
        if len(model.prior_var):
            pv = np.asarray(model.prior_var).reshape(-1)
            var = np.asarray(model.prior_variance, float).reshape(len(pv))
            eta = (np.asarray(model.prior_mean, float) / var).reshape(len(pv), 1)
            lam = (1.0 / var).reshape(len(pv), 1, 1)
            opaque = (pv, np.asarray(model.prior_fac), eta, lam)
        else:
            opaque = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, d)), np.zeros((0, d, d)))
    ov, of, oe, ol = opaque
    return GModel(d=d, var_ids=var_ids, obs=obs, y=y, groups=groups, opq_var=np.asarray([vpos[int(v)] for v in ov], np.int64),
                  opq_fac=np.asarray(of, np.int64), opq_eta=np.asarray(oe, float).reshape(len(ov), d), opq_lam=np.asarray(ol, float).reshape(len(ov), d, d))


def _gmodel_additive(model):
    """gmodel of a scalar model whose rule factors are all CX_FACTOR_GAUSS_ADDITIVE (the grids: millions of factors), vectorised"""
    kinds = np.asarray(model.factor_kind)
    rule = kinds != L.FACTOR_OPAQUE
    if not (kinds[rule] == L.FACTOR_GAUSS_ADDITIVE).all():
        return None
    var_ids = np.unique(model.edge_var)
    ev = np.searchsorted(var_ids, model.edge_var)
    fids = np.asarray(model.factor_ids)[rule]
    q = np.asarray(model.factor_var, float).reshape(len(kinds), -1)[rule, 0]
    order = np.argsort(fids)
    fids, q = fids[order], q[order]
    pos = np.searchsorted(fids, model.edge_fac)
    on = (pos < len(fids)) & (fids[np.minimum(pos, len(fids) - 1)] == model.edge_fac)
    e_on = np.flatnonzero(on)
    e_on = e_on[np.lexsort((ev[e_on], pos[e_on]))]          # by factor, then variable
    if len(e_on) != 2 * len(fids):
        return None
    vars_ = ev[e_on].reshape(-1, 2)
    n = len(fids)
    obs = np.zeros(len(var_ids), bool)
    y = np.zeros((len(var_ids), 1))
    if len(model.data_var):
        dv = np.searchsorted(var_ids, model.data_var)
        obs[dv] = True
        y[dv, 0] = model.data_y
    C = np.zeros((n, 2, 1, 1)); C[:, 0] = 1.0; C[:, 1] = -1.0
    groups = {2: {"fid": fids.astype(np.int64), "vars": vars_.astype(np.int64), "C": C, "b": np.zeros((n, 1)), "Q": q.reshape(n, 1, 1)}}
    pv = np.asarray(model.prior_var).reshape(-1)
    var = np.asarray(model.prior_variance, float).reshape(len(pv))
    return GModel(d=1, var_ids=var_ids, obs=obs, y=y, groups=groups, opq_var=np.searchsorted(var_ids, pv).astype(np.int64),
                  opq_fac=np.asarray(model.prior_fac, np.int64).reshape(len(pv)), opq_eta=(np.asarray(model.prior_mean, float) / var).reshape(len(pv), 1),
                  opq_lam=(1.0 / var).reshape(len(pv), 1, 1))


def _pd(lam):
    """[n, d, d] -> [n] bool: positive definite"""
    if len(lam) == 0:
        return np.zeros(0, bool)
    with np.errstate(invalid="ignore"):
        ev = np.linalg.eigvalsh(np.where(np.isnan(lam), 0.0, lam))
    return (ev[:, 0] > 0) & ~np.isnan(lam).any(axis=(1, 2))


# ---- dense --------------------------------------------------------------------------------------------------------------------------
def dense_log_z(gm: GModel) -> float:
    d = gm.d
    free = np.flatnonzero(~gm.obs)
    fpos = -np.ones(len(gm.var_ids), np.int64)
    fpos[free] = np.arange(len(free))
    n = len(free) * d
    J, h, const = np.zeros((n, n)), np.zeros(n), 0.0
    for g in gm.groups.values():
        for vs, C, b, Q in zip(g["vars"], g["C"], g["b"], g["Q"]):
            Qi = np.linalg.inv(Q)
            bp = b - sum(C[j] @ gm.y[v] for j, v in enumerate(vs) if gm.obs[v])
            const += -0.5 * bp @ Qi @ bp - 0.5 * np.linalg.slogdet(2 * np.pi * Q)[1]
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
        if _pd(lam[None])[0]:
            const += -0.5 * eta @ np.linalg.solve(lam, eta) + 0.5 * np.linalg.slogdet(lam)[1] - 0.5 * d * LOG2PI
    if n == 0:
        return const
    sign, ld = np.linalg.slogdet(J)
    assert sign > 0, "the joint precision is not positive definite"
    return float(const + 0.5 * h @ np.linalg.solve(J, h) - 0.5 * ld + 0.5 * n * LOG2PI)


# ---- the formula of cx_log_evidence from messages -------------------------------------------------------------------------------------
def bethe_log_z(gm: GModel, f2v: dict, opq_msgs=None) -> float:
    """f2v: arity k -> (eta [n, k, d], Lambda [n, k, d, d]), the stored factor→variable message of every edge of the group's factors
    (entries into observed variables are ignored).  opq_msgs: (eta [no, d], Lambda [no, d, d]) of the opaque messages (default: the
    model's).  Returns the value (NaN when a term reads an undefined message or a belief that is not positive definite)."""
    d, nv = gm.d, len(gm.var_ids)
    oe, ol = (gm.opq_eta, gm.opq_lam) if opq_msgs is None else opq_msgs
    M_eta, M_lam, deg = np.zeros((nv, d)), np.zeros((nv, d, d)), np.zeros(nv, np.int64)
    for k, g in gm.groups.items():
        e, l = f2v[k]
        for j in range(k):
            np.add.at(M_eta, g["vars"][:, j], e[:, j])
            np.add.at(M_lam, g["vars"][:, j], l[:, j])
            np.add.at(deg, g["vars"][:, j], 1)
    np.add.at(M_eta, gm.opq_var, oe)
    np.add.at(M_lam, gm.opq_var, ol)
    free = ~gm.obs
    pd = _pd(M_lam)
    mu = np.zeros((nv, d))
    if pd.any():
        mu[pd] = np.linalg.solve(M_lam[pd], M_eta[pd][..., None])[..., 0]
    eta_c = np.where(pd[:, None], 0.0, M_eta)          # the belief's natural mean in centred coordinates (0 where centred)
    terms = []
    bad = False
    # variables
    vt = free & (deg != 1)
    if vt.any():
        if np.isnan(M_lam[vt]).any() or np.isnan(M_eta[vt]).any() or not pd[vt].all():
            bad = True
        else:
            terms.append((1 - deg[vt]) * (0.5 * d * LOG2PI - 0.5 * np.linalg.slogdet(M_lam[vt])[1]))
    # opaque messages, centred
    keep = free[gm.opq_var] & ~np.isnan(oe).any(axis=1) & ~np.isnan(ol).any(axis=(1, 2))
    if keep.any():
        v, e, l = gm.opq_var[keep], oe[keep], ol[keep]
        m = mu[v]
        r = e - np.einsum("nij,nj->ni", l, m)
        opd = _pd(l)
        t = np.einsum("ni,ni->n", m, e) - 0.5 * np.einsum("ni,nij,nj->n", m, l, m)
        if opd.any():
            q = np.einsum("ni,ni->n", r[opd], np.linalg.solve(l[opd], r[opd][..., None])[..., 0])
            t[opd] = -0.5 * q + 0.5 * np.linalg.slogdet(l[opd])[1] - 0.5 * d * LOG2PI
        terms.append(t)
    # factors
    for k, g in gm.groups.items():
        e, l = f2v[k]
        V, C, b, Q = g["vars"], g["C"], g["b"], g["Q"]
        n = len(V)
        fr = free[V]                                    # [n, k]
        x = np.where(fr[..., None], mu[V], gm.y[V])     # data, or the centre
        lt = M_lam[V] - l                               # leave-one-out precision
        et = eta_c[V] - (e - np.einsum("nkij,nkj->nki", l, mu[V]))
        undefined = ((np.isnan(lt).any(axis=(2, 3)) | np.isnan(et).any(axis=2)) & fr).any(axis=1)
        if undefined.any():
            bad = True
            continue
        Qi = np.linalg.inv(Q)
        ldq = np.linalg.slogdet(2 * np.pi * Q)[1]
        bp = b - np.einsum("nkij,nkj->ni", C, x)
        g_ = np.einsum("nij,nj->ni", Qi, bp)
        c = -0.5 * np.einsum("ni,ni->n", bp, g_) - 0.5 * ldq
        # joint over all k entries; observed entries decoupled (identity block, zero right-hand side)
        Jb = np.einsum("nkpi,npq,nlqj->nkilj", C, Qi, C)            # [n, k, d, k, d]
        hb = np.einsum("nkpi,np->nki", C, g_) + et
        for j in range(k):
            Jb[:, j, :, j, :] += np.where(fr[:, j, None, None], lt[:, j], 0.0)
        mask = fr[:, :, None, None, None] & fr[:, None, None, :, None]
        Jb = np.where(mask, Jb, 0.0)
        for j in range(k):
            Jb[:, j, :, j, :] += np.where(fr[:, j, None, None], 0.0, np.eye(d))
        hb = np.where(fr[..., None], hb, 0.0)
        J = Jb.reshape(n, k * d, k * d)
        hv = hb.reshape(n, k * d)
        sign, ld = np.linalg.slogdet(J)
        if not (sign > 0).all():
            bad = True
            continue
        quad = np.einsum("ni,ni->n", hv, np.linalg.solve(J, hv[..., None])[..., 0])
        N = fr.sum(axis=1) * d
        terms.append(c + 0.5 * quad - 0.5 * ld + 0.5 * N * LOG2PI)
    if bad:
        return float("nan")
    return math.fsum(np.concatenate([np.atleast_1d(t) for t in terms]).tolist()) if terms else 0.0


# ---- messages ---------------------------------------------------------------------------------------------------------------------
def device_messages(gm: GModel, dev):
    """the stored factor→variable messages of every group edge and every opaque edge, natural form, from a DeviceGraph"""
    d = gm.d
    out = {}
    for k, g in gm.groups.items():
        vids = gm.var_ids[g["vars"]].reshape(-1)
        fids = np.repeat(g["fid"], k)
        m = dev.get_messages(vids, fids, L.TO_VARIABLE, L.FORM_NATURAL)
        out[k] = (m[:, :d].reshape(len(g["fid"]), k, d), m[:, d:].reshape(len(g["fid"]), k, d, d))
    m = dev.get_messages(gm.var_ids[gm.opq_var], gm.opq_fac, L.TO_VARIABLE, L.FORM_NATURAL) if len(gm.opq_var) else np.zeros((0, d + d * d))
    return out, (m[:, :d], m[:, d:].reshape(len(m), d, d))


def numpy_bp(gm: GModel, max_iter: int = 500, tol: float = 1e-13, seed_precision=None):
    """flooding Gaussian BP on the GModel; a message is computed once all its inputs are defined (undefined = NaN).  Returns the f2v
    dict bethe_log_z takes.  On a forest the fixed point is exact.  seed_precision: start every message at N(0, I / seed_precision)
    instead of undefined (loopy graphs)."""
    d, nv = gm.d, len(gm.var_ids)
    if seed_precision is None:
        f2v = {k: (np.full((len(g["fid"]), k, d), np.nan), np.full((len(g["fid"]), k, d, d), np.nan)) for k, g in gm.groups.items()}
    else:
        f2v = {k: (np.zeros((len(g["fid"]), k, d)), np.broadcast_to(seed_precision * np.eye(d), (len(g["fid"]), k, d, d)).copy()) for k, g in gm.groups.items()}
    opq_M_eta, opq_M_lam = np.zeros((nv, d)), np.zeros((nv, d, d))
    np.add.at(opq_M_eta, gm.opq_var, gm.opq_eta)
    np.add.at(opq_M_lam, gm.opq_var, gm.opq_lam)
    for _ in range(max_iter):
        # sums over the defined messages and, per variable, how many are undefined: a leave-one-out sum is defined when the
        # one left out is the only undefined one
        M_eta, M_lam, n_undef = opq_M_eta.copy(), opq_M_lam.copy(), np.zeros(nv, np.int64)
        for k, g in gm.groups.items():
            e, l = f2v[k]
            for j in range(k):
                u = np.isnan(e[:, j]).any(axis=1) | np.isnan(l[:, j]).any(axis=(1, 2))
                np.add.at(M_eta, g["vars"][:, j], np.where(u[:, None], 0.0, e[:, j]))
                np.add.at(M_lam, g["vars"][:, j], np.where(u[:, None, None], 0.0, l[:, j]))
                np.add.at(n_undef, g["vars"][:, j], u)
        delta = 0.0
        new = {}
        for k, g in gm.groups.items():
            e, l = f2v[k]
            ne, nl = e.copy(), l.copy()
            for fi in range(len(g["fid"])):
                V, C, b, Q = g["vars"][fi], g["C"][fi], g["b"][fi], g["Q"][fi]
                Qi = np.linalg.inv(Q)
                fr = [j for j in range(k) if not gm.obs[V[j]]]
                bp = b - sum(C[j] @ gm.y[V[j]] for j in range(k) if gm.obs[V[j]])
                own_u = {o: bool(np.isnan(e[fi, o]).any() or np.isnan(l[fi, o]).any()) for o in fr}
                for j in fr:
                    others = [o for o in fr if o != j]
                    if any(n_undef[V[o]] - own_u[o] > 0 for o in others):
                        continue
                    ve = [M_eta[V[o]] - (0.0 if own_u[o] else e[fi, o]) for o in others]
                    vl = [M_lam[V[o]] - (0.0 if own_u[o] else l[fi, o]) for o in others]
                    Jjj = C[j].T @ Qi @ C[j]
                    hj = C[j].T @ Qi @ bp
                    if others:
                        no = len(others)
                        Joo = np.zeros((no * d, no * d)); ho = np.zeros(no * d); Jjo = np.zeros((d, no * d))
                        for a, oa in enumerate(others):
                            ho[a * d:(a + 1) * d] = C[oa].T @ Qi @ bp + ve[a]
                            Jjo[:, a * d:(a + 1) * d] = C[j].T @ Qi @ C[oa]
                            for c_, oc in enumerate(others):
                                Joo[a * d:(a + 1) * d, c_ * d:(c_ + 1) * d] = C[oa].T @ Qi @ C[oc] + (vl[a] if a == c_ else 0.0)
                        Jjj = Jjj - Jjo @ np.linalg.solve(Joo, Jjo.T)
                        hj = hj - Jjo @ np.linalg.solve(Joo, ho)
                    if not np.isnan(e[fi, j]).any():
                        delta = max(delta, float(np.max(np.abs(hj - e[fi, j]))), float(np.max(np.abs(Jjj - l[fi, j]))))
                    else:
                        delta = np.inf
                    ne[fi, j], nl[fi, j] = hj, 0.5 * (Jjj + Jjj.T)
            new[k] = (ne, nl)
        f2v = new
        if delta <= tol:
            break
    return f2v


# ---- Kalman ----------------------------------------------------------------------------------------------------------------------
def kalman_log_lik(A, b, Q, R, y) -> float:
    """log p(y_1..y_T) of x_{t+1} = A_t x_t + b_t + N(0, Q_t), y_t = x_t + N(0, R_t), with a FLAT prior on x_1 (the graphs of
    synth.ssm_chain / ssm_chain_linear / lgssm_chain have no prior factor): ∫ N(y_1; x_1, R_1) dx_1 = 1, x_1 | y_1 ~ N(y_1, R_1), then the
    prediction errors.  A, b, Q: [T-1, d, d], [T-1, d], [T-1, d, d]; R: [T, d, d]; y: [T, d].  d == 1 runs on plain floats."""
    T, d = y.shape
    if d == 1:
        a_, b_, q_, r_, yy = (np.asarray(z, float).reshape(-1).tolist() for z in (A, b, Q, R, y))
        m, P, ll = yy[0], r_[0], 0.0
        log, c = math.log, -0.5 * LOG2PI
        for t in range(1, T):
            mp = a_[t - 1] * m + b_[t - 1]
            Pp = a_[t - 1] * a_[t - 1] * P + q_[t - 1]
            S = Pp + r_[t]
            e = yy[t] - mp
            ll += c - 0.5 * log(S) - 0.5 * e * e / S
            K = Pp / S
            m = mp + K * e
            P = Pp - K * Pp
        return ll
    m, P, ll = y[0].copy(), R[0].copy(), 0.0
    for t in range(1, T):
        mp = A[t - 1] @ m + b[t - 1]
        Pp = A[t - 1] @ P @ A[t - 1].T + Q[t - 1]
        S = Pp + R[t]
        Ls = np.linalg.cholesky(S)
        e = y[t] - mp
        z = np.linalg.solve(Ls, e)
        ll += -0.5 * d * LOG2PI - np.log(np.diag(Ls)).sum() - 0.5 * z @ z
        K = np.linalg.solve(S, Pp).T
        m = mp + K @ e
        P = Pp - K @ Pp
        P = 0.5 * (P + P.T)
    return float(ll)


def kalman_of_chain(model) -> float:
    """kalman_log_lik of a synth.ssm_chain / ssm_chain_linear / lgssm_chain model"""
    kind, T, d = model.meta["kind"], model.meta["T"], model.dim
    y = np.asarray(model.data_y, float).reshape(T, d)
    if kind == "ssm_chain":
        r, q = np.broadcast_to(model.meta["r"], (T,)), np.broadcast_to(model.meta["q"], (T - 1,))
        return kalman_log_lik(np.ones(T - 1), np.zeros(T - 1), q, r, y)
    if kind == "ssm_chain_linear":
        return kalman_log_lik(model.meta["a"], model.meta["b"], model.meta["q"], np.full(T, model.meta["r"]), y)
    A, Q, R = model.meta["A"], model.meta["Q"], model.meta["R"]
    return kalman_log_lik(np.broadcast_to(A, (T - 1, d, d)), np.zeros((T - 1, d)), np.broadcast_to(Q, (T - 1, d, d)), np.broadcast_to(R, (T, d, d)), y)


def one_variable_model(y: float, r: float) -> "cx.synth.Model":
    """x ~ N(0, 1) (an opaque prior), y = x + N(0, r) observed: log p(y) = log N(y; 0, 1 + r)"""
    return cx.synth.Model(edge_var=np.array([1, 1, 2], np.int64), edge_fac=np.array([3, 4, 4], np.int64), factor_ids=np.array([3, 4], np.int64),
                          factor_kind=np.array([L.FACTOR_OPAQUE, L.FACTOR_GAUSS_ADDITIVE], np.int32), factor_var=np.array([1.0, r]),
                          x_ids=np.array([1], np.int64), data_var=np.array([2], np.int64), data_fac=np.array([4], np.int64), data_y=np.array([y]),
                          prior_var=np.array([1], np.int64), prior_fac=np.array([3], np.int64), prior_mean=np.array([0.0]),
                          prior_variance=np.array([1.0]), meta={"kind": "one"})
