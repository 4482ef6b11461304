"""Shared by the linear-functional tests: two independent statements of what cx_linear_moments returns.

  dense_moments     W μ and W Σ Wᵀ from the dense float64 posterior (tests/learning_support.dense_posterior over evidence_support's
                    GModel): the yardstick
  adjoint_moments   the adjoint recursion restated in numpy on a rooted forest, from the factor→variable MESSAGES: the belief centres,
                    the links (G | off | L⁻ᵀ) of §4g from each factor belief's joint precision, the ε = 0 walk for the mean, and
                    u_parent += Gᵀ u_child, g = L⁻¹ u leaf-to-root for the covariance.  Rooted at the lowest free variable of every
                    component — not where the device roots it: at a fixed point the answer does not depend on the root
  rel_errors        the error measure of every comparison: covariances relative to sqrt(cov[k][k] cov[l][l]), means to the posterior
                    spread sqrt(cov[k][k])
  REL_TOL           the tolerance of the GPU tests: 10 x the largest error adjoint_moments itself shows against dense_moments on the
                    test models (tests/test_functional_checker.py measures it and pins this constant)

A functional is (variable ids, weights [n, d]); the same id may repeat, its weights add.
"""
from __future__ import annotations

import numpy as np

from tests import evidence_support as E
from tests import learning_support as LS

# measured by tests/test_functional_checker.py::test_restatement_error_sets_the_tolerance: the restatement's largest relative error
# against the dense solve over the test models is 2.7e-12 — the means of ssm_chain(4200), whose states reach 8.4e3 against a posterior
# spread of 0.7: one ulp of such a mean is already 2.7e-12 of the spread (ssm_chain(130): 1.3e-13; every covariance: under 2e-15).
# 10 x that, rounded up.  One constant for every case: the long chain raises it for all
REL_TOL = 3e-11


def as_csr(functionals, d):
    off = np.concatenate([[0], np.cumsum([len(np.atleast_1d(i)) for i, _ in functionals])]).astype(np.int64)
    ids = np.concatenate([np.atleast_1d(i) for i, _ in functionals]).astype(np.int64) if functionals else np.zeros(0, np.int64)
    w = np.concatenate([np.asarray(x, float).reshape(-1, d) for _, x in functionals]) if functionals else np.zeros((0, d))
    return off, ids, w


def weight_matrix(gm: E.GModel, functionals):
    """W [K, nv, d] over every variable of the model (ascending id)"""
    d = gm.d
    W = np.zeros((len(functionals), len(gm.var_ids), d))
    for k, (ids, w) in enumerate(functionals):
        idx = np.searchsorted(gm.var_ids, np.atleast_1d(ids))
        np.add.at(W[k], idx, np.asarray(w, float).reshape(-1, d))
    return W


def dense_moments(gm: E.GModel, functionals, dense=None):
    """(mean [K], cov [K, K]) from the dense posterior; dense: a cached LS.dense_posterior(gm)"""
    mean, Sig, _ = LS.dense_posterior(gm) if dense is None else dense
    W = weight_matrix(gm, functionals)
    free = np.flatnonzero(~gm.obs)
    Wf = W[:, free, :].reshape(len(W), -1)
    return np.einsum("kvi,vi->k", W, mean), Wf @ Sig @ Wf.T


def rel_errors(mean, cov, ref_mean, ref_cov):
    """(largest mean error / posterior spread, largest covariance error / sqrt(cov_kk cov_ll)); a functional of zero spread (observed
    variables only) is measured against max(|mean|, 1)"""
    sd = np.sqrt(np.maximum(np.diag(ref_cov), 0.0))
    scale_m = np.where(sd > 0, sd, np.maximum(np.abs(ref_mean), 1.0))
    scale_c = np.outer(sd, sd)
    scale_c = np.where(scale_c > 0, scale_c, 1.0)
    em = float(np.max(np.abs(mean - ref_mean) / scale_m)) if len(ref_mean) else 0.0
    ec = float(np.max(np.abs(cov - ref_cov) / scale_c)) if cov is not None and ref_cov.size else 0.0
    return em, ec


def _rooted_links(gm: E.GModel, f2v):
    """the links of §4g from the messages, the forest rooted at the lowest free variable of every component.  Returns (mu [nv, d], roots
    [(v, L_r)], links [(parent v, children [v], G [md, d], off [md], L [md, md])] parents before children)"""
    d, nv = gm.d, len(gm.var_ids)
    M_eta, M_lam = np.zeros((nv, d)), np.zeros((nv, d, d))
    for k, g in gm.groups.items():
        e, l = f2v[k]
        for j in range(k):
            fr = ~gm.obs[g["vars"][:, j]]
            np.add.at(M_eta, g["vars"][fr, j], e[fr, j])
            np.add.at(M_lam, g["vars"][fr, j], l[fr, j])
    np.add.at(M_eta, gm.opq_var, gm.opq_eta)
    np.add.at(M_lam, gm.opq_var, gm.opq_lam)
    free = ~gm.obs
    mu = np.zeros((nv, d))
    mu[free] = np.linalg.solve(M_lam[free], M_eta[free][..., None])[..., 0]
    facs = []            # (group, row, free entries)
    by_var = [[] for _ in range(nv)]
    for k, g in gm.groups.items():
        for fi, vs in enumerate(g["vars"]):
            fr = [j for j in range(k) if free[vs[j]]]
            if len(fr) >= 2:
                for j in fr:
                    by_var[vs[j]].append(len(facs))
                facs.append((k, fi, fr))
    roots, links = [], []
    done, used = np.zeros(nv, bool), np.zeros(len(facs), bool)
    for r in np.flatnonzero(free):
        if done[r]:
            continue
        done[r] = True
        roots.append((int(r), np.linalg.cholesky(M_lam[r])))
        queue = [int(r)]
        while queue:
            p = queue.pop(0)
            for a in by_var[p]:
                if used[a]:
                    continue
                used[a] = True
                k, fi, fr = facs[a]
                g = gm.groups[k]
                V, C, b, Q = g["vars"][fi], g["C"][fi], g["b"][fi], g["Q"][fi]
                e, l = f2v[k][0][fi], f2v[k][1][fi]
                Qi = np.linalg.inv(Q)
                x = np.where(free[V][:, None], mu[V], gm.y[V])
                bp = b - np.einsum("kij,kj->i", C, x)
                # the factor belief over its free entries, centred: J = C'Q⁻¹C + the leave-one-out precisions, h likewise
                order = [j for j in fr if V[j] == p] + [j for j in fr if V[j] != p]
                n = len(order)
                J, h = np.zeros((n * d, n * d)), np.zeros(n * d)
                for a_, ja in enumerate(order):
                    lt = M_lam[V[ja]] - l[ja]
                    et = -(e[ja] - l[ja] @ mu[V[ja]])
                    h[a_ * d:(a_ + 1) * d] = C[ja].T @ Qi @ bp + et
                    for c_, jc in enumerate(order):
                        J[a_ * d:(a_ + 1) * d, c_ * d:(c_ + 1) * d] = C[ja].T @ Qi @ C[jc] + (lt if a_ == c_ else 0.0)
                Jcc, Jcp = J[d:, d:], J[d:, :d]
                Lc = np.linalg.cholesky(Jcc)
                ch = [int(V[j]) for j in order[1:]]
                if any(done[c] for c in ch):
                    raise ValueError("the free variables form a cycle")
                links.append((p, ch, -np.linalg.solve(Jcc, Jcp), np.linalg.solve(Jcc, h[d:]), Lc))
                for c in ch:
                    done[c] = True
                    queue.append(c)
    return mu, roots, links


def adjoint_moments(gm: E.GModel, f2v, functionals):
    """(mean [K], cov [K, K]) by the recursion of §4i, in numpy, from the messages"""
    d, nv = gm.d, len(gm.var_ids)
    mu, roots, links = _rooted_links(gm, f2v)
    W = weight_matrix(gm, functionals)
    K = len(W)
    # the mean: the ε = 0 walk, root to leaves
    z = np.zeros((nv, d))
    for p, ch, G, off, _L in links:
        z[ch] = (G @ z[p] + off).reshape(len(ch), d)
    x = np.where(gm.obs[:, None], gm.y, mu + z)
    mean = np.einsum("kvi,vi->k", W, x)
    # the covariance: u leaf-to-root, the noise coordinates g = L⁻¹ u of every link's child block and L_r⁻¹ u_r of every root
    u = np.where(gm.obs[None, :, None], 0.0, W).transpose(1, 2, 0).copy()           # [nv, d, K]
    cov = np.zeros((K, K))
    for p, ch, G, _off, L in reversed(links):
        uc = u[ch].reshape(len(ch) * d, K)
        g = np.linalg.solve(L, uc)                    # (L⁻ᵀ)ᵀ u: a child's ε reaches its earlier siblings too
        cov += g.T @ g
        u[p] += G.T @ uc
    for r, Lr in roots:
        g = np.linalg.solve(Lr, u[r])
        cov += g.T @ g
    return mean, cov


def forest_bp(gm: E.GModel):
    """the fixed point of Gaussian BP on a forest in two passes (leaves to roots, roots to leaves) over the rooted order of _rooted_links:
    every message once, O(n) — E.numpy_bp floods and needs as many rounds as the forest is deep.  The same update as numpy_bp's; returns
    its f2v dict (tests/test_functional_checker.py pins the two against each other)."""
    d, nv = gm.d, len(gm.var_ids)
    f2v = {k: (np.full((len(g["fid"]), k, d), np.nan), np.full((len(g["fid"]), k, d, d), np.nan)) for k, g in gm.groups.items()}
    edges = [[] for _ in range(nv)]                     # per variable: (group, row, entry) of every rule edge
    for k, g in gm.groups.items():
        for fi, vs in enumerate(g["vars"]):
            for j in range(k):
                edges[vs[j]].append((k, fi, j))
    opq_eta, opq_lam = np.zeros((nv, d)), np.zeros((nv, d, d))
    np.add.at(opq_eta, gm.opq_var, gm.opq_eta)
    np.add.at(opq_lam, gm.opq_var, gm.opq_lam)

    def cavity(v, skip):
        e, l = opq_eta[v].copy(), opq_lam[v].copy()
        for (k, fi, j) in edges[v]:
            if (k, fi, j) != skip:
                e += f2v[k][0][fi, j]
                l += f2v[k][1][fi, j]
        return e, l

    def send(k, fi, j):
        g = gm.groups[k]
        V, C, b, Q = g["vars"][fi], g["C"][fi], g["b"][fi], g["Q"][fi]
        Qi = np.linalg.inv(Q)
        others = [o for o in range(k) if o != j and not gm.obs[V[o]]]
        bp = b - sum(C[o] @ gm.y[V[o]] for o in range(k) if gm.obs[V[o]])
        Jjj, hj = C[j].T @ Qi @ C[j], C[j].T @ Qi @ bp
        if others:
            no = len(others)
            Joo, ho, Jjo = np.zeros((no * d, no * d)), np.zeros(no * d), np.zeros((d, no * d))
            for a, oa in enumerate(others):
                ve, vl = cavity(V[oa], (k, fi, oa))
                ho[a * d:(a + 1) * d] = C[oa].T @ Qi @ bp + ve
                Jjo[:, a * d:(a + 1) * d] = C[j].T @ Qi @ C[oa]
                for c_, oc in enumerate(others):
                    Joo[a * d:(a + 1) * d, c_ * d:(c_ + 1) * d] = C[oa].T @ Qi @ C[oc] + (vl if a == c_ else 0.0)
            Jjj = Jjj - Jjo @ np.linalg.solve(Joo, Jjo.T)
            hj = hj - Jjo @ np.linalg.solve(Joo, ho)
        f2v[k][0][fi, j], f2v[k][1][fi, j] = hj, 0.5 * (Jjj + Jjj.T)

    # the rooted order (the structure alone: _rooted_links' traversal without its numbers)
    free = ~gm.obs
    facs, by_var = [], [[] for _ in range(nv)]
    for k, g in gm.groups.items():
        for fi, vs in enumerate(g["vars"]):
            fr = [j for j in range(k) if free[vs[j]]]
            if len(fr) == 1:
                send(k, fi, fr[0])                      # a factor of one free variable: its message needs no other
            elif len(fr) >= 2:
                for j in fr:
                    by_var[vs[j]].append(len(facs))
                facs.append((k, fi, fr))
    order, done, used = [], np.zeros(nv, bool), np.zeros(len(facs), bool)
    for r in np.flatnonzero(free):
        if done[r]:
            continue
        done[r] = True
        queue = [int(r)]
        while queue:
            p = queue.pop(0)
            for a in by_var[p]:
                if used[a]:
                    continue
                used[a] = True
                k, fi, fr = facs[a]
                V = gm.groups[k]["vars"][fi]
                jp = [j for j in fr if V[j] == p][0]
                order.append((k, fi, jp, [j for j in fr if j != jp]))
                for j in fr:
                    if j != jp:
                        if done[V[j]]:
                            raise ValueError("the free variables form a cycle")
                        done[V[j]] = True
                        queue.append(int(V[j]))
    for k, fi, jp, _ch in reversed(order):
        send(k, fi, jp)
    for k, fi, _jp, ch in order:
        for j in ch:
            send(k, fi, j)
    return f2v


# ---- the test models and their functionals ------------------------------------------------------------------------------------------
def standard_functionals(gm: E.GModel, seed=0, max_units=140):
    """the functionals every model is asked: unit functionals (every free variable and component, or a subset that keeps the tile
    boundaries 64 k and 4096 k of a long chain), contrasts of near and far pairs, a window mean, random dense weights, a variable named
    twice, the siblings of a factor of three or more free variables, and one functional with and without a weight on an observed
    variable.  Returns (functionals, names)"""
    rng = np.random.default_rng(seed)
    d = gm.d
    free = gm.var_ids[~gm.obs]
    n = len(free)
    eye = np.eye(d)
    if n * d <= max_units:
        pick = np.arange(n)
    else:
        pick = np.unique(np.concatenate([np.arange(0, n, max(n // 24, 1)), [62, 63, 64, 65, 127, 128, 4094, 4095, 4096, 4097, n - 1]]))
        pick = pick[pick < n]
    fs, names = [], []
    for a in pick:
        for i in range(d):
            fs.append(([free[a]], eye[i:i + 1])); names.append(f"unit {free[a]}.{i}")
    one = np.ones((1, d))
    for a, b in [(3, 40), (60, 70), (0, n - 1), (n // 2, n // 2 + 1)]:
        a, b = a % n, b % n
        if a != b:
            fs.append(([free[a], free[b]], np.concatenate([one, -one]))); names.append(f"contrast {free[a]} {free[b]}")
    w = min(n, 50)
    s0 = min(40, n - w)
    fs.append((free[s0:s0 + w], np.full((w, d), 1.0 / w))); names.append("window mean")
    fs.append((free, rng.standard_normal((n, d)))); names.append("dense")
    fs.append(([free[1 % n], free[n - 1], free[1 % n]], rng.standard_normal((3, d)))); names.append("repeat")
    for k, g in gm.groups.items():
        if k < 3:
            continue
        for vs in g["vars"]:
            fv = [v for v in vs if not gm.obs[v]]
            if len(fv) >= 3:
                fs.append((gm.var_ids[fv], rng.standard_normal((len(fv), d)))); names.append(f"siblings {k}")
                fs.append((gm.var_ids[fv[-2:]], np.concatenate([one, -one]))); names.append(f"sibling contrast {k}")
                break
    if gm.obs.any():
        o = gm.var_ids[gm.obs][len(gm.var_ids[gm.obs]) // 2]
        base = ([free[0], free[n // 3]], rng.standard_normal((2, d)))
        fs.append(base); names.append("without observed")
        fs.append((list(base[0]) + [o], np.concatenate([base[1], 2.0 * one]))); names.append("with observed")
    return fs, names


def kary_case(d, seed):
    """the k-ary tree of tests/test_gpu_kary_mv at dim d: (model, gm, loader(schedule) -> DeviceGraph)"""
    from tests.test_gpu_kary_mv import _kary_tree, _load
    model, prior, facs, fid, sets, _m, _c = _kary_tree(12, d, seed, k_choices=(2, 3, 5))
    n = len(model.x_ids)
    edge_sets = {(int(model.x_ids[i]), int(f)): s for f, (_o, ins, ss, _q) in zip(fid, facs) for i, s in zip(ins, ss)}
    gm = E.gmodel(model, edge_sets=edge_sets, opaque=(model.x_ids, model.x_ids + n, prior[0], prior[1]))
    return model, gm, lambda schedule: _load(model, prior, facs, fid, sets, schedule)


def cases(long=False):
    """name -> (make() -> (model, gm, loader or None), chain?) for every model of the issue; long: ssm_chain(4200) too (the GPU file
    gives it a test of its own)"""
    import cortex.jl_amd as cx

    def plain(make):
        def f():
            m = make()
            return m, E.gmodel(m), None
        return f
    out = {"ssm_chain 130": (plain(lambda: cx.synth.ssm_chain(130, seed=401)), True)}
    for d in (2, 3, 4):
        out[f"lgssm_chain 70 d={d}"] = (plain(lambda d=d: cx.synth.lgssm_chain(70, d=d, seed=410 + d)), True)
        out[f"lgssm_comb 15 d={d}"] = (plain(lambda d=d: cx.synth.lgssm_comb(15, d=d, teeth=1, seed=420 + d)), False)
    out["tree_model 60"] = (plain(lambda: cx.synth.tree_model(60, seed=430, k_choices=(1, 2, 3, 4, 5, 6), observe=0.2)), False)
    for d in (2, 3):
        out[f"kary tree d={d}"] = ((lambda d=d: kary_case(d, 440 + d)), False)
    if long:
        out["ssm_chain 4200"] = (plain(lambda: cx.synth.ssm_chain(4200, seed=402)), True)
    return out
