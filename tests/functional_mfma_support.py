"""Shared by the cx_linear_moments_mfma tests (tests/test_gpu_linear_moments_mfma.py, pinned on the CPU by
tests/test_functional_mfma_checker.py): the recursion the device runs, restated in numpy.

  uncentred_moments   the UNCENTRED recursion on a rooted forest, from the factor→variable MESSAGES and the data: for a link factor with
                      child end C and parent end p,  M = C_C'Q⁻¹C_C + Σ (C's other messages) = U'U,  η_C = C_C'Q⁻¹b' + Σ their η,
                      x_C = G x_p + off + U⁻¹ ε_C  with  G = -M⁻¹ C_C'Q⁻¹C_p,  off = M⁻¹ η_C;  a root: Λ_r = Σ all its messages = U'U,
                      x_r = Λ_r⁻¹ η_r + U⁻¹ ε_r.  The mean is the ε = 0 walk root to leaves, the covariance  t ← u + Σ G_c' t_c  leaf to
                      root,  g = U⁻ᵀ t,  cov = Σ g gᵀ.  Rooted at the lowest free variable of every component — not where the device
                      roots it: at a fixed point the answer does not depend on the root.  Only factors with two free ends are links:
                      nothing else exists at the matrix-core dims.

The yardstick (dense_moments), the centred restatement (adjoint_moments over forest_bp), the functionals and the error measure are those
of tests/functional_support.py; the models and the two tolerances those of tests/sample_mfma_support.py.
"""
from __future__ import annotations

import numpy as np

from tests import evidence_support as E
from tests import functional_support as FS


def uncentred_links(gm: E.GModel, f2v):
    """(roots [(v, x_r⁰, L_r)], links [(p, c, G, off, L)] parents before children), L = U' the lower Cholesky factor of M"""
    d, nv = gm.d, len(gm.var_ids)
    tot_eta, tot_lam = np.zeros((nv, d)), np.zeros((nv, d, d))
    for k, g in gm.groups.items():
        e, l = f2v[k]
        for j in range(k):
            fr = ~gm.obs[g["vars"][:, j]]
            np.add.at(tot_eta, g["vars"][fr, j], e[fr, j])
            np.add.at(tot_lam, g["vars"][fr, j], l[fr, j])
    if gm.opq_var is not None and len(gm.opq_var):
        np.add.at(tot_eta, gm.opq_var, gm.opq_eta)
        np.add.at(tot_lam, gm.opq_var, gm.opq_lam)
    free = ~gm.obs
    facs, by_var = [], [[] for _ in range(nv)]
    for k, g in gm.groups.items():
        for fi, vs in enumerate(g["vars"]):
            fr = [j for j in range(k) if free[vs[j]]]
            if len(fr) > 2:
                raise ValueError("a factor with more than two free ends: no such link at the matrix-core dims")
            if len(fr) == 2:
                for j in fr:
                    by_var[vs[j]].append(len(facs))
                facs.append((k, fi, fr))
    roots, links = [], []
    done, used = np.zeros(nv, bool), np.zeros(len(facs), bool)
    for r in np.flatnonzero(free):
        if done[r]:
            continue
        done[r] = True
        roots.append((int(r), np.linalg.solve(tot_lam[r], tot_eta[r]), np.linalg.cholesky(tot_lam[r])))
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
                jp, jc = (fr[0], fr[1]) if V[fr[0]] == p else (fr[1], fr[0])
                c = int(V[jc])
                if done[c]:
                    raise ValueError("the free variables form a cycle")
                Qi = np.linalg.inv(Q)
                bp = b - sum(C[o] @ gm.y[V[o]] for o in range(k) if gm.obs[V[o]])
                M = C[jc].T @ Qi @ C[jc] + (tot_lam[c] - f2v[k][1][fi, jc])
                eta = C[jc].T @ Qi @ bp + (tot_eta[c] - f2v[k][0][fi, jc])
                M = 0.5 * (M + M.T)
                links.append((p, c, -np.linalg.solve(M, C[jc].T @ Qi @ C[jp]), np.linalg.solve(M, eta), np.linalg.cholesky(M)))
                done[c] = True
                queue.append(c)
    return roots, links


def uncentred_moments(gm: E.GModel, f2v, functionals):
    """(mean [K], cov [K, K]) by the recursion of §4s, in numpy, from the messages"""
    roots, links = uncentred_links(gm, f2v)
    W = FS.weight_matrix(gm, functionals)
    K = len(W)
    x = gm.y.copy()
    for r, x0, _L in roots:
        x[r] = x0
    for p, c, G, off, _L in links:
        x[c] = G @ x[p] + off
    mean = np.einsum("kvi,vi->k", W, x)
    t = np.where(gm.obs[None, :, None], 0.0, W).transpose(1, 2, 0).copy()            # [nv, d, K]
    cov = np.zeros((K, K))
    for p, c, G, _off, L in reversed(links):
        g = np.linalg.solve(L, t[c])                   # U⁻ᵀ t, U = L'
        cov += g.T @ g
        t[p] += G.T @ t[c]
    for r, _x0, L in roots:
        g = np.linalg.solve(L, t[r])
        cov += g.T @ g
    return mean, cov
