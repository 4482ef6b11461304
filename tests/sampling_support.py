"""Shared by the posterior-sampling tests: independent statements of what cx_sample_posterior draws.

  philox4x32_10 / normals   the device generator restated in numpy (uint64 arithmetic, vectorised): Philox4x32-10 with counter
                            (j, v, s mod 2^32, s >> 32) and key (seed mod 2^32, seed >> 32), Box–Muller over two 53-bit uniforms
  tree_sampler              a forest sampler from the DENSE posterior: every component rooted at its lowest free variable, each factor's
                            other free variables drawn jointly given the one nearest the root (Gaussian conditioning of the dense
                            covariance; on a forest that is conditioning on every ancestor); returns the mean and the whitening matrix
                            B (z = B ε), so that B Bᵀ is the posterior covariance
  identity_noise            ε as identity columns: sample k of n_free * d samples is the unit vector of free component k
"""
from __future__ import annotations

import numpy as np

from tests import evidence_support as E
from tests import learning_support as LS

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr [n, 4], key [n, 2] or [2] (uint32 values) -> [n, 4] uint32 values (as uint64)"""
    ctr = np.asarray(ctr, np.uint64).reshape(-1, 4)
    c = [ctr[:, i].copy() for i in range(4)]
    key = np.broadcast_to(np.asarray(key, np.uint64), (len(c[0]), 2))
    k0, k1 = key[:, 0].copy(), key[:, 1].copy()
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(W0)) & MASK
            k1 = (k1 + np.uint64(W1)) & MASK
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & MASK, p1 & MASK, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & MASK, p0 & MASK]
    return np.stack(c, axis=1)


def normals(seed: int, samples, n_variables: int, d: int):
    """the device's standard normals [len(samples), n_variables, d] for the given global sample indices"""
    s = np.asarray(samples, np.uint64)
    S, nv, J = len(s), n_variables, (d + 1) // 2
    jj, vv, ss = np.meshgrid(np.arange(J, dtype=np.uint64), np.arange(nv, dtype=np.uint64), s, indexing="ij")
    ctr = np.stack([jj.ravel(), vv.ravel(), ss.ravel() & MASK, ss.ravel() >> np.uint64(32)], axis=1)
    seed = int(seed) & (2 ** 64 - 1)
    x = philox4x32_10(ctr, [seed & 0xFFFFFFFF, seed >> 32])
    w1 = ((x[:, 1] << np.uint64(32)) | x[:, 0]) >> np.uint64(11)
    w2 = ((x[:, 3] << np.uint64(32)) | x[:, 2]) >> np.uint64(11)
    u1 = (w1.astype(np.float64) + 0.5) * 2.0 ** -53
    u2 = (w2.astype(np.float64) + 0.5) * 2.0 ** -53
    r = np.sqrt(-2.0 * np.log(u1))
    n = np.stack([r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)], axis=-1).reshape(J, nv, S, 2)
    out = np.transpose(n, (2, 1, 0, 3)).reshape(S, nv, 2 * J)
    return np.ascontiguousarray(out[:, :, :d])


def identity_noise(gm: E.GModel):
    """noise [n_free * d, nv, d]: sample a * d + k is the unit vector of component k of the a-th free variable"""
    d = gm.d
    free = np.flatnonzero(~gm.obs)
    eps = np.zeros((len(free) * d, len(gm.var_ids), d))
    for a, v in enumerate(free):
        for k in range(d):
            eps[a * d + k, v, k] = 1.0
    return eps


def samples_to_b(x, mean, gm: E.GModel):
    """samples [n_free * d, nv, d] drawn with identity_noise and the posterior mean -> B [n_free d, n_free d] (column = sample)"""
    free = np.flatnonzero(~gm.obs)
    z = (x[:, free, :] - mean[free][None]).reshape(len(x), -1)
    return z.T


def tree_sampler(gm: E.GModel):
    """(mean [nv, d], B [n_free d, n_free d], Σ [n_free d, n_free d]) of the forest sampler from the dense posterior; raises on a cycle"""
    d = gm.d
    mean, Sig, fpos = LS.dense_posterior(gm)
    free = np.flatnonzero(~gm.obs)
    nf = len(free)
    facs = []                           # factors of two or more free variables, as lists of free indices
    for g in gm.groups.values():
        for vs in g["vars"]:
            fv = [int(fpos[v]) for v in vs if not gm.obs[v]]
            if len(fv) >= 2:
                facs.append(fv)
    by_var = [[] for _ in range(nf)]
    for i, fv in enumerate(facs):
        for a in fv:
            by_var[a].append(i)
    B = np.zeros((nf * d, nf * d))
    done = np.zeros(nf, bool)
    used = np.zeros(len(facs), bool)
    for r in range(nf):
        if done[r]:
            continue
        ri = np.arange(r * d, (r + 1) * d)
        B[np.ix_(ri, ri)] = np.linalg.cholesky(Sig[np.ix_(ri, ri)])
        done[r] = True
        queue = [r]
        while queue:
            p = queue.pop(0)
            for fi in by_var[p]:
                if used[fi]:
                    continue
                used[fi] = True
                ch = [a for a in facs[fi] if a != p]
                if any(done[a] for a in ch):
                    raise ValueError("the free variables form a cycle")
                ci = np.concatenate([np.arange(a * d, (a + 1) * d) for a in ch])
                pi = np.arange(p * d, (p + 1) * d)
                Spp, Scp, Scc = Sig[np.ix_(pi, pi)], Sig[np.ix_(ci, pi)], Sig[np.ix_(ci, ci)]
                G = Scp @ np.linalg.inv(Spp)
                B[ci] = G @ B[pi]                                   # z_C = G z_p + chol(Σ_C|p) ε_C
                B[np.ix_(ci, ci)] += np.linalg.cholesky(Scc - G @ Scp.T)
                for a in ch:
                    done[a] = True
                    queue.append(a)
    return mean, B, Sig
