"""Shared by the cx_factor_disturbances_mfma tests (tests/test_gpu_factor_disturbances_mfma.py, pinned on the CPU by
tests/test_disturbances_mfma_checker.py): what the posterior of every factor's own noise is, stated twice.  Every two-variable
CX_FACTOR_GAUSS_LINEAR factor is x_out = A x_in + b + w, w ~ N(0, Q), and r = x_out - A x_in - b is w.

  dense(model, b, opaque)   per factor (E[r], Cov(r), t, q) from the joint posterior of offsets_support.joint_solve_offsets:
                            r = c + Σ_a M_a x_a over the factor's non-observed ends (M_out = I, M_in = -A, c = -b + Σ_observed M y), so
                            E[r] = c + Σ M_a μ_a and Cov(r) = Σ_ab M_a S_ab M_b'; t = tr(Q⁻¹ Cov(r)) + q, q = E[r]'Q⁻¹E[r].  Exact on
                            every graph; an opaque prior (evidence_support's 4-tuple) is added to the joint precision
  restated(gm, f2v, opq)    learn_mfma_support.restate(..., stats=True) reshaped to the same rows: the kernel's algebra on GIVEN
                            messages (the device's own, on a loop).  restate asserts zero offsets: the offsets tests use dense
  scores(mean, cov, Q)      (t, q, Σ|terms|) from rows in numpy: the sums the kernel forms, with the size of their terms for the
                            rounding bound of a d²-term sum
  latent_dims(model)        d x the number of non-observed variables: Σ_f (t_f - q_f) on a forest whose every message comes from
                            the model (no opaque one), with and without offsets — the trace identity of DESIGN.md §4v
Both return {"factor_ids" ascending, "mean" [n, d], "cov" [n, d, d], "expected_mahalanobis" [n], "mahalanobis" [n]}: the keys and the
default order of DeviceGraph.factor_disturbances_mfma.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from cortex.jl_amd import _lib as L
from tests import learn_mfma_support as M
from tests import offsets_support as O


def _rows(fids, mean, cov, Qs):
    order = np.argsort(np.asarray(fids))
    mean, cov, Qs = np.asarray(mean)[order], np.asarray(cov)[order], np.asarray(Qs)[order]
    Qi = np.linalg.inv(Qs)
    q = np.einsum("ni,nij,nj->n", mean, Qi, mean)
    return {"factor_ids": np.asarray(fids, np.int64)[order], "mean": mean, "cov": cov,
            "expected_mahalanobis": np.einsum("nij,nij->n", Qi, cov) + q, "mahalanobis": q}


def _without_opaque(model):
    keep_f = np.asarray(model.factor_kind) != L.FACTOR_OPAQUE
    gone = set(np.asarray(model.factor_ids)[~keep_f].tolist())
    keep_e = np.array([f not in gone for f in np.asarray(model.edge_fac).tolist()])
    return dataclasses.replace(model, edge_var=np.asarray(model.edge_var)[keep_e], edge_fac=np.asarray(model.edge_fac)[keep_e],
                               edge_role=np.asarray(model.edge_role)[keep_e], factor_ids=np.asarray(model.factor_ids)[keep_f],
                               factor_kind=np.asarray(model.factor_kind)[keep_f], factor_var=np.asarray(model.factor_var)[keep_f])


def dense(model, b=None, opaque=None):
    d = model.dim
    b = {} if b is None else b
    base = _without_opaque(model) if opaque is not None else model
    mean, S, pos, _ = O.joint_solve_offsets(base, b)
    if opaque is not None:      # the prior's (η, Λ) into the joint precision: J = S⁻¹, h = J μ
        J = np.linalg.inv(S)
        h = J @ mean
        for v, eta, lam in zip(np.asarray(opaque[0]).tolist(), opaque[2], opaque[3]):
            a = pos[int(v)]
            J[a * d:(a + 1) * d, a * d:(a + 1) * d] += lam
            h[a * d:(a + 1) * d] += eta
        S = np.linalg.inv(0.5 * (J + J.T))
        S = 0.5 * (S + S.T)
        mean = S @ h
    data = {int(v): np.asarray(y, float) for v, y in zip(base.data_var, np.asarray(base.data_y).reshape(len(base.data_var), d))}
    ends = O._ends(base)
    fids = O.linear_factors(base)
    sets = dict(zip(np.asarray(base.factor_ids).tolist(), np.asarray(base.factor_var).astype(int).tolist()))
    means, covs, Qs = [], [], []
    for f in fids.tolist():
        A, Q = (np.asarray(x, float) for x in base.psets[sets[f]])
        c = -np.asarray(b.get(f, np.zeros(d)), float)
        terms = []
        for v, Mv in ((ends[f][L.ROLE_OUT], np.eye(d)), (ends[f][L.ROLE_IN], -A)):
            if v in data:
                c = c + Mv @ data[v]
            else:
                terms.append((pos[v], Mv))
        er, cr = c.copy(), np.zeros((d, d))
        for a, Ma in terms:
            er = er + Ma @ mean[a * d:(a + 1) * d]
            for a2, Mb in terms:
                cr = cr + Ma @ S[a * d:(a + 1) * d, a2 * d:(a2 + 1) * d] @ Mb.T
        means.append(er); covs.append(0.5 * (cr + cr.T)); Qs.append(Q)
    return _rows(fids, means, covs, Qs)


def restated(gm, f2v, opq_msgs=None):
    rows = M.restate(gm, f2v, opq_msgs, stats=True)
    assert all(r[5] == M.OK for r in rows)
    g = gm.groups[2]
    return _rows(g["fid"], [r[0] for r in rows], [r[2] for r in rows], g["Q"])


def scores(mean, cov, Q):
    """(t [n], q [n], Σ|terms| [n]) of rows; Q: [d, d] or [n, d, d]"""
    mean, cov = np.asarray(mean, float), np.asarray(cov, float)
    Qi = np.linalg.inv(np.broadcast_to(np.asarray(Q, float), cov.shape))
    mm = mean[:, :, None] * mean[:, None, :]
    q = np.sum(Qi * mm, axis=(1, 2))
    return np.sum(Qi * cov, axis=(1, 2)) + q, q, np.sum(np.abs(Qi * cov), axis=(1, 2)) + np.sum(np.abs(Qi * mm), axis=(1, 2))


def factor_Q(model, fids):
    """[n, d, d]: the Q of every factor of fids"""
    sets = dict(zip(np.asarray(model.factor_ids).tolist(), np.asarray(model.factor_var).astype(int).tolist()))
    return np.stack([np.asarray(model.psets[sets[int(f)]][1], float) for f in fids])


def latent_dims(model):
    return model.dim * len(set(int(v) for v in model.edge_var) - set(int(v) for v in model.data_var))
