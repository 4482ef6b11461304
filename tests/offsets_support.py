"""Shared by the factor-offset tests (cx_set_factor_offsets, dim 2..4): models of tests/anisotropic.py whose CX_FACTOR_GAUSS_LINEAR factors
are x_out = A x_in + b + N(0, Q) with a b of their own, and independent statements of what such a model's posterior is.

  with_offsets(model, seed, scale)   b ~ scale N(0, I) for every rule factor, transitions and observation factors alike: {factor id: b}
  consistent_offsets(model, seed)    a shift s per variable and b_a = s_out - A s_in: the model is then the zero-offset model in
                                     x' = x - s (works on loopy graphs too); returns (b, s)
  joint_solve_offsets(model, b)      AN.joint_solve with the residual x_out - A x_in - b: mean, covariance, positions, log Z
  gmodel_offsets(model, b)           evidence_support.gmodel with the pairwise group's b filled in: bethe_log_z, dense_log_z, numpy_bp and the
                                     readers' dense references then see the offsets
  shifted_twin(model, b, s)          the zero-offset model with data y - s at the observed variables, and the map of a natural-form
                                     message of the offset model onto the twin's, eta' = eta - Lambda s
"""
from __future__ import annotations

import dataclasses

import numpy as np

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from tests import anisotropic as AN
from tests import evidence_support as E


def _ends(model):
    ends = {}
    for v, f, r in zip(model.edge_var.tolist(), model.edge_fac.tolist(), model.edge_role.tolist()):
        ends.setdefault(f, {})[r] = v
    return ends


def linear_factors(model):
    """ids of the two-variable CX_FACTOR_GAUSS_LINEAR factors, ascending"""
    return np.sort(np.asarray(model.factor_ids)[np.asarray(model.factor_kind) == L.FACTOR_GAUSS_LINEAR])


def with_offsets(model, seed, scale=1.0):
    rng = np.random.default_rng([seed, model.dim, 91])
    return {int(f): scale * rng.standard_normal(model.dim) for f in linear_factors(model)}


def consistent_offsets(model, seed):
    rng = np.random.default_rng([seed, model.dim, 92])
    d = model.dim
    s = {int(v): rng.standard_normal(d) for v in np.unique(model.edge_var)}
    ends = _ends(model)
    sets = dict(zip(model.factor_ids.tolist(), np.asarray(model.factor_var).astype(int).tolist()))
    b = {}
    for f in linear_factors(model).tolist():
        A = np.asarray(model.psets[sets[f]][0])
        b[f] = s[ends[f][L.ROLE_OUT]] - A @ s[ends[f][L.ROLE_IN]]
    return b, s


def arrays(b):
    """({id: b}) -> (ids [n], b [n, d]) as DeviceGraph.set_factor_offsets takes them"""
    ids = np.array(sorted(b), np.int64)
    return ids, np.stack([b[int(f)] for f in ids])


def joint_solve_offsets(model, b):
    """AN.joint_solve's assembly with c += -b: every factor is x_out - A x_in - b ~ N(0, Q), an observed end replaced by its datum"""
    d = model.dim
    data = {int(v): np.asarray(y, float) for v, y in zip(model.data_var, np.asarray(model.data_y).reshape(len(model.data_var), d))}
    latent = sorted(set(int(v) for v in model.edge_var) - set(data))
    pos = {v: a for a, v in enumerate(latent)}
    n = len(latent) * d
    J, h, const = np.zeros((n, n)), np.zeros(n), 0.0
    ends = _ends(model)
    per_set = {k: (np.linalg.inv(Q), np.linalg.slogdet(2 * np.pi * np.asarray(Q))[1]) for k, (_, Q) in model.psets.items()}
    for f, s in zip(model.factor_ids.tolist(), np.asarray(model.factor_var).astype(int).tolist()):
        A = model.psets[s][0]
        Qi, ldq = per_set[s]
        terms, c = [], -np.asarray(b.get(f, np.zeros(d)), float)
        for v, M in ((ends[f][L.ROLE_OUT], np.eye(d)), (ends[f][L.ROLE_IN], -np.asarray(A))):
            if v in data:
                c = c + M @ data[v]
            else:
                terms.append((pos[v], M))
        const += -0.5 * c @ Qi @ c - 0.5 * ldq
        for a, Ma in terms:
            h[a * d:(a + 1) * d] -= Ma.T @ Qi @ c
            for a2, Mb in terms:
                J[a * d:(a + 1) * d, a2 * d:(a2 + 1) * d] += Ma.T @ Qi @ Mb
    J = 0.5 * (J + J.T)
    Lj = np.linalg.cholesky(J)                           # the posterior is proper, or this raises
    S = np.linalg.inv(J)
    S = 0.5 * (S + S.T)
    mean = S @ h
    log_z = const + 0.5 * h @ mean - np.log(np.diag(Lj)).sum() + 0.5 * n * np.log(2 * np.pi)
    return mean, S, pos, float(log_z)


def dense_posterior_offsets(model, b):
    """(mean [n, d], covariance blocks [n, d, d]) of model.x_ids from joint_solve_offsets"""
    d = model.dim
    mean, S, pos, _ = joint_solve_offsets(model, b)
    p = [pos[int(x)] for x in model.x_ids]
    return np.stack([mean[a * d:(a + 1) * d] for a in p]), np.stack([S[a * d:(a + 1) * d, a * d:(a + 1) * d] for a in p])


def gmodel_offsets(model, b):
    gm = E.gmodel(model)
    g = gm.groups[2]
    g["b"] = np.stack([np.asarray(b.get(int(f), np.zeros(model.dim)), float) for f in g["fid"]])
    return gm


def shifted_twin(model, b, s):
    """(twin model, to_twin): the twin is `model` without offsets and with data y - s; to_twin(variable ids, natural rows [n, d + d d]) maps
    messages into those variables (or their beliefs) of the offset model onto the twin's: Lambda' = Lambda, eta' = eta - Lambda s"""
    d = model.dim
    y = np.asarray(model.data_y, float).reshape(len(model.data_var), d)
    twin = dataclasses.replace(model, data_y=y - np.stack([s[int(v)] for v in model.data_var]))

    def to_twin(var_ids, nat):
        nat = np.array(nat, float)
        sv = np.stack([s[int(v)] for v in var_ids])
        lam = nat[:, d:].reshape(len(nat), d, d)
        ok = ~np.isnan(lam).any(axis=(1, 2))
        nat[ok, :d] -= np.einsum("nij,nj->ni", lam[ok], sv[ok])
        return nat
    return twin, to_twin



# ---- shared by tests/test_gpu_factor_offsets.py (dim 2 .. 4) and tests/test_gpu_factor_offsets_mfma.py (dim 5 .. 64) ------------------------
def latent_edges(model):
    keep = np.isin(model.edge_var, model.x_ids)
    return model.edge_var[keep], model.edge_fac[keep]


def messages(dev, model):
    ev, ef = latent_edges(model)
    return dev.get_messages(ev, ef, L.TO_VARIABLE, L.FORM_NATURAL)


_REF = {}


def ref(key, make):
    """a reference computed once per key and left unchanged (one cache for both files: their keys carry the dim or differ in form)"""
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def tree_case(name, make):
    def build():
        model = make()
        b1, b2 = with_offsets(model, 5), with_offsets(model, 6, scale=2.0)
        return model, b1, dense_posterior_offsets(model, b1), b2, dense_posterior_offsets(model, b2)
    return ref(("tree", name), build)


def hub_model(d, seed=9):
    """u (observed) -> x -> y (observed), x -> z (a free leaf): every direction of a message through a factor, from either kind of sender"""
    A, Q, R, H = AN.general_sets(d, seed)
    rng = np.random.default_rng([seed, d, 93])
    IN, OUT = L.ROLE_IN, L.ROLE_OUT
    return cx.synth.Model(edge_var=np.array([1, 2, 2, 3, 2, 4], np.int64), edge_fac=np.array([10, 10, 11, 11, 12, 12], np.int64),
                          edge_role=np.array([IN, OUT, IN, OUT, IN, OUT], np.int32), factor_ids=np.array([10, 11, 12], np.int64),
                          factor_kind=np.full(3, L.FACTOR_GAUSS_LINEAR, np.int32), factor_var=np.array([0.0, 1.0, 0.0]), x_ids=np.array([2, 4], np.int64),
                          data_var=np.array([1, 3], np.int64), data_fac=np.array([10, 11], np.int64), data_y=rng.standard_normal((2, d)), dim=d,
                          psets={0: (A, Q), 1: (H, R)}, meta={"kind": "hub"})
