"""Shared by the per-component log-evidence tests: an independent statement of the connected components of a
synth.Model, the GModel of one component, a random relabelling of every id, and small model builders.  Pinned by
tests/test_components_checker.py; numpy only.

  labels(model)        the component of every variable (ascending id) by a numpy union-find over the connections: observed variables and
                       opaque factors are nodes like any other; components are numbered by their least variable id
  restrict(gm, k)      the evidence_support.GModel of component k alone (the sum of dense_log_z over the components is the whole model's)
  relabel(model, rng)  one random permutation over all ids in use (variables and factors stay distinct)
  join_scalar(models)  several dim 1 models as one graph, ids shifted past each other (synth.concat_models is for dim > 1)
  lone_variable(d)     one variable with an opaque prior and nothing else: log Z = 0
"""
from __future__ import annotations

import dataclasses

import numpy as np

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from tests import evidence_support as E


def _components(n_nodes, a, b):
    """union-find over nodes 0 .. n_nodes-1 joined by the pairs (a[i], b[i]); returns the least node of every node's set"""
    parent = np.arange(n_nodes, dtype=np.int64)

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for x, y in zip(np.asarray(a).tolist(), np.asarray(b).tolist()):
        rx, ry = find(x), find(y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)
    return np.array([find(i) for i in range(n_nodes)], dtype=np.int64)


def _number(root_of_var):
    """roots (least node of the set; a variable index) -> labels 0 .. C-1 in the order of the least variable"""
    roots, lab = np.unique(root_of_var, return_inverse=True)      # ascending root = ascending least variable index
    return lab.astype(np.int64), len(roots)


def labels(model):
    """(var_ids ascending, label per variable, C)"""
    var_ids = np.unique(model.edge_var)
    fac_ids = np.unique(np.concatenate([model.edge_fac, model.factor_ids]))
    nv = len(var_ids)
    root = _components(nv + len(fac_ids), np.searchsorted(var_ids, model.edge_var), nv + np.searchsorted(fac_ids, model.edge_fac))
    lab, C = _number(root[:nv])
    return var_ids, lab, C


def gm_labels(gm):
    """the same from a GModel (its rule factors join their variables; an opaque message joins nothing): (label per variable index, C)"""
    nv = len(gm.var_ids)
    a, b = [], []
    for k, g in gm.groups.items():
        for j in range(1, k):
            a.append(g["vars"][:, 0]); b.append(g["vars"][:, j])
    root = _components(nv, np.concatenate(a) if a else np.zeros(0, np.int64), np.concatenate(b) if b else np.zeros(0, np.int64))
    return _number(root)


def restrict(gm, k, lab=None):
    """the GModel of component k (numbered as labels() numbers them)"""
    if lab is None:
        lab, _ = gm_labels(gm)
    sel = np.flatnonzero(lab == k)
    new = -np.ones(len(gm.var_ids), np.int64)
    new[sel] = np.arange(len(sel))
    groups = {}
    for a, g in gm.groups.items():
        keep = lab[g["vars"][:, 0]] == k
        if keep.any():
            groups[a] = {"fid": g["fid"][keep], "vars": new[g["vars"][keep]], "C": g["C"][keep], "b": g["b"][keep], "Q": g["Q"][keep]}
    ok = lab[gm.opq_var] == k
    return E.GModel(d=gm.d, var_ids=gm.var_ids[sel], obs=gm.obs[sel], y=gm.y[sel], groups=groups, opq_var=new[gm.opq_var[ok]],
                    opq_fac=gm.opq_fac[ok], opq_eta=gm.opq_eta[ok], opq_lam=gm.opq_lam[ok])


def restrict_messages(gm, f2v, opq, k, lab=None):
    """the messages of evidence_support.device_messages / numpy_bp that belong to component k, in restrict(gm, k)'s order"""
    if lab is None:
        lab, _ = gm_labels(gm)
    out = {}
    for a, g in gm.groups.items():
        keep = lab[g["vars"][:, 0]] == k
        if keep.any():
            out[a] = (f2v[a][0][keep], f2v[a][1][keep])
    ok = lab[gm.opq_var] == k
    return out, (None if opq is None else (opq[0][ok], opq[1][ok]))


_ID_FIELDS = ("edge_var", "edge_fac", "factor_ids", "x_ids", "data_var", "data_fac", "prior_var", "prior_fac")
_ID_META = ("coef_var", "coef_fac", "all_coef_var", "all_coef_fac", "out_var", "kary_ids", "used")


def relabel(model, rng):
    """the same model under one random permutation of all ids in use; meta["relabel"] = (old ids ascending, their new ids)"""
    old = np.unique(np.concatenate([model.edge_var, model.edge_fac, model.factor_ids]))
    new = rng.permutation(old)
    f = lambda ids: new[np.searchsorted(old, np.asarray(ids, dtype=np.int64))]      # noqa: E731
    meta = dict(model.meta)
    for key in _ID_META:
        if key in meta:
            meta[key] = f(meta[key])
    meta["relabel"] = (old, new)
    return dataclasses.replace(model, meta=meta, **{k: f(getattr(model, k)) for k in _ID_FIELDS})


def new_id(model, old_id):
    old, new = model.meta["relabel"]
    return int(new[np.searchsorted(old, int(old_id))])


def join_scalar(models):
    """several dim 1 models without k-ary coefficients as one graph of disjoint components; meta["offsets"] lists the id shifts"""
    off, offs = 0, []
    for m in models:
        offs.append(off)
        off += int(max(m.edge_var.max(), m.edge_fac.max()))
    cat = lambda name, shift: np.concatenate([getattr(m, name) + (o if shift else 0) for m, o in zip(models, offs)])      # noqa: E731
    role = None
    if any(m.edge_role is not None for m in models):
        role = np.concatenate([m.edge_role if m.edge_role is not None else np.full(len(m.edge_var), L.ROLE_OUT, np.int32) for m in models])
    return cx.synth.Model(edge_var=cat("edge_var", True), edge_fac=cat("edge_fac", True), factor_ids=cat("factor_ids", True),
                          factor_kind=cat("factor_kind", False), factor_var=cat("factor_var", False), x_ids=cat("x_ids", True),
                          data_var=cat("data_var", True), data_fac=cat("data_fac", True), data_y=cat("data_y", False),
                          prior_var=cat("prior_var", True), prior_fac=cat("prior_fac", True), prior_mean=cat("prior_mean", False),
                          prior_variance=cat("prior_variance", False), edge_role=role, meta={"kind": "joined", "offsets": offs})


def lone_variable(d, seed=7):
    """(model, opaque) — variable 1 with the opaque factor 2 and nothing else; opaque = (var ids, fac ids, eta [1, d], Lambda [1, d, d]) for
    evidence_support.gmodel and for set_messages (FORM_NATURAL).  Its evidence is ∫ N(x; m, Λ⁻¹) dx = 1: log Z = 0"""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((d, d))
    lam = B @ B.T + d * np.eye(d)
    eta = 10.0 * rng.standard_normal(d)
    model = cx.synth.Model(edge_var=np.array([1], np.int64), edge_fac=np.array([2], np.int64), factor_ids=np.array([2], np.int64),
                           factor_kind=np.array([L.FACTOR_OPAQUE], np.int32), factor_var=np.zeros(1), x_ids=np.array([1], np.int64),
                           dim=d, edge_role=np.array([L.ROLE_OUT], np.int32), meta={"kind": "lone"})
    return model, (np.array([1], np.int64), np.array([2], np.int64), eta[None], lam[None])


def chain_parts(d, lengths, seed0=None):
    """lgssm_chain(T, d, seed=100 * d + T) for T in lengths, all under ONE explicit (A, Q, R) (concat_models keeps the first part's
    psets; at d = 3 the default A differs by seed)"""
    first = cx.synth.lgssm_chain(lengths[0], d=d, seed=100 * d + lengths[0])
    A, Q, R = first.meta["A"], first.meta["Q"], first.meta["R"]
    return [cx.synth.lgssm_chain(T, d=d, seed=(100 * d + T) if seed0 is None else seed0 + T, A=A, Q=Q, R=R) for T in lengths]
