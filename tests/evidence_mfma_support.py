"""Shared by the cx_log_evidence_mfma tests (tests/test_gpu_evidence_mfma.py, pinned on the CPU by tests/test_evidence_mfma_checker.py):
the models that are not in synth.py as they stand.

  ring(d)            synth.lgssm_chain(5, d) closed by one more transition factor of set 0 from x_T (IN) to x_1 (OUT): one loop, where the
                     stored messages give the Bethe estimate and not the exact value
  forecast_chain(d)  a chain with a datum at every second state and three states behind the last datum (tests/missing_data.py: thin, tail);
                     the last state is a latent leaf, its variable→factor message the flat one (missing_data.load sets it)
"""
from __future__ import annotations

import dataclasses

import numpy as np

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from tests import missing_data as MD

RING_T = 5
RING_DIMS = (5, 16, 64)
RING_SWEEPS = 150
FORECAST_DIMS = (16, 8)


def ring(d, seed=None):
    m = cx.synth.lgssm_chain(RING_T, d=d, seed=700 + d if seed is None else seed)
    f = int(max(np.max(m.edge_var), np.max(m.edge_fac))) + 1
    return dataclasses.replace(
        m, edge_var=np.concatenate([m.edge_var, [m.x_ids[-1], m.x_ids[0]]]).astype(np.int64), edge_fac=np.concatenate([m.edge_fac, [f, f]]).astype(np.int64),
        edge_role=np.concatenate([m.edge_role, [L.ROLE_IN, L.ROLE_OUT]]).astype(np.int32), factor_ids=np.concatenate([m.factor_ids, [f]]).astype(np.int64),
        factor_kind=np.concatenate([m.factor_kind, [L.FACTOR_GAUSS_LINEAR]]).astype(np.int32), factor_var=np.concatenate([m.factor_var, [0.0]]),
        meta={**m.meta, "kind": "lgssm_ring"})


def clamped_middle(d, T=5, i=2):
    """lgssm_chain(T, d) with state i observed as well (its datum on every one of its edges): its likelihood factor has both ends observed,
    the transition into it an observed OUT end, the transition out of it an observed IN end"""
    m = cx.synth.lgssm_chain(T, d=d, seed=900 + d)
    x = m.x_ids[i]
    facs = np.asarray(m.edge_fac)[np.asarray(m.edge_var) == x]
    value = np.random.default_rng(901 + d).standard_normal(d)
    return dataclasses.replace(m, data_var=np.concatenate([m.data_var, np.full(len(facs), x)]), data_fac=np.concatenate([m.data_fac, facs]),
                               data_y=np.vstack([m.data_y, np.tile(value, (len(facs), 1))]), meta={**m.meta, "clamped_state": i})


OPAQUE_DIMS = (16, 8)      # native, and embedded in the 16-tile


def _with_opaque(model, var_ids):
    """`model` with one CX_FACTOR_OPAQUE factor on each of var_ids (a caller-set factor→variable message); returns (model, factor ids)"""
    top = int(max(np.max(model.edge_var), np.max(model.edge_fac)))
    f = top + 1 + np.arange(len(var_ids), dtype=np.int64)
    return dataclasses.replace(
        model, edge_var=np.concatenate([model.edge_var, var_ids]).astype(np.int64), edge_fac=np.concatenate([model.edge_fac, f]).astype(np.int64),
        edge_role=np.concatenate([model.edge_role, np.full(len(f), L.ROLE_OUT)]).astype(np.int32), factor_ids=np.concatenate([model.factor_ids, f]).astype(np.int64),
        factor_kind=np.concatenate([model.factor_kind, np.full(len(f), L.FACTOR_OPAQUE)]).astype(np.int32),
        factor_var=np.concatenate([model.factor_var, np.zeros(len(f))])), f


def _spd(d, seed):
    G = np.random.default_rng(seed).standard_normal((d, d))
    return G @ G.T / d + 0.5 * np.eye(d)


def prior_chain(d, T=6):
    """(model, opaque): lgssm_chain(T, d) with a proper prior on x_1 as an opaque message, N⁻¹(η, Λ) with Λ a dense positive definite
    matrix and η of the data's size.  opaque = (variable ids, factor ids, η [1, d], Λ [1, d, d]) as evidence_support.gmodel takes it"""
    base = cx.synth.lgssm_chain(T, d=d, seed=600 + d)
    m, f = _with_opaque(base, base.x_ids[:1])
    eta = np.random.default_rng(601 + d).standard_normal((1, d)) * 2.0
    return m, (m.x_ids[:1], f, eta, _spd(d, 602 + d)[None])


def flat_opaque_tail(d, T=9, h=3):
    """(model, opaque): forecast_chain's model whose last state carries, in place of nothing, an OPAQUE message of natural zeros (the flat
    forecast end as a caller-set factor→variable message), and a proper opaque prior on x_1 beside it"""
    base = MD.tail(MD.thin(cx.synth.lgssm_chain(T, d=d, seed=800 + d), MD.alt(T)), h)
    ends = np.array([base.x_ids[0], base.x_ids[-1]])
    m, f = _with_opaque(base, ends)
    eta = np.vstack([np.random.default_rng(611 + d).standard_normal(d), np.zeros(d)])
    lam = np.stack([_spd(d, 612 + d), np.zeros((d, d))])
    return m, (ends, f, eta, lam)


def set_opaque(dev, opaque):
    v, f, eta, lam = opaque
    dev.set_messages(v, f, L.TO_VARIABLE, L.FORM_NATURAL, np.concatenate([eta, lam.reshape(len(v), -1)], axis=1))


def forecast_chain(d, T=9, h=3):
    """(model with the tail, the same model without it): the tail's own terms sum to zero, so both have one log-evidence"""
    thin = MD.thin(cx.synth.lgssm_chain(T, d=d, seed=800 + d), MD.alt(T))
    return MD.tail(thin, h), thin
