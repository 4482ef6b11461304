"""Shared by the matrix-core reader tests on GENERAL models (tests/test_gpu_general_mfma.py, pinned on the CPU by
tests/test_general_mfma_checker.py): the models of cx_log_evidence_mfma, cx_factor_beliefs_mfma, cx_factor_statistics_mfma and
cx_log_evidence_components_mfma with the matrices of tests/anisotropic.py — A non-normal, Q and R dense SPD, H neither symmetric nor the
identity — in place of the isotropic ones of synth.py, on which H' for H, a wrong triangle or a dropped off-diagonal tile changes nothing.
Every model is built once (functools.lru_cache) and never changed; numpy only.

  chain(d) / comb(d)   anisotropic.chain(6, d) / anisotropic.comb(4, d, teeth=1)
  gen(d)               predictive_mfma_support.gen(d): a datum at every second state, three forecast states (load with missing_data.load)
  prior(d)             (model, opaque): anisotropic.chain(6, d) with the dense SPD opaque prior of evidence_mfma_support.prior_chain on x_1
  clamped(d)           anisotropic.chain(5, d) with state 2 observed on every one of its edges
  ring(d)              anisotropic.chain(5, d) closed by one more set-0 factor x_T (IN) -> x_1 (OUT): one loop
  parts(d)             (parts, model): three general chains of 2, 3 and 9 states under one general_sets as one graph, the data of every
                       part from a random stream of its own
  forest(d)            anisotropic.comb(4, d, teeth=1) and two such chains (3 and 6 states) as one graph
  velocity(d)          anisotropic.velocity_chain(6, d): H has zero rows for the velocities
  second_sets(d)       another (A, Q, R, H) for the tests that change parameters on one handle
  em_case()            anisotropic.chain(60, 17) and perturbed general starts (A0, Q0, C0, R0)
  gpu_models()         name -> builder of (model, opaque or None) of every model above; the checker walks it
"""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np

from cortex.jl_amd import _lib as L
from cortex.jl_amd import synth
from tests import anisotropic as AN
from tests import components_support as CS
from tests import evidence_mfma_support as S
from tests import predictive_mfma_support as PM

DIMS = (5, 8, 16, 17, 32, 33, 40, 64)      # 5: the least; 17, 33: the first of the next tile size; 8, 40: embedded; 16, 32, 64: native
GEN_DIMS = PM.GEN_DIMS
PRIOR_DIMS = (16, 8)
CLAMPED_DIMS = (16, 40)
RING_DIMS = (5, 16, 64)
RING_T, RING_SWEEPS, RING_SEED_VARIANCE = 5, 150, 1e6
DIMS_C = (5, 16, 17, 33, 64)
LENGTHS = (2, 3, 9)
FOREST_DIMS = (5, 17)
FOREST_CHAINS = (3, 6)
VELOCITY_DIMS = (6, 16, 40, 64)
EMBEDDED_DIMS = (8, 20)
SET_CHANGE_DIMS = (16, 40)
EM_T, EM_D, EM_ITER = 60, 17, 4


@functools.lru_cache(maxsize=None)
def chain(d):
    return AN.chain(6, d)


@functools.lru_cache(maxsize=None)
def comb(d):
    return AN.comb(4, d, teeth=1)


@functools.lru_cache(maxsize=None)
def gen(d):
    return PM.gen(d)


@functools.lru_cache(maxsize=None)
def prior(d):
    """(model, opaque) with opaque = (variable ids, factor ids, eta [1, d], Lambda [1, d, d]) as evidence_support.gmodel takes it"""
    base = AN.chain(6, d)
    m, f = S._with_opaque(base, base.x_ids[:1])
    eta = np.random.default_rng(601 + d).standard_normal((1, d)) * 2.0
    return m, (m.x_ids[:1], f, eta, S._spd(d, 602 + d)[None])


@functools.lru_cache(maxsize=None)
def clamped(d, T=5, i=2):
    """the construction of evidence_mfma_support.clamped_middle on the general chain: the likelihood of state i has both ends observed,
    the transition into it an observed OUT end (J = -A), the transition out of it an observed IN end (eta' = B y)"""
    m = AN.chain(T, d)
    x = m.x_ids[i]
    facs = np.asarray(m.edge_fac)[np.asarray(m.edge_var) == x]
    value = np.random.default_rng(901 + d).standard_normal(d)
    return dataclasses.replace(m, data_var=np.concatenate([m.data_var, np.full(len(facs), x)]), data_fac=np.concatenate([m.data_fac, facs]),
                               data_y=np.vstack([m.data_y, np.tile(value, (len(facs), 1))]), meta={**m.meta, "clamped_state": i})


@functools.lru_cache(maxsize=None)
def ring(d):
    """the general chain first (anisotropic._simulate needs a root), then the closing edge as evidence_mfma_support.ring adds it"""
    m = AN.chain(RING_T, d)
    f = int(max(np.max(m.edge_var), np.max(m.edge_fac))) + 1
    return dataclasses.replace(
        m, edge_var=np.concatenate([m.edge_var, [m.x_ids[-1], m.x_ids[0]]]).astype(np.int64), edge_fac=np.concatenate([m.edge_fac, [f, f]]).astype(np.int64),
        edge_role=np.concatenate([m.edge_role, [L.ROLE_IN, L.ROLE_OUT]]).astype(np.int32), factor_ids=np.concatenate([m.factor_ids, [f]]).astype(np.int64),
        factor_kind=np.concatenate([m.factor_kind, [L.FACTOR_GAUSS_LINEAR]]).astype(np.int32), factor_var=np.concatenate([m.factor_var, [0.0]]),
        meta={**m.meta, "kind": "lgssm_ring"})


def _chain_part(T, d, part):
    """anisotropic.chain(T, d) with data from a stream keyed by `part`: anisotropic.chain draws the data of every length from ONE stream,
    so two chains of different lengths would share their first data"""
    m = AN.chain(T, d)
    return dataclasses.replace(m, data_y=AN._simulate(m, np.random.default_rng([AN.seed_of(d), d, 78, 1 + part])))


@functools.lru_cache(maxsize=None)
def parts(d):
    """(the parts, the joined model); synth.concat_models keeps the first part's parameter sets, which are every part's"""
    ps = tuple(_chain_part(T, d, k) for k, T in enumerate(LENGTHS))
    return ps, synth.concat_models(list(ps))


@functools.lru_cache(maxsize=None)
def forest(d):
    return synth.concat_models([AN.comb(4, d, teeth=1)] + [_chain_part(T, d, 10 + k) for k, T in enumerate(FOREST_CHAINS)])


@functools.lru_cache(maxsize=None)
def forest_relabelled(d):
    return CS.relabel(forest(d), np.random.default_rng(31))


@functools.lru_cache(maxsize=None)
def velocity(d):
    return AN.velocity_chain(6, d)


@functools.lru_cache(maxsize=None)
def second_sets(d):
    return AN.general_sets(d, AN.seed_of(d) + 100)


@functools.lru_cache(maxsize=None)
def em_case():
    """(model, A0, Q0, C0, R0): the starts of tests/test_gpu_learn_mfma.py's EM test around the general matrices"""
    d = EM_D
    model = AN.chain(EM_T, d)
    rng = np.random.default_rng(d)
    m = model.meta
    A0 = m["A"] + 0.05 * rng.standard_normal((d, d)) / math.sqrt(d)
    C0 = m["H"] + 0.05 * rng.standard_normal((d, d)) / math.sqrt(d)
    return model, A0, 2.0 * m["Q"], C0, 0.5 * m["R"]


def gpu_models():
    """name -> builder of (model, opaque or None) of every model tests/test_gpu_general_mfma.py runs (the EM chain has its own CPU test)"""
    out = {}
    for d in DIMS + (20,):
        out[f"chain d={d}"] = lambda d=d: (chain(d), None)
    for d in DIMS:
        out[f"comb d={d}"] = lambda d=d: (comb(d), None)
    for d in GEN_DIMS:
        out[f"gen d={d}"] = lambda d=d: (gen(d), None)
    for d in PRIOR_DIMS:
        out[f"prior d={d}"] = lambda d=d: prior(d)
    for d in CLAMPED_DIMS:
        out[f"clamped d={d}"] = lambda d=d: (clamped(d), None)
    for d in RING_DIMS:
        out[f"ring d={d}"] = lambda d=d: (ring(d), None)
    for d in DIMS_C:
        out[f"parts d={d}"] = lambda d=d: (parts(d)[1], None)
    for d in FOREST_DIMS:
        out[f"forest d={d}"] = lambda d=d: (forest(d), None)
        out[f"forest relabelled d={d}"] = lambda d=d: (forest_relabelled(d), None)
    for d in VELOCITY_DIMS:
        out[f"velocity d={d}"] = lambda d=d: (velocity(d), None)
    return out


def is_forest(name):
    return not name.startswith("ring")


def is_recipe(name):
    """the models whose every state carries the recipe's general likelihood: chain, comb and gen"""
    return name.startswith(("chain", "comb", "gen"))
