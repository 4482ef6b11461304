"""Shared by the cx_log_evidence_components_mfma tests (tests/test_gpu_evidence_components_mfma.py, pinned on the CPU by
tests/test_components_mfma_checker.py): the graphs of several components at the matrix-core dims, each built once and never changed.
The helpers are those of tests/components_support.py and tests/evidence_support.py; numpy only.

  chains(d)    three chains of 2, 3 and 9 states under one (A, Q, R) as one graph: (parts, model, dense_log_z of every part alone)
  forest(d)    lgssm_comb(4, d, teeth=1) and two chains under the comb's (A, Q, R) as one graph
  borders()    d = 5: one chain of 400 states (1,199 terms: more than one tile of 1,024), 70 chains of 2 states and a lone variable with an
               opaque prior, every id relabelled
  rings(d)     two evidence_mfma_support.ring models (one loop each) as one graph
"""
from __future__ import annotations

import functools

import numpy as np

import cortex.jl_amd as cx
from tests import components_support as CS
from tests import evidence_mfma_support as S
from tests import evidence_support as E

DIMS = (5, 16, 17, 33, 64)      # 5: the least; 17, 33: the first of the next tile size; 16, 64: native
LENGTHS = (2, 3, 9)
LONG, N_SHORT = 400, 70


@functools.lru_cache(maxsize=None)
def chains(d):
    parts = CS.chain_parts(d, LENGTHS)
    return parts, cx.synth.concat_models(parts), tuple(E.dense_log_z(E.gmodel(p)) for p in parts)


@functools.lru_cache(maxsize=None)
def forest(d):
    comb = cx.synth.lgssm_comb(4, d=d, teeth=1, seed=50 + d)
    A, Q = comb.psets[0]
    R = comb.psets[1][1]
    return cx.synth.concat_models([comb] + [cx.synth.lgssm_chain(T, d=d, seed=60 + d + T, A=A, Q=Q, R=R) for T in (3, 6)])


@functools.lru_cache(maxsize=None)
def borders():
    """(model, opaque message of the lone variable under the new ids, component of every part, dense_log_z of every part alone, C)"""
    d = 5
    first = cx.synth.lgssm_chain(LONG, d=d, seed=77)
    A, Q, R = first.meta["A"], first.meta["Q"], first.meta["R"]
    parts = [first] + [cx.synth.lgssm_chain(2, d=d, seed=1000 + i, A=A, Q=Q, R=R) for i in range(N_SHORT)]
    lone, opq = CS.lone_variable(d)
    lone.data_y = np.zeros((0, d))
    wants = [E.dense_log_z(E.gmodel(p)) for p in parts] + [E.dense_log_z(E.gmodel(lone, opaque=opq))]
    cat = cx.synth.concat_models(parts + [lone])
    model = CS.relabel(cat, np.random.default_rng(29))
    offs = [o for _, o in cat.meta["parts"]]
    ids, lab, n = CS.labels(model)
    comp_of_part = [int(lab[np.searchsorted(ids, CS.new_id(model, 1 + o))]) for o in offs]
    opq_new = (np.array([CS.new_id(model, 1 + offs[-1])], np.int64), np.array([CS.new_id(model, 2 + offs[-1])], np.int64), opq[2], opq[3])
    return model, opq_new, comp_of_part, wants, n


@functools.lru_cache(maxsize=None)
def rings(d):
    """two rings under the first one's (A, Q, R) (concat_models keeps the first part's parameter sets): the same precisions, other data"""
    return cx.synth.concat_models([S.ring(d), S.ring(d, seed=701 + d)])
