"""Shared by the cx_predictive_mfma tests (tests/test_gpu_predictive_mfma.py, pinned on the CPU by tests/test_predictive_mfma_checker.py):
the models of the GPU tests by name, and the references of tests/predictive_support.py, tests/missing_data.py and
tests/evidence_support.py brought to one layout (the dict of predictive_support.predictive_from_messages).

  forest_cases()     name -> builder of (model, opaque or None) for every forest the GPU tests run (the ring of test 6 is no forest: its
                     reference is the formula on the device's own messages; the long chains of test 10 are lgssm_chain like the short ones)
  leading_gap(d)     anisotropic.chain(5, d) without the likelihood of its FIRST state: x_1 is a latent leaf whose flat message reaches
                     x_2 through the first transition as the rounding of C - B M^-1 B' — the input of the flat-pivot rule
  causal_reference   the Kalman statement of the CX_PREDICT_CAUSAL rows of a chain
"""
from __future__ import annotations

import numpy as np

import cortex.jl_amd as cx
from tests import anisotropic as AN
from tests import evidence_mfma_support as S
from tests import missing_data as MD
from tests import predictive_support as P

SCHEDULE_DIMS = (5, 8, 16, 17, 32, 33, 64)      # 5: the least; 17, 33: the first of the next tile size; 16, 32, 64: native
GEN_DIMS = (5, 16, 17, 40, 64)
PRIOR_DIMS = (16, 8)
CLAMPED_DIMS = (16, 40)
GAP_KEEP = (False, True, True, True, True)


def chain(d):
    return cx.synth.lgssm_chain(6, d=d, seed=30 + d)


def comb(d):
    return cx.synth.lgssm_comb(4, d=d, teeth=1, seed=40 + d)


def gen(d):
    return MD.make("gen", 9, d, "alt", 3)


def leading_gap(d):
    return MD.thin(AN.chain(5, d), np.array(GAP_KEEP))


def forest_cases():
    out = {}
    for d in SCHEDULE_DIMS:
        out[f"chain d={d}"] = lambda d=d: (chain(d), None)
        out[f"comb d={d}"] = lambda d=d: (comb(d), None)
    for d in GEN_DIMS:
        out[f"gen alt tail d={d}"] = lambda d=d: (gen(d), None)
        out[f"leading gap d={d}"] = lambda d=d: (leading_gap(d), None)
    for d in PRIOR_DIMS:
        out[f"prior d={d}"] = lambda d=d: S.prior_chain(d)
    for d in CLAMPED_DIMS:
        out[f"clamped middle d={d}"] = lambda d=d: (S.clamped_middle(d), None)
    return out


def as_rows(factor_ids, yhat, cov, log_density, maha):
    """arrays in the order of factor_ids -> the dict assert_rows_close compares (a NaN log density: status 2, as the references leave
    out nothing but the improper row)"""
    ld = np.asarray(log_density, float)
    return {"factor_ids": np.asarray(factor_ids, np.int64), "mean": np.asarray(yhat, float), "cov": np.asarray(cov, float), "log_density": ld,
            "mahalanobis": np.asarray(maha, float), "status": np.where(np.isnan(ld), 2, 0)}


def innovations_rows(model):
    """predictive_support.innovations_of_chain of an lgssm_chain, rows in ascending factor id of the likelihoods"""
    yh, Sm, term, maha = P.innovations_of_chain(model)
    fac = np.asarray(model.data_fac)
    o = np.argsort(fac, kind="stable")
    return as_rows(fac[o], yh[o], Sm[o], term[o], maha[o])


def kalman_rows(model):
    """(rows, log_first) of missing_data.kalman_missing"""
    k = MD.kalman_missing(model)
    return as_rows(k["factor_ids"], k["yhat"], k["S"], k["log_density"], k["mahalanobis"]), float(k["log_first"])


def status_of(res):
    """0 scored, 2 not scored, from a device result (the counts tell undefined from improper)"""
    return np.where(np.isnan(np.asarray(res["log_density"])), 2, 0)
