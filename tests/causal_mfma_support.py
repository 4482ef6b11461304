"""Shared by the cx_causal_marginals_mfma tests (tests/test_gpu_causal_marginals_mfma.py, pinned on the CPU by
tests/test_causal_mfma_checker.py).  The references are those of tests/causal_support.py (causal_from_messages: the definition on arrays
of messages; dense_causal_all: the dense solve without the data a mode leaves out), the models those of
tests/predictive_mfma_support.forest_cases(); added here are the Kalman statements of a chain:

  kalman(model)        missing_data.kalman_filter of a chain of tests/missing_data.py: mf, Pf (filtered), mp, Pp (predicted)
  rts_lag(s, f, L)     the fixed-lag smoother p(x_t | y_<=t+L) written as L Rauch-Tung-Striebel steps back from the filtered state at
                       min(t + L, n - 1)

and two models with a state of MORE than three sources (its datum and three transitions onward), which the backward pass sums into a
scratch record first — no model of predictive_mfma_support has one:

  branching(d)         a tree of 13 states, three children per node: the three states below the root have four sources each
  two_parents(d)       the same with a 14th state, a second root that is a second parent of the first inner state: that state is the
                       OUT end of TWO transitions, which share its summed record.  Still a forest, but a state with two parents couples
                       them once its descendants' data are left out: the dense solve is no reference, the definition on messages is
"""
from __future__ import annotations

import numpy as np

from tests import anisotropic as AN
from tests import causal_support as CS
from tests import missing_data as MD

# (name of the mode for DeviceGraph.causal_marginals_mfma, lag, mode of causal_support)
MODES = (("predicted", 0, CS.PREDICTED), ("filtered", 0, CS.FILTERED), ("filtered", 1, CS.FILTERED), ("filtered", 3, CS.FILTERED), ("filtered", 12, CS.FILTERED))

BRANCH_DIMS = (16, 20, 32, 64)      # one per tile size, and one embedded (20 in 32)
BRANCH_MODES = MODES[1:]            # filtered, and lags 1, 3, 12: from lag 2 on the summed record reads β of the other buffer


def _tree_pairs(n, b):
    return [(p, c) for p in range(n) for c in range(b * p + 1, b * p + b + 1) if c < n]


def branching(d):
    return AN.branching(13, d, 3)


def two_parents(d):
    return AN.branching(14, d, 3, pairs=_tree_pairs(13, 3) + [(13, 1)])


def kalman(model):
    """(chain_spec, kalman_filter) of a chain whose first state has a datum"""
    s = MD.chain_spec(model)
    return s, MD.kalman_filter(s["A"], s["b"], s["Q"], s["H"], s["R"], s["y"], s["keep"])


def rts_lag(s, f, lag):
    """(means [n, d], covariances [n, d, d]) of p(x_t | y_<=t+lag) from kalman_filter's result"""
    A = s["A"]
    mf, Pf, mp, Pp = f["mf"], f["Pf"], f["mp"], f["Pp"]
    n = len(mf)
    ms, Ps = mf.copy(), Pf.copy()
    for t in range(n):
        m, P = mf[min(t + lag, n - 1)], Pf[min(t + lag, n - 1)]
        for k in range(min(t + lag, n - 1) - 1, t - 1, -1):
            G = np.linalg.solve(Pp[k + 1], A[k] @ Pf[k]).T
            m = mf[k] + G @ (m - mp[k + 1])
            P = Pf[k] + G @ (P - Pp[k + 1]) @ G.T
            P = 0.5 * (P + P.T)
        ms[t], Ps[t] = m, P
    return ms, Ps


def rows(mean, cov, ids=None):
    """(mean, cov) arrays as a result in causal_support's layout, every row finite"""
    n = len(mean)
    return {"variable_ids": np.arange(n) if ids is None else np.asarray(ids), "mean": np.asarray(mean), "cov": np.asarray(cov), "status": np.zeros(n, np.int64)}


def status_of(res):
    """0 finite, 2 NaN, from a device result (the counts tell undefined from improper)"""
    return np.where(np.isnan(np.asarray(res["mean"])).any(axis=1), 2, 0)
