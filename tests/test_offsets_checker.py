"""The references of the factor-offset tests (tests/offsets_support.py) against each other, numpy against numpy on graphs of at most 40
states, at 1e-10: the joint solve with offsets, the GModel with offsets (dense log Z, dense posterior, numpy BP), the shift-equivalent
twin, and the M-step's intercept.  Also what Change::RuleOffsets voids (csrc/cx_derived.h)."""
import ctypes as C

import numpy as np
import pytest

from cortex.jl_amd import learn
from tests import anisotropic as AN
from tests import evidence_support as E
from tests import hostlogic as H
from tests import learning_support as LS
from tests import offsets_support as O

TOL = 1e-10


def _close(a, b, what):
    a, b = np.asarray(a, float), np.asarray(b, float)
    err = float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0)))
    assert err <= TOL, (what, err)


MODELS = {"comb": lambda: AN.comb(12, 3, teeth=1), "loopy": lambda: AN.loopy(20, 3)}


@pytest.mark.parametrize("name", MODELS)
def test_joint_solve_with_offsets_agrees_with_the_gmodel(name):
    model = MODELS[name]()
    b = O.with_offsets(model, 5)
    mean, S, pos, log_z = O.joint_solve_offsets(model, b)
    gm = O.gmodel_offsets(model, b)
    _close(E.dense_log_z(gm), log_z, name + " log Z")
    gmean, gS, fpos = LS.dense_posterior(gm)
    d = model.dim
    for v, a in pos.items():
        i = int(np.searchsorted(gm.var_ids, v))
        _close(gmean[i], mean[a * d:(a + 1) * d], f"{name} mean of {v}")
        p = fpos[i]
        _close(gS[p * d:(p + 1) * d, p * d:(p + 1) * d], S[a * d:(a + 1) * d, a * d:(a + 1) * d], f"{name} covariance of {v}")
    # the offsets matter: the zero-offset model has another mean and another evidence
    m0, _, _, z0 = AN.joint_solve(model)
    assert np.max(np.abs(m0 - mean)) > 0.1 and abs(z0 - log_z) > 0.1


def test_zero_offsets_are_the_model_without():
    model = AN.comb(12, 3, teeth=1)
    a, b = O.joint_solve_offsets(model, {}), AN.joint_solve(model)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    _close(a[3], b[3], "log Z")


@pytest.mark.parametrize("name", MODELS)
def test_consistent_offsets_are_a_shift(name):
    model = MODELS[name]()
    b, s = O.consistent_offsets(model, 7)
    twin, to_twin = O.shifted_twin(model, b, s)
    mean, S, pos, log_z = O.joint_solve_offsets(model, b)
    tm, tS, tpos, tz = AN.joint_solve(twin)
    assert pos == tpos
    d = model.dim
    shift = np.concatenate([s[v] for v in sorted(pos, key=pos.get)])
    _close(mean, tm + shift, name + " means differ by s")
    _close(S, tS, name + " covariances")
    _close(log_z, tz, name + " log Z")


def test_messages_of_consistent_offsets_are_the_twins_shifted():
    """every message of the offset model is the twin's under Lambda' = Lambda, eta' = eta - Lambda s (numpy BP on a comb)"""
    model = AN.comb(12, 2, teeth=1)
    b, s = O.consistent_offsets(model, 7)
    twin, to_twin = O.shifted_twin(model, b, s)
    gm, gt = O.gmodel_offsets(model, b), E.gmodel(twin)
    (e, l), (te, tl) = E.numpy_bp(gm)[2], E.numpy_bp(gt)[2]
    d = model.dim
    g = gm.groups[2]
    for j in range(2):
        ok = ~gm.obs[g["vars"][:, j]]
        nat = np.concatenate([e[ok, j], l[ok, j].reshape(-1, d * d)], axis=1)
        want = np.concatenate([te[ok, j], tl[ok, j].reshape(-1, d * d)], axis=1)
        got = to_twin(gm.var_ids[g["vars"][ok, j]], nat)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        _close(np.nan_to_num(got), np.nan_to_num(want), f"messages of end {j}")


def test_numpy_bp_on_a_tree_reproduces_the_joint_solve():
    model = AN.comb(12, 2, teeth=1)
    b = O.with_offsets(model, 3)
    gm = O.gmodel_offsets(model, b)
    f2v = E.numpy_bp(gm)
    d, nv = gm.d, len(gm.var_ids)
    eta, lam = np.zeros((nv, d)), np.zeros((nv, d, d))
    g = gm.groups[2]
    e, l = f2v[2]
    assert not np.isnan(l[~gm.obs[g["vars"]]]).any()
    for j in range(2):
        ok = ~gm.obs[g["vars"][:, j]]
        np.add.at(eta, g["vars"][ok, j], e[ok, j])
        np.add.at(lam, g["vars"][ok, j], l[ok, j])
    mean, S, pos, log_z = O.joint_solve_offsets(model, b)
    for v, a in pos.items():
        i = int(np.searchsorted(gm.var_ids, v))
        cov = np.linalg.inv(lam[i])
        _close(cov @ eta[i], mean[a * d:(a + 1) * d], f"mean of {v}")
        _close(cov, S[a * d:(a + 1) * d, a * d:(a + 1) * d], f"covariance of {v}")
    _close(E.bethe_log_z(gm, f2v), log_z, "Bethe log Z on a tree")


def test_m_step_recovers_a_planted_intercept_from_exact_statistics():
    """statistics of n exact residual / input pairs taken under (A0, b0) when the truth is (A*, b*): one M-step lands on the truth"""
    rng = np.random.default_rng(11)
    d, n = 3, 50
    A_true, b_true = 0.5 * rng.standard_normal((d, d)), rng.standard_normal(d)
    A0, b0 = A_true + 0.1 * rng.standard_normal((d, d)), np.zeros(d)
    x = rng.standard_normal((n, d))
    noise = 0.05 * rng.standard_normal((n, d))
    noise -= noise.mean(axis=0)
    noise -= x @ np.linalg.lstsq(np.hstack([x, np.ones((n, 1))]), noise, rcond=None)[0][:d]      # orthogonal to [x, 1]: the regression is exact
    noise -= noise.mean(axis=0)
    xo = x @ A_true.T + b_true + noise
    r = xo - x @ A0.T - b0
    st = {"n": np.array([float(n)]), "sum_r": r.sum(0), "sum_x": x.sum(0), "S_rr": r.T @ r, "S_rx": r.T @ x, "S_xx": x.T @ x}
    new = learn.m_step(st, A0, b0, learn=("A", "b", "Q"))
    _close(new["A"], A_true, "A")
    _close(new["b"], b_true, "b")
    _close(new["Q"], noise.T @ noise / n, "Q")
    only_b = learn.m_step(st, A0, b0, learn=("b",))
    _close(only_b["b"], b0 + r.mean(0), "b alone: the mean residual")
    assert np.array_equal(only_b["A"], A0) and only_b["Q"] is None


# ---- what the change voids (cx_derived.h: Change::RuleOffsets) -------------------------------------------------------------------------
def _apply_offsets(dim, flags=None):
    L = H.lib()
    L.cxh_derived_apply_offsets.restype = C.c_int32
    L.cxh_derived_apply_offsets.argtypes = [C.c_int32, C.c_void_p, C.c_void_p]
    flags = H.DERIVED_CLEAN if flags is None else flags
    a = np.array([flags[f] for f in H.DERIVED_FLAGS], dtype=np.int64)
    out = np.zeros_like(a)
    assert L.cxh_derived_apply_offsets(int(dim), a.ctypes.data, out.ctypes.data) == 0
    return dict(zip(H.DERIVED_FLAGS, out.tolist()))


def test_rule_offsets_voids_what_reads_eta():
    """the cached messages out of observed variables (both Jacobi buffers), the chains' leaf messages and side sums, and the parameter
    epoch of the derived calls' caches — what RuleMatrices voids and that reads eta; nothing else (precisions, plans and k-ary tables
    do not see b)"""
    after = _apply_offsets(3)
    moved = {f for f in H.DERIVED_FLAGS if after[f] != H.DERIVED_CLEAN[f]}
    assert moved == {"param_epoch", "observed_passes_due", "chain_side_dirty"}
    assert after["observed_passes_due"] == 2 and after["param_epoch"] == 1
    matrices = H.derived_apply(3, "RuleMatrices")
    assert moved <= {f for f in H.DERIVED_FLAGS if matrices[f] != H.DERIVED_CLEAN[f]}
    # a change only ever raises
    due = {**{f: 1 for f in H.DERIVED_FLAGS}, "observed_passes_due": 2, "pot64_fresh": 0, "vinfo_epoch": 7, "param_epoch": 7}
    again = _apply_offsets(3, due)
    for f in H.DERIVED_FLAGS:
        assert again[f] >= due[f] if f != "pot64_fresh" else again[f] == 0, f
    # the numbered entry still ends where its table does
    with pytest.raises(ValueError):
        H.derived_apply(3, len(H.CHANGES))
