"""-m gpu: cx_sample_posterior against the dense posterior (its mean, and B Bᵀ = Σ through identity noise), the numpy
restatement of the device generator and exact sampling distributions (tests/sampling_support.py, pinned by
tests/test_sampling_checker.py)."""
import ctypes as C
import math

import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from tests import evidence_support as E
from tests import learning_support as LS
from tests import sampling_support as SS
from tests.test_gpu_kary_mv import _kary_tree, _load as _load_kary
from tests.gpu_support import code_of, run_demo
from tests.learning_support import assert_rel_close as _close

pytestmark = pytest.mark.gpu


def _dev(model, schedule, sweeps=1):
    dev = cx.DeviceGraph(dim=model.dim, schedule=schedule)
    cx.synth.load_into_device(model, dev, seed_variance=1e6 if schedule == L.SCHED_FUSED else None)
    dev.sweep(sweeps)
    return dev


EXACT = [("ssm_chain", lambda: cx.synth.ssm_chain(60, seed=301), True),
         ("ssm_chain_linear", lambda: cx.synth.ssm_chain_linear(60, seed=302), True),
         ("kary_model", lambda: cx.synth.kary_model(16, seed=303, tree=True, observe=0.3), False),
         ("tree_model", lambda: cx.synth.tree_model(40, seed=304, observe=0.25, components=3), False)]
EXACT += [(f"lgssm_chain d={d}", (lambda d=d: cx.synth.lgssm_chain(25, d=d, seed=310 + d)), True) for d in (2, 3, 4)]
EXACT += [(f"lgssm_comb d={d}", (lambda d=d: cx.synth.lgssm_comb(6, d=d, teeth=1, seed=320 + d)), False) for d in (2, 3, 4)]


@pytest.mark.parametrize("name,make,chain", EXACT, ids=[m[0] for m in EXACT])
def test_exact_mean_and_covariance(hip_lib, name, make, chain):
    model = make()
    gm = E.gmodel(model)
    mean, Sig, _ = LS.dense_posterior(gm)
    nv, d = len(gm.var_ids), gm.d
    free = np.flatnonzero(~gm.obs)
    eps = SS.identity_noise(gm)
    for s in [L.SCHED_TREE, L.SCHED_REFERENCE] + ([L.SCHED_CHAIN_SCAN] if chain else []):
        dev = _dev(model, s)
        what = f"{name} schedule {s}"
        x0, cnt = dev.sample_posterior(1, noise=np.zeros((1, nv, d)))
        _close(x0[0], mean, 1e-9, what + " mean")
        assert cnt["free"] == len(free) and cnt["undefined"] == 0 and cnt["not_positive_definite"] == 0, (what, cnt)
        x, _ = dev.sample_posterior(len(eps), noise=eps)
        B = SS.samples_to_b(x, mean, gm)
        assert np.max(np.abs(B @ B.T - Sig)) <= 1e-9 * np.max(np.abs(Sig)), what + " B B'"
        assert np.array_equal(x[:, gm.obs], np.broadcast_to(gm.y[gm.obs], x[:, gm.obs].shape)), what + " data"
        dev.close()


@pytest.mark.parametrize("d", [2, 3, 4])
def test_exact_kary_tree_dims_2_to_4(hip_lib, d):
    """CX_FACTOR_GAUSS_LINEAR_N at dim 2 - 4 (factors of 3 .. 6 variables, a parameter set per input, opaque priors): the links of
    k_sp_cond_kary<D> — the parent's block skipped, G / off / L⁻ᵀ scattered over the children, the siblings' d x d noise blocks"""
    model, prior, facs, fid, sets, _m, _c = _kary_tree(12, d, 360 + d, k_choices=(2, 3, 5))
    n = len(model.x_ids)
    edge_sets = {(int(model.x_ids[i]), int(f)): s for f, (_o, ins, ss, _q) in zip(fid, facs) for i, s in zip(ins, ss)}
    gm = E.gmodel(model, edge_sets=edge_sets, opaque=(model.x_ids, model.x_ids + n, prior[0], prior[1]))
    assert max(gm.groups) >= 4
    mean, Sig, _ = LS.dense_posterior(gm)
    nv = len(gm.var_ids)
    eps = SS.identity_noise(gm)
    for s in (L.SCHED_TREE, L.SCHED_REFERENCE):
        dev = _load_kary(model, prior, facs, fid, sets, s)
        dev.sweep(1)
        what = f"d {d} k-ary tree, schedule {s}"
        x0, cnt = dev.sample_posterior(1, noise=np.zeros((1, nv, d)))
        _close(x0[0], mean, 1e-9, what + " mean")
        assert cnt["free"] == int((~gm.obs).sum()) and cnt["undefined"] == 0 and cnt["not_positive_definite"] == 0, (what, cnt)
        x, _ = dev.sample_posterior(len(eps), noise=eps)
        B = SS.samples_to_b(x, mean, gm)
        assert np.max(np.abs(B @ B.T - Sig)) <= 1e-9 * np.max(np.abs(Sig)), what + " B B'"
        assert np.array_equal(x[:, gm.obs], np.broadcast_to(gm.y[gm.obs], x[:, gm.obs].shape)), what + " data"
        dev.close()


def test_generator(hip_lib):
    for model, s in [(cx.synth.lgssm_chain(30, d=3, seed=330), L.SCHED_CHAIN_SCAN), (cx.synth.tree_model(60, seed=331, observe=0.2), L.SCHED_TREE)]:
        dev = _dev(model, s)
        nv, d = dev.stats()["n_variables"], model.dim
        x, _ = dev.sample_posterior(5, seed=7)
        y, _ = dev.sample_posterior(5, noise=SS.normals(7, np.arange(5), nv, d))
        _close(x, y, 1e-12, "Philox restated")
        assert np.array_equal(x, dev.sample_posterior(5, seed=7)[0])                       # bit-identical
        x10, _ = dev.sample_posterior(10, seed=7)
        assert np.array_equal(x10[:5], x) and np.array_equal(dev.sample_posterior(3, seed=7)[0], x10[:3])
        ids = np.unique(model.edge_var)
        sub = ids[::3][::-1]
        got, _ = dev.sample_posterior(5, seed=7, variable_ids=sub)
        assert np.array_equal(got, x[:, np.searchsorted(ids, sub)])
        other, _ = dev.sample_posterior(5, seed=8)
        assert not np.allclose(other, x)
        dev.close()


def _ks_normal(x, m, v):
    x = np.sort(np.asarray(x, float))
    n = len(x)
    erf = np.frompyfunc(math.erf, 1, 1)
    cdf = 0.5 * (1.0 + erf((x - m) / math.sqrt(2.0 * v)).astype(float))
    i = np.arange(1, n + 1)
    return max(float(np.max(i / n - cdf)), float(np.max(cdf - (i - 1) / n)))


def test_statistics(hip_lib):
    y, r = 1.3, 0.5
    dev = _dev(E.one_variable_model(y, r), L.SCHED_TREE)
    v = 1.0 / (1.0 + 1.0 / r)
    m = v * y / r
    n = 1 << 20
    x, _ = dev.sample_posterior(n, seed=11, variable_ids=[1])
    assert _ks_normal(x.ravel(), m, v) < 1.95 / math.sqrt(n)                                  # p ~ 0.001
    dev.close()
    model = cx.synth.lgssm_chain(40, d=2, seed=340)
    gm = E.gmodel(model)
    mean, Sig, _ = LS.dense_posterior(gm)
    dev = _dev(model, L.SCHED_CHAIN_SCAN)
    n = 1 << 16
    x, _ = dev.sample_posterior(n, seed=12, variable_ids=model.x_ids)
    z = x.reshape(n, -1)
    free = np.searchsorted(gm.var_ids, model.x_ids)
    mu = mean[free].ravel()
    assert np.all(np.abs(z.mean(0) - mu) <= 6 * np.sqrt(np.diag(Sig) / n))
    C = np.cov(z, rowvar=False)
    sd = np.sqrt((np.outer(np.diag(Sig), np.diag(Sig)) + Sig ** 2) / n)
    assert np.all(np.abs(C - Sig) <= 6 * sd)
    dev.close()


def _standardised(x, marg, d):
    m, cov = marg[:, :d], marg[:, d:].reshape(-1, d, d)
    Li = np.linalg.inv(np.linalg.cholesky(cov))
    return np.einsum("tij,stj->sti", Li, x - m[None]).ravel()


def test_size(hip_lib):
    for model, s in [(cx.synth.lgssm_chain(1_000_000, d=4), L.SCHED_CHAIN_SCAN), (cx.synth.ssm_chain(250_001, seed=1234), L.SCHED_CHAIN_SCAN),
                     (cx.synth.tree_model(200_000, shape="deep", observe=0.2), L.SCHED_TREE)]:
        dev = _dev(model, s)
        d = model.dim
        nv = dev.stats()["n_variables"]
        marg = dev.get_marginals(model.x_ids)
        x0, cnt = dev.sample_posterior(1, variable_ids=model.x_ids, noise=np.zeros((1, nv, d)))
        _close(x0[0], marg[:, :d], 1e-8, f"mean, {len(model.x_ids)} states d={d}")
        assert cnt["undefined"] == 0 and cnt["not_positive_definite"] == 0
        x, _ = dev.sample_posterior(4, seed=21, variable_ids=model.x_ids)
        w = _standardised(x, marg, d) if d > 1 else ((x[:, :, 0] - marg[None, :, 0]) / np.sqrt(marg[None, :, 1])).ravel()
        n = len(w)
        assert abs(w.mean()) < 6 / math.sqrt(n) and abs(w.var() - 1.0) < 6 * math.sqrt(2.0 / n), (w.mean(), w.var())
        dev.close()


def test_no_side_effects(hip_lib):
    model = cx.synth.lgssm_chain(30, d=2, seed=350)
    dev = _dev(model, L.SCHED_CHAIN_SCAN)
    dev.sample_posterior(1, seed=1)                     # (the chain scan brings its messages to their slots on first read)
    blob, health, marg = dev.export_state(), dev.message_health(), dev.get_marginals(model.x_ids)
    msgs = dev.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE)
    dev.sample_posterior(7, seed=2)
    assert np.array_equal(blob, dev.export_state()) and np.array_equal(marg, dev.get_marginals(model.x_ids))
    assert np.array_equal(msgs, dev.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE), equal_nan=True)
    assert np.array_equal(np.asarray(health), np.asarray(dev.message_health()))
    dev.close()
    model = cx.synth.tree_model(40, seed=351, k_choices=(1, 2, 3), observe=0.2)
    dev = _dev(model, L.SCHED_REFERENCE)
    blob, trace = dev.export_state(), dev.ref_trace()
    dev.sample_posterior(3, seed=3)
    assert np.array_equal(blob, dev.export_state()) and dev.ref_trace() == trace
    dev.close()


def _components(gm):
    """component label of every free variable index (the others: -1)"""
    lab = -np.ones(len(gm.var_ids), np.int64)
    parent = list(range(len(gm.var_ids)))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for g in gm.groups.values():
        for vs in g["vars"]:
            fv = [int(v) for v in vs if not gm.obs[v]]
            for a in fv[1:]:
                parent[find(a)] = find(fv[0])
    for v in np.flatnonzero(~gm.obs):
        lab[v] = find(int(v))
    return lab


def test_undefined_component_is_nan(hip_lib):
    model = cx.synth.tree_model(40, seed=360, observe=0.25, components=3)
    gm = E.gmodel(model)
    mean, _, _ = LS.dense_posterior(gm)
    lab = _components(gm)
    bad = lab == lab[np.flatnonzero(~gm.obs)[0]]
    dev = cx.DeviceGraph(schedule=L.SCHED_REFERENCE)
    cx.synth.load_into_device(model, dev)
    dev.sweep_for(gm.var_ids[(lab >= 0) & ~bad])        # the other components only: the messages of the first are never computed
    x, cnt = dev.sample_posterior(2, seed=4)
    assert cnt["components"] == 3 and cnt["undefined"] == 1 and cnt["not_positive_definite"] == 0, cnt
    assert np.isnan(x[:, bad]).all()
    assert np.isfinite(x[:, ~bad]).all()
    x0, _ = dev.sample_posterior(1, noise=np.zeros((1, len(gm.var_ids), 1)))
    _close(x0[0, ~bad], mean[~bad], 1e-9, "the other components")
    dev.close()


def test_refusals(hip_lib):
    dev = cx.DeviceGraph()
    assert code_of(dev.sample_posterior, 1)[0] == L.ERR_STATE                                          # no graph
    dev.close()
    dev = cx.DeviceGraph(family=L.FAMILY_NATURAL2)
    assert code_of(dev.sample_posterior, 1)[0] == L.ERR_UNSUPPORTED
    dev.close()
    vm = cx.synth.vmp_ssm(8)
    dev = cx.DeviceGraph(schedule=L.SCHED_CHAIN_SCAN, family=L.FAMILY_VMP_STRUCTURED)
    cx.synth.load_vmp_into_device(vm, dev)
    assert code_of(dev.sample_posterior, 1)[0] == L.ERR_UNSUPPORTED
    dev.close()
    dev = _dev(cx.synth.lgssm_chain(4, d=16, seed=370), L.SCHED_FUSED, 2)
    assert code_of(dev.sample_posterior, 1)[0] == L.ERR_UNSUPPORTED                                    # dim >= 5
    dev.close()
    dev = _dev(cx.synth.gaussian_grid(6, 5, seed=371), L.SCHED_FUSED, 5)                             # a loopy graph
    code, msg = code_of(dev.sample_posterior, 1)
    assert code == L.ERR_UNSUPPORTED and "cx_sample_posterior" in msg and "cycle" in msg and "variable" in msg, msg
    dev.close()
    model = cx.synth.ssm_chain(20, seed=372)
    dev = _dev(model, L.SCHED_TREE)
    assert code_of(dev.sample_posterior, 0)[0] == L.ERR_INVALID_ARGUMENT                               # n_samples < 1
    code, msg = code_of(dev.sample_posterior, 1, variable_ids=[99999])
    assert code == L.ERR_NOT_FOUND and "99999" in msg
    ids = np.array([1, 2], np.int64)
    out = np.zeros(2)
    cnt = (C.c_int64 * 4)()
    pi, po = ids.ctypes.data_as(C.POINTER(C.c_int64)), out.ctypes.data_as(C.POINTER(C.c_double))
    assert dev.lib.cx_sample_posterior(dev.h, 1, C.c_uint64(0), None, 2, pi, None, cnt) == L.ERR_INVALID_ARGUMENT      # no output
    assert dev.lib.cx_sample_posterior(dev.h, 1, C.c_uint64(0), None, -1, pi, po, cnt) == L.ERR_INVALID_ARGUMENT       # n < 0 with ids
    dev.halo_configure([1], [2 * 20 + 1], [], [])                                                    # a partitioned handle
    assert code_of(dev.sample_posterior, 1)[0] == L.ERR_UNSUPPORTED
    dev.close()
    model = cx.synth.ssm_chain(10, seed=373, q=0.0)
    dev = cx.DeviceGraph(schedule=L.SCHED_TREE)
    cx.synth.load_into_device(model, dev)
    code, msg = code_of(dev.sample_posterior, 1)
    assert code == L.ERR_UNSUPPORTED and "factor 31" in msg and "zero noise" in msg
    dev.close()


def test_cpp_host_class_sample_posterior(hip_lib, tmp_path):
    out_lines = run_demo("sample_demo", tmp_path)
    rows = {line.split()[0]: [float(v) for v in line.split()[1:]] for line in out_lines}
    T = 50
    model = cx.synth.ssm_chain(T, seed=1)
    model.data_y = np.array([0.5 * t + (7 * t) % 5 for t in range(1, T + 1)], dtype=np.float64)
    gm = E.gmodel(model)
    mean, Sig, _ = LS.dense_posterior(gm)
    xs = np.searchsorted(gm.var_ids, np.arange(1, T + 1))
    _close(rows["mean"], mean[xs, 0], 1e-9, "C++ mean")
    assert rows["counts"] == [T, 1, 0, 0]
    draws = np.asarray(rows["draws"]).reshape(4, T)
    # the values of a draw depend on the device's root and order, its law does not: (x - m)' Σ⁻¹ (x - m) ~ χ²_T, loosely
    r = draws - mean[xs, 0][None]
    q = np.einsum("si,ij,sj->s", r, np.linalg.inv(Sig), r)
    assert np.all(q < T + 12 * math.sqrt(2 * T))
