"""-m gpu: cx_linear_moments against the dense posterior (W μ, W Σ Wᵀ), against cx_sample_posterior through its noise
argument (the adjoint identity, independent of any solve), and against itself (determinism, independence of the other functionals and
of the chunking).  Tolerance: tests/functional_support.REL_TOL, set by the restatement's own error (tests/test_functional_checker.py)."""
import ctypes as C

import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from tests import evidence_support as E
from tests import functional_support as F
from tests import learning_support as LS
from tests import sampling_support as SS
from tests.test_gpu_posterior_samples import _components, _dev
from tests.gpu_support import code_of, run_demo

pytestmark = pytest.mark.gpu
CASES = F.cases()


def _check(dev, gm, fs, dense, what):
    ref = F.dense_moments(gm, fs, dense)
    mean, cov, cnt = dev.linear_moments(fs)
    em, ec = F.rel_errors(mean, cov, *ref)
    print(f"{what}: K = {len(fs)}, mean error {em:.3e}, covariance error {ec:.3e} (tolerance {F.REL_TOL:.1e})")
    assert em <= F.REL_TOL and ec <= F.REL_TOL, (what, em, ec)
    assert np.array_equal(cov, cov.T), what + " symmetry"
    assert cnt["failed"] == 0 and cnt["nan_functionals"] == 0 and cnt["free"] == int((~gm.obs).sum()), (what, cnt)
    return mean, cov, ref


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_dense_posterior(hip_lib, name):
    """every model under every exact schedule: unit functionals (cov = the dense Σ_ij), contrasts inside a tile, across a tile
    boundary and across the whole model, a window mean, siblings of a k-ary factor, a weight on an observed variable"""
    make, chain = CASES[name]
    model, gm, load = make()
    dense = LS.dense_posterior(gm)
    fs, names = F.standard_functionals(gm)
    for s in [L.SCHED_TREE, L.SCHED_REFERENCE] + ([L.SCHED_CHAIN_SCAN] if chain else []):
        dev = _dev(model, s) if load is None else load(s)
        if load is not None:
            dev.sweep(1)
        mean, cov, ref = _check(dev, gm, fs, dense, f"{name} schedule {s}")
        if "with observed" in names:
            a, b = names.index("without observed"), names.index("with observed")
            o = gm.var_ids[gm.obs][int(gm.obs.sum()) // 2]
            shift = 2.0 * gm.y[np.searchsorted(gm.var_ids, o)].sum()
            assert cov[a, a] == cov[b, b] and abs((mean[b] - mean[a]) - shift) <= F.REL_TOL * max(abs(shift), np.sqrt(cov[a, a])), name
        r = names.index("repeat")
        ids, w = fs[r]
        m2, c2, _ = dev.linear_moments([([ids[0], ids[1]], np.stack([w[0] + w[2], w[1]]))])
        assert abs(c2[0, 0] - cov[r, r]) <= 1e-15 * cov[r, r] and abs(m2[0] - mean[r]) <= 1e-13 * max(abs(mean[r]), 1.0)
        dev.close()


def test_long_scalar_chain_third_tile_level(hip_lib):
    """ssm_chain(4200): 66 tiles of 64, a second level of two tiles — contrasts across the whole chain and around positions 4096"""
    model = cx.synth.ssm_chain(4200, seed=402)
    gm = E.gmodel(model)
    dense = LS.dense_posterior(gm)
    fs, _ = F.standard_functionals(gm)
    for s in (L.SCHED_CHAIN_SCAN, L.SCHED_TREE):
        dev = _dev(model, s)
        _check(dev, gm, fs, dense, f"ssm_chain 4200 schedule {s}")
        dev.close()


def test_conveniences(hip_lib):
    model = cx.synth.lgssm_comb(15, d=3, teeth=1, seed=423)
    gm = E.gmodel(model)
    _mean, Sig, fpos = LS.dense_posterior(gm)
    dev = _dev(model, L.SCHED_TREE)
    free = gm.var_ids[~gm.obs]
    a, b = free[len(free) // 4], free[-1]               # a spine state and a tooth far from it: up a light edge and down another
    ia, ib = (int(fpos[np.searchsorted(gm.var_ids, v)]) for v in (a, b))
    d = 3
    want = Sig[ia * d:(ia + 1) * d, ib * d:(ib + 1) * d]
    sa, sb = np.sqrt(np.diag(Sig)[ia * d:(ia + 1) * d]), np.sqrt(np.diag(Sig)[ib * d:(ib + 1) * d])
    got = dev.posterior_covariance(a, b)
    assert np.max(np.abs(got - want) / np.outer(sa, sb)) <= F.REL_TOL
    one = np.ones(d)
    cv = one @ (Sig[ia * d:(ia + 1) * d, ia * d:(ia + 1) * d] + Sig[ib * d:(ib + 1) * d, ib * d:(ib + 1) * d] - want - want.T) @ one
    assert abs(dev.contrast_variance(a, b) - cv) <= F.REL_TOL * cv
    off, ids, w = F.as_csr([([a], np.eye(d)[:1]), ([b, a], np.ones((2, d)))], d)
    m1, c1, _ = dev.linear_moments((off, ids, w))
    m2, c2, _ = dev.linear_moments([([a], np.eye(d)[:1]), ([b, a], np.ones((2, d)))])
    assert np.array_equal(m1, m2) and np.array_equal(c1, c2)
    m3, c3, _ = dev.linear_moments((off, ids, w), cov=False)
    assert c3 is None and np.array_equal(m3, m1)
    dev.close()


def test_components_are_uncorrelated(hip_lib):
    model = cx.synth.tree_model(40, seed=360, observe=0.25, components=3)
    gm = E.gmodel(model)
    lab = _components(gm)
    dev = _dev(model, L.SCHED_TREE)
    labs = np.unique(lab[lab >= 0])
    va, vb = gm.var_ids[lab == labs[0]], gm.var_ids[lab == labs[1]]
    rng = np.random.default_rng(5)
    _, cov, cnt = dev.linear_moments([(va, rng.standard_normal((len(va), 1))), (vb, rng.standard_normal((len(vb), 1)))])
    assert cnt["components"] == 3 and cov[0, 1] == 0.0 and cov[1, 0] == 0.0 and cov[0, 0] > 0 and cov[1, 1] > 0
    dev.close()


@pytest.mark.parametrize("which", ["tree_model", "kary d=2"])
def test_adjoint_identity(hip_lib, which):
    """no solve: φ(sample(ε)) - mean is linear in ε, mean = φ(sample(0)), and Σ_e (φ_k(F e))² over the unit noise vectors = cov[k][k]"""
    if which == "tree_model":
        model = cx.synth.tree_model(12, seed=450, k_choices=(1, 2, 3, 4), observe=0.2)
        gm = E.gmodel(model)
        dev = _dev(model, L.SCHED_TREE)
    else:
        model, gm, load = F.kary_case(2, 442)
        dev = load(L.SCHED_TREE)
        dev.sweep(1)
    d, nv = gm.d, len(gm.var_ids)
    fs, _ = F.standard_functionals(gm, seed=3)
    W = F.weight_matrix(gm, fs)
    mean, cov, _ = dev.linear_moments(fs)
    x0, _ = dev.sample_posterior(1, noise=np.zeros((1, nv, d)))
    phi0 = np.einsum("kvi,vi->k", W, x0[0])
    sd = np.sqrt(np.diag(cov))
    assert np.max(np.abs(phi0 - mean) / sd) <= F.REL_TOL
    eps = SS.identity_noise(gm)
    x, _ = dev.sample_posterior(len(eps), noise=eps)
    Fe = np.einsum("kvi,svi->sk", W, x) - phi0[None]                 # row s: φ(F e_s)
    got = Fe.T @ Fe
    assert np.max(np.abs(got - cov) / np.outer(sd, sd)) <= F.REL_TOL
    rng = np.random.default_rng(9)
    e1, e2 = rng.standard_normal((2, 1, nv, d))
    p1, p2, p12 = (np.einsum("kvi,vi->k", W, dev.sample_posterior(1, noise=e)[0][0]) - phi0 for e in (e1, e2, 2.0 * e1 - 3.0 * e2))
    assert np.max(np.abs(p12 - (2.0 * p1 - 3.0 * p2)) / sd) <= 1e-12
    dev.close()


def test_independence_and_determinism(hip_lib, monkeypatch):
    model = cx.synth.lgssm_comb(15, d=2, teeth=1, seed=422)
    gm = E.gmodel(model)
    dev = _dev(model, L.SCHED_TREE)
    free = gm.var_ids[~gm.obs]
    rng = np.random.default_rng(11)
    fs = [(rng.choice(free, size=int(rng.integers(1, 9)), replace=False), rng.standard_normal((8, 2))) for _ in range(37)]
    fs = [(i, w[:len(i)]) for i, w in fs]
    mean, cov, _ = dev.linear_moments(fs)
    m2, c2, _ = dev.linear_moments(fs)
    assert np.array_equal(mean, m2) and np.array_equal(cov, c2)                       # bit-identical
    for k in (0, 17, 36):
        m1, c1, _ = dev.linear_moments([fs[k]])
        assert m1[0] == mean[k] and c1[0, 0] == cov[k, k], k                          # alone = among 37
    sub = [5, 30, 16]
    ms, cs, _ = dev.linear_moments([fs[k] for k in sub])
    assert np.array_equal(ms, mean[sub]) and np.array_equal(cs, cov[np.ix_(sub, sub)])
    monkeypatch.setenv("CX_FN_CHUNK", "19")                                            # two chunks: 19 + 18
    m3, c3, _ = dev.linear_moments(fs)
    assert np.array_equal(m3, mean) and np.array_equal(c3, cov)
    dev.close()


def test_undefined_component_is_nan(hip_lib):
    model = cx.synth.tree_model(40, seed=360, observe=0.25, components=3)
    gm = E.gmodel(model)
    dense = LS.dense_posterior(gm)
    lab = _components(gm)
    bad = lab == lab[np.flatnonzero(~gm.obs)[0]]
    good = (lab >= 0) & ~bad
    dev = cx.DeviceGraph(schedule=L.SCHED_REFERENCE)
    cx.synth.load_into_device(model, dev)
    dev.sweep_for(gm.var_ids[good])                     # the other components only: the messages of the first are never computed
    vb, vg = gm.var_ids[bad], gm.var_ids[good]
    fs = [([vg[0]], [[1.0]]), ([vb[0]], [[1.0]]), ([vg[1], vg[-1]], [[1.0], [-1.0]]), ([vg[2], vb[-1]], [[1.0], [1.0]]), (vg, np.ones((len(vg), 1)))]
    mean, cov, cnt = dev.linear_moments(fs)
    nanf = np.array([False, True, False, True, False])
    assert cnt == {"components": 3, "failed": 1, "nan_functionals": 2, "free": int((~gm.obs).sum())}, cnt
    assert np.isnan(mean[nanf]).all() and np.isnan(cov[nanf]).all() and np.isnan(cov[:, nanf]).all()
    ok = np.flatnonzero(~nanf)
    ref = F.dense_moments(gm, [fs[k] for k in ok], dense)
    em, ec = F.rel_errors(mean[ok], cov[np.ix_(ok, ok)], *ref)
    assert em <= F.REL_TOL and ec <= F.REL_TOL, (em, ec)
    dev.close()


def test_refusals(hip_lib):
    one = [([1], [[1.0]])]
    dev = _dev(cx.synth.gaussian_grid(6, 5, seed=371), L.SCHED_FUSED, 5)                             # a loopy graph
    code, msg = code_of(dev.linear_moments, one)
    assert code == L.ERR_UNSUPPORTED and "cx_linear_moments" in msg and "cycle" in msg and "variable" in msg, msg
    dev.close()
    dev = _dev(cx.synth.lgssm_chain(4, d=16, seed=370), L.SCHED_FUSED, 2)
    code, msg = code_of(dev.linear_moments, [([1], np.ones((1, 16)))])
    assert code == L.ERR_UNSUPPORTED and "cx_linear_moments" in msg                                  # dim >= 5
    dev.close()
    vm = cx.synth.vmp_ssm(8)
    dev = cx.DeviceGraph(schedule=L.SCHED_CHAIN_SCAN, family=L.FAMILY_VMP_STRUCTURED)
    cx.synth.load_vmp_into_device(vm, dev)
    assert code_of(dev.linear_moments, one)[0] == L.ERR_UNSUPPORTED
    dev.close()
    model = cx.synth.ssm_chain(20, seed=372)
    dev = _dev(model, L.SCHED_TREE)
    code, msg = code_of(dev.linear_moments, [([99999], [[1.0]])])
    assert code == L.ERR_NOT_FOUND and "99999" in msg and "cx_linear_moments" in msg
    off, ids, w = np.array([0, 2, 1], np.int64), np.array([1, 2], np.int64), np.ones((2, 1))
    assert code_of(dev.linear_moments, (off, ids, w))[0] == L.ERR_INVALID_ARGUMENT                     # offsets decrease
    assert code_of(dev.linear_moments, (np.array([1, 2], np.int64), ids, w))[0] == L.ERR_INVALID_ARGUMENT      # do not start at 0
    cnt = (C.c_int64 * 4)()
    off1 = np.array([0, 1], np.int64)
    po, pi, pw = off1.ctypes.data_as(C.POINTER(C.c_int64)), ids.ctypes.data_as(C.POINTER(C.c_int64)), w.ctypes.data_as(C.POINTER(C.c_double))
    out = np.zeros(1)
    pm = out.ctypes.data_as(C.POINTER(C.c_double))
    assert dev.lib.cx_linear_moments(dev.h, 1, po, pi, pw, None, None, cnt) == L.ERR_INVALID_ARGUMENT          # no mean
    assert dev.lib.cx_linear_moments(dev.h, -1, po, pi, pw, pm, None, cnt) == L.ERR_INVALID_ARGUMENT
    assert dev.lib.cx_linear_moments(dev.h, 1, None, pi, pw, pm, None, cnt) == L.ERR_INVALID_ARGUMENT
    assert dev.lib.cx_linear_moments(dev.h, 1, po, pi, None, pm, None, cnt) == L.ERR_INVALID_ARGUMENT
    assert dev.lib.cx_linear_moments(dev.h, 1, po, pi, pw, pm, None, cnt) == L.OK
    dev.halo_configure([1], [2 * 20 + 1], [], [])                                                    # a partitioned handle
    assert code_of(dev.linear_moments, one)[0] == L.ERR_UNSUPPORTED
    dev.close()
    model = cx.synth.ssm_chain(10, seed=373, q=0.0)
    dev = cx.DeviceGraph(schedule=L.SCHED_TREE)
    cx.synth.load_into_device(model, dev)
    code, msg = code_of(dev.linear_moments, one)
    assert code == L.ERR_UNSUPPORTED and "zero noise" in msg and "cx_linear_moments" in msg
    dev.close()


def test_sampler_is_unchanged_after_a_moments_call(hip_lib):
    """the two entries share one plan: a draw is the same before and after cx_linear_moments has used its buffers"""
    model = cx.synth.tree_model(60, seed=331, observe=0.2)
    dev = _dev(model, L.SCHED_TREE)
    x, _ = dev.sample_posterior(5, seed=7)
    free = np.setdiff1d(np.unique(model.edge_var), model.data_var)
    dev.linear_moments([(free[:9], np.ones((9, 1))), ([free[3]], [[1.0]])])
    assert np.array_equal(x, dev.sample_posterior(5, seed=7)[0])
    dev.close()


def test_cpp_host_class_linear_moments(hip_lib, tmp_path):
    out_lines = run_demo("functional_demo", tmp_path)
    rows = {line.split()[0]: [float(v) for v in line.split()[1:]] for line in out_lines}
    T = 50
    model = cx.synth.ssm_chain(T, seed=1)
    model.data_y = np.array([0.5 * t + (7 * t) % 5 for t in range(1, T + 1)], dtype=np.float64)
    gm = E.gmodel(model)
    fs = [([1, T], [[1.0], [-1.0]]), (np.arange(11, 31), np.full((20, 1), 1.0 / 20)), ([25, T + 25], [[1.0], [2.0]])]
    ref = F.dense_moments(gm, fs)
    em, ec = F.rel_errors(np.asarray(rows["mean"]), np.asarray(rows["cov"]).reshape(3, 3), *ref)
    assert em <= F.REL_TOL and ec <= F.REL_TOL, (em, ec)
    assert rows["mean_only"] == rows["mean"] and rows["counts"] == [1, 0, 0, T, 0]
