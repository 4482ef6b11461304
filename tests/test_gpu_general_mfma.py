"""-m gpu: cx_log_evidence_mfma, cx_factor_beliefs_mfma, cx_factor_statistics_mfma and cx_log_evidence_components_mfma (cx_create dim
5 .. 64) on GENERAL models — A non-normal, Q and R dense SPD, H neither symmetric nor the identity
(tests/general_mfma_support.py on tests/anisotropic.py).  The files of those calls run isotropic models, where every message is a multiple
of the identity, Cholesky factors are diagonal and the likelihood tables are P = B = B' = C = I / r: H' for H, a wrong triangle or a
dropped off-diagonal tile passes there.  tests/test_general_mfma_checker.py pins every input used here on the CPU and shows that such an
error moves these references by a thousand times the bounds below.

Bounds: those of tests/test_gpu_evidence_mfma.py, tests/test_gpu_learn_mfma.py and tests/test_gpu_evidence_components_mfma.py for the same
calls — log-evidence 1e-9 relative, belief means 1e-9, covariances and statistics 1e-9 max(1, max|want|), tile-size invariance 1e-12, the
formula on the device's own messages 1e-10, the M-step and the EM trace 1e-7."""
import dataclasses
import functools
import math

import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from cortex.jl_amd import learn
from tests import anisotropic as AN
from tests import components_support as CS
from tests import evidence_mfma_support as S
from tests import evidence_support as E
from tests import general_mfma_support as G
from tests import learn_mfma_support as LM
from tests import learning_support as LS
from tests import missing_data as MD
from tests.helpers import assert_close
from tests.learn_mfma_support import assert_within as _close
from tests.learn_mfma_support import bound_of as _scale

pytestmark = pytest.mark.gpu

SCHEDULES = {"tree": L.SCHED_TREE, "reference": L.SCHED_REFERENCE, "fused": L.SCHED_FUSED, "chain-scan": L.SCHED_CHAIN_SCAN}
FUSED_SWEEPS = 60      # seed variance 1e6; on a forest of diameter under 20 the result is exact whatever the seed


# ---- helpers (those of the three files named above) -----------------------------------------------------------------------------------
def _dev(model, schedule, sweeps=None, opaque=None, missing=False):
    fused = schedule == L.SCHED_FUSED
    dev = cx.DeviceGraph(dim=model.dim, schedule=schedule)
    if missing:
        MD.load(model, dev)                    # the flat message on the last state's one edge
    else:
        cx.synth.load_into_device(model, dev, seed_variance=1e6 if fused else None)
    if opaque is not None:
        S.set_opaque(dev, opaque)
    dev.sweep(sweeps if sweeps is not None else (FUSED_SWEEPS if fused else 1))
    return dev


def _n_rule_factors(gm):
    return sum(len(g["fid"]) for g in gm.groups.values())


def _set_groups(model, gm):
    sets = {int(f): int(s) for f, s in zip(*LS.pset_groups(model))}
    fids = gm.groups[2]["fid"]
    return fids, np.array([sets[int(f)] for f in fids])


class _Ref:
    """the dense references of one model, computed once and never changed"""

    def __init__(self, model, opaque=None, psets=None, n_groups=2):
        self.model, self.n_groups = model, n_groups
        self.gm = E.gmodel(model, opaque=opaque, psets=psets)
        self.log_z = E.dense_log_z(self.gm)
        self.fids, self.groups = _set_groups(model, self.gm)
        self.beliefs = LS.dense_factor_beliefs(self.gm, self.fids)
        self.stats = LS.grouped_statistics(self.gm, self.fids, self.groups, n_groups, beliefs=self.beliefs)


@functools.lru_cache(maxsize=None)
def _ref(kind, d):
    """kind: a builder of general_mfma_support; chain and comb carry a third, unused group"""
    built = getattr(G, kind)(d)
    model, opq = built if kind == "prior" else (built, None)
    if kind in ("chain", "comb", "velocity"):
        log_z = AN.joint_solve(model)[3]      # the reference the models were pinned against
        r = _Ref(model, n_groups=3 if kind != "velocity" else 2)
        r.log_z = log_z
        return r
    return _Ref(model, opaque=opq)


def _check_evidence(dev, want, what, rtol=1e-9):
    got, cnt = dev.log_evidence_mfma()
    print(f"{what} log-evidence: got {got!r} want {want!r} relative error {abs(got - want) / abs(want):.3e} (bound {rtol:.0e}) {cnt}")
    assert cnt["undefined"] == 0 and cnt["not_positive_definite"] == 0, (what, cnt)
    assert abs(got - want) <= rtol * abs(want), (what, got, want)
    return got, cnt


def _check_beliefs(dev, fids, want, what):
    got_m, got_c = dev.factor_beliefs_mfma(fids)
    _close(got_m, want[0], 1e-9, what + " belief means")
    _close(got_c, want[1], _scale(want[1]), what + " belief covariances")
    return got_m, got_c


def _check_stats(dev, want, n_groups, n_counted, n_groups_used, what):
    got, cnt = dev.factor_statistics_mfma(n_groups=n_groups)
    for k in LS.KEYS:
        _close(got[k], want[k], _scale(want[k]), f"{what} {k}")
    assert cnt == {"factors": n_counted, "groups": n_groups_used, "undefined": 0, "not_positive_definite": 0}, (what, cnt)
    assert np.array_equal(got["n"], want["n"]), (what, got["n"])
    return got


def _check_all(dev, r, what, n_variable_terms=None):
    """the three calls of one handle against the references of r; returns what they gave"""
    z, cnt = _check_evidence(dev, r.log_z, what)
    assert cnt["factor_terms"] == _n_rule_factors(r.gm), (what, cnt)
    if n_variable_terms is not None:
        assert cnt["variable_terms"] == n_variable_terms, (what, cnt)
    b = _check_beliefs(dev, r.fids, r.beliefs, what)
    s = _check_stats(dev, r.stats, r.n_groups, len(r.fids), 2, what)
    return z, b, s


# ---- 1. every schedule, every tile size ------------------------------------------------------------------------------------------------
CASES_1 = [(d, shape, s) for d in G.DIMS for shape in ("chain", "comb") for s in SCHEDULES if shape == "chain" or s != "chain-scan"]


@pytest.mark.parametrize("d,shape,sched", CASES_1, ids=[f"d{d}-{shape}-{s}" for d, shape, s in CASES_1])
def test_every_schedule_every_tile_size(hip_lib, d, shape, sched):
    r = _ref(shape, d)
    model = r.model
    what = f"d {d} {shape} {sched}"
    dev = _dev(model, SCHEDULES[sched])
    _, _, got = _check_all(dev, r, what, n_variable_terms=len(model.x_ids))      # every state has two or three factors
    assert got["n"][2] == 0 and not any(np.any(got[k][2]) for k in LS.KEYS)      # set 2 unused: a zero row
    # the M-step against one written out in numpy: A alone, then Q alone (five factors do not determine both at d = 64); for set 1 this
    # is the M-step of H and R
    for k in (0, 1):
        A = np.asarray(model.psets[k][0], float)
        want_k = {key: v[k] for key, v in r.stats.items()}
        wantA, wantQ = LM.numpy_m_step(want_k, A, learn=("A",))[0], LM.numpy_m_step(want_k, A, learn=())[1]
        _close(learn.m_step(learn.group(got, k), A, learn=("A",))["A"], wantA, 1e-7 * max(1.0, float(np.max(np.abs(wantA)))), f"{what} M-step A of set {k}")
        _close(learn.m_step(learn.group(got, k), A, learn=("Q",))["Q"], wantQ, 1e-7 * max(1.0, float(np.max(np.abs(wantQ)))), f"{what} M-step Q of set {k}")
    dev.close()


# ---- 2. gaps and a forecast tail, a prior, a clamped state -----------------------------------------------------------------------------
@pytest.mark.parametrize("d", G.GEN_DIMS)
def test_gaps_and_a_forecast_tail(hip_lib, d):
    r = _ref("gen", d)
    dev = _dev(r.model, L.SCHED_TREE, missing=True)
    _check_all(dev, r, f"gen d {d}")
    dev.close()


@pytest.mark.parametrize("sched", ["tree", "fused"])
@pytest.mark.parametrize("d", G.PRIOR_DIMS)
def test_dense_opaque_prior(hip_lib, d, sched):
    r = _ref("prior", d)
    dev = _dev(r.model, SCHEDULES[sched], opaque=G.prior(d)[1])
    _check_all(dev, r, f"prior d {d} {sched}")
    dev.close()


@pytest.mark.parametrize("sched", ["tree", "fused"])
@pytest.mark.parametrize("d", G.CLAMPED_DIMS)
def test_an_observed_state_in_the_middle(hip_lib, d, sched):
    # a factor with both ends observed, one with its OUT end observed (J = -A) and one with its IN end observed (eta' = B y), A and H general
    r = _ref("clamped", d)
    dev = _dev(r.model, SCHEDULES[sched])
    _, (_, got_c), _ = _check_all(dev, r, f"clamped d {d} {sched}", n_variable_terms=len(r.model.x_ids) - 1)
    obs = r.gm.obs[r.gm.groups[2]["vars"]]
    assert obs.sum() > len(r.model.x_ids)
    for row in range(len(r.fids)):      # zero rows and columns on the observed ends, exactly
        for e in range(2):
            if obs[row, e]:
                assert not np.any(got_c[row, e * d:(e + 1) * d, :]) and not np.any(got_c[row, :, e * d:(e + 1) * d])
    dev.close()


# ---- 3. a loop ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", G.RING_DIMS)
def test_loop_matches_the_restatement_on_the_device_messages(hip_lib, d):
    model = G.ring(d)
    gm = E.gmodel(model)
    fids, groups = _set_groups(model, gm)
    dev = _dev(model, L.SCHED_FUSED, G.RING_SWEEPS)
    f2v, opq = E.device_messages(gm, dev)
    want, exact = E.bethe_log_z(gm, f2v, opq), E.dense_log_z(gm)
    got, cnt = _check_evidence(dev, want, f"ring d {d} (exact {exact!r})", rtol=1e-10)
    assert cnt["factor_terms"] == 2 * G.RING_T and cnt["variable_terms"] == G.RING_T
    assert abs(got - exact) > 1e-6 * abs(exact), (got, exact)             # the Bethe estimate, not the exact value
    want_m, want_c, status = LM.beliefs(gm, f2v, opq, fids=fids)
    assert np.all(status == LM.OK)
    _check_beliefs(dev, fids, (want_m, want_c), f"ring d {d}")
    _check_stats(dev, LM.statistics(gm, f2v, fids, groups, 2, opq)[0], 2, len(fids), 2, f"ring d {d}")
    dev.close()


# ---- 4. components ---------------------------------------------------------------------------------------------------------------------
def _components(dev, what):
    """values and per-component counts; their sum against log_evidence_mfma"""
    total, cnt = dev.log_evidence_mfma()
    values, cc, counts = dev.log_evidence_components_mfma()
    assert counts == cnt and [int(x) for x in cc.sum(axis=0)] == list(cnt.values()), (what, counts, cnt, cc.sum(axis=0))
    assert cc[:, 2:].sum() == 0 and np.isfinite(values).all(), (what, values, cc)
    gap, scale = abs(math.fsum(values.tolist()) - total), float(np.abs(values).sum())
    print(f"{what}: |fsum(values) - log_evidence_mfma| = {gap:.3e}, sum |values| = {scale:.6e}, relative {gap / scale:.3e} (bound 1e-12)")
    assert gap <= 1e-12 * scale, (what, gap, scale)
    return values, cc


@functools.lru_cache(maxsize=None)
def _parts_wants(d):
    return tuple(E.dense_log_z(E.gmodel(p)) for p in G.parts(d)[0])


@pytest.mark.parametrize("sched", ["chain-scan", "tree", "reference", "fused"])
@pytest.mark.parametrize("d", G.DIMS_C)
def test_chains_exact_per_component(hip_lib, d, sched):
    _, model = G.parts(d)
    _, lab, n = CS.labels(model)
    assert n == len(G.LENGTHS)
    dev = _dev(model, SCHEDULES[sched], 2 * max(G.LENGTHS) + 40 if sched == "fused" else 1)
    got_lab, got_n = dev.components()
    assert got_n == n and (got_lab == lab).all()
    values, cc = _components(dev, f"parts d {d} {sched}")
    for k, want in enumerate(_parts_wants(d)):
        print(f"parts d {d} {sched} component {k}: got {values[k]!r} want {want!r} relative error {abs(values[k] - want) / abs(want):.3e} (bound 1e-9)")
        assert abs(want) >= 1
        assert abs(values[k] - want) <= 1e-9 * abs(want), (d, sched, k, values[k], want)
    assert [int(x) for x in cc[:, 0]] == [2 * T - 1 for T in G.LENGTHS] and [int(x) for x in cc[:, 1]] == list(G.LENGTHS)
    dev.close()


@pytest.mark.parametrize("relabelled", [False, True], ids=["as-built", "relabelled"])
@pytest.mark.parametrize("d", G.FOREST_DIMS)
def test_forest_as_built_and_relabelled(hip_lib, d, relabelled):
    m = G.forest_relabelled(d) if relabelled else G.forest(d)
    gm = E.gmodel(m)
    lab, n = CS.gm_labels(gm)
    assert n == 3 and (lab == CS.labels(m)[1]).all()
    dev = _dev(m, L.SCHED_TREE)
    got_lab, got_n = dev.components()
    assert got_n == n and (got_lab == lab).all()
    values, cc = _components(dev, f"forest d {d}")
    for k in range(n):
        want = E.dense_log_z(CS.restrict(gm, k, lab))
        print(f"forest d {d} component {k}: got {values[k]!r} want {want!r} relative error {abs(values[k] - want) / abs(want):.3e} (bound 1e-9)")
        assert abs(want) >= 1
        assert abs(values[k] - want) <= 1e-9 * abs(want), (d, k, values[k], want)
    assert cc[:, 0].sum() == _n_rule_factors(gm)
    dev.close()


# ---- 5. embedded dims: blockdiag(H, I) / blockdiag(R, I) ---------------------------------------------------------------------------------
@pytest.mark.parametrize("d", G.EMBEDDED_DIMS)
def test_embedded_dims_give_the_real_models_values_at_any_tile_size(hip_lib, d, monkeypatch):
    r = _ref("chain", d)
    dev = _dev(r.model, L.SCHED_TREE)
    nat_z, nat_b, nat_s = _check_all(dev, r, f"d {d}, native tile")
    dev.close()
    monkeypatch.setenv("CX_MFMA_DIM", "64")
    dev = _dev(r.model, L.SCHED_TREE)
    monkeypatch.delenv("CX_MFMA_DIM")
    for_z, for_b, for_s = _check_all(dev, r, f"d {d}, 4 x 4 tiles")
    dev.close()
    print(f"d {d} forced against native, log-evidence: relative {abs(for_z - nat_z) / abs(nat_z):.3e} (bound 1e-12)")
    assert abs(for_z - nat_z) <= 1e-12 * abs(nat_z), (for_z, nat_z)
    for a, b, what in [(for_b[0], nat_b[0], "means"), (for_b[1], nat_b[1], "covariances")] + [(for_s[k], nat_s[k], k) for k in LS.KEYS]:
        _close(a, b, 1e-12 * max(1.0, float(np.max(np.abs(b)))), f"d {d} forced against native, {what}")


# ---- 6. new likelihood parameters, then new transition parameters, on one handle ----------------------------------------------------------
@pytest.mark.parametrize("d", G.SET_CHANGE_DIMS)
def test_new_parameters_of_either_set_on_one_handle(hip_lib, d):
    r = _ref("chain", d)
    model = r.model
    A2, Q2, R2, H2 = G.second_sets(d)
    dev = _dev(model, L.SCHED_TREE)
    first = _check_all(dev, r, f"d {d} old sets")
    psets = dict(model.psets)
    last = first
    for k, pair in ((1, (H2, R2)), (0, (A2, Q2))):      # the rule table, [A | A'] and the log-det table of THAT set follow
        dev.set_factor_matrices(k, *pair)
        dev.sweep(1)
        psets[k] = pair
        rk = _Ref(model, psets=dict(psets), n_groups=3)
        rk.log_z = AN.joint_solve(_with_psets(model, psets))[3]
        now = _check_all(dev, rk, f"d {d} new set {k}")
        assert abs(now[0] - last[0]) > 1e-3 and np.max(np.abs(now[1][0] - last[1][0])) > 1e-3 and np.max(np.abs(now[2]["S_rr"][k] - last[2]["S_rr"][k])) > 1e-3
        last = now
    dev.close()


def _with_psets(model, psets):
    return dataclasses.replace(model, psets=dict(psets))


# ---- 7. EM at an embedded tile ---------------------------------------------------------------------------------------------------------
def test_em_matches_shumway_stoffer_on_a_general_chain(hip_lib):
    model, A0, Q0, C0, R0 = G.em_case()
    d, n_iter = G.EM_D, G.EM_ITER
    y = np.asarray(model.data_y).reshape(G.EM_T, d)
    want_trace, want_params = LS.ss_em(y, A0, Q0, C0, R0, n_iter=n_iter)
    dev = cx.DeviceGraph(dim=d, schedule=L.SCHED_CHAIN_SCAN)
    cx.synth.load_into_device(model, dev)
    trace, params = learn.em(dev, {0: (A0, Q0), 1: (C0, R0)}, n_iter=n_iter, learn=("A", "Q"))
    print("trace", trace, "want", want_trace)
    assert np.all(np.diff(trace) >= -1e-9 * abs(trace[-1])), np.diff(trace)
    got, want = np.asarray(trace), np.asarray(want_trace)
    err = float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1.0)))
    print(f"d {d} EM trace: max relative error {err:.3e} (bound 1e-7)")
    assert err <= 1e-7, err
    for s, (wa, wq) in ((0, want_params[-1][:2]), (1, want_params[-1][2:])):
        _close(params[s][0], wa, 1e-7 * max(1.0, float(np.max(np.abs(wa)))), f"EM final matrix of set {s}")
        _close(params[s][1], wq, 1e-7 * max(1.0, float(np.max(np.abs(wq)))), f"EM final covariance of set {s}")
    dev.close()


# ---- 8. rank-deficient H ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sched", ["tree", "chain-scan"])
@pytest.mark.parametrize("d", G.VELOCITY_DIMS)
def test_rank_deficient_observation_matrix(hip_lib, d, sched):
    """positions observed, velocities not: every likelihood message has the singular precision H' R^-1 H, improper alone and proper once
    a neighbour's message is added.  tests/test_gpu_anisotropic.py runs this at dim 2 and 4"""
    r = _ref("velocity", d)
    model, n = r.model, len(r.model.x_ids)
    what = f"velocity d {d} {sched}"
    dev = _dev(model, SCHEDULES[sched])
    em, ecov = AN.chain_posterior(model)
    marg = dev.get_marginals(model.x_ids)
    assert not np.any(np.isnan(marg)), f"{what}: undefined marginals"
    for name, got, want in (("means", marg[:, :d], em), ("covariances", marg[:, d:].reshape(n, d, d), ecov)):
        err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
        print(f"{what}: marginal {name}: largest error {err:.3e} of the largest entry (bound 1e-9)")
        assert_close(got, want, 1e-9, f"{what} marginal {name}", scale_by="max")
    _check_all(dev, r, what, n_variable_terms=n)
    dev.close()
