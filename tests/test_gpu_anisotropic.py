"""-m gpu: every d-dimensional kernel family on GENERAL matrices (tests/anisotropic.py): A non-normal, Q and R dense SPD, H neither
symmetric nor the identity — the models whose Cholesky factors are not diagonal, whose A S A' differs from A' S A and whose packed
symmetric records differ between the triangles.  The rest of the suite runs isotropic models; tests/test_anisotropic_checkers.py
shows on the CPU that a transposed rule passes there and fails here, and pins the references used below on these models.

Tolerances are the project's: 1e-8 per sweep and 1e-9 at the fixed point for d <= 4, 1e-7 and 1e-8 on the matrix cores, the readers at
their support modules' constants.  The models are benign (cond <= 20, the f64 references good to 2e-15)."""
import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from oracle.mv import MvFlood, MvFloodC
from tests import anisotropic as AN
from tests import evidence_support as E
from tests import functional_support as F
from tests import learning_support as LS
from tests import predictive_support as P
from tests import sampling_support as SS
from tests.helpers import assert_close_by_max as assert_close
from tests.learning_support import assert_rel_close as _close

pytestmark = pytest.mark.gpu


def _tols(d):
    """(per sweep, fixed point)"""
    return (1e-8, 1e-9) if d <= 4 else (1e-7, 1e-8)


def _dev(model, schedule=L.SCHED_FUSED, seed_variance=None, **kw):
    dev = cx.DeviceGraph(dim=model.dim, schedule=schedule, **kw)
    cx.synth.load_into_device(model, dev, seed_variance)
    return dev


def _per_sweep(dev, o, model, sweeps, tol, what):
    """`sweeps` sweeps of the device and of the restatement o (MvFlood or MvFloodC) side by side: every message into a latent variable,
    the same ones defined; improper messages (none on a full-rank H) skipped as the isotropic tests skip them"""
    d, g = model.dim, o.g
    pe = AN.latent_edges(g, model)
    for sweep in range(sweeps):
        dev.sweep(1)
        o.sweep(1)
        got = dev.get_messages(g.edge_var[pe], g.edge_fac[pe], L.TO_VARIABLE)
        for row, e in zip(got, pe):
            if o.f2v[e] is None:
                assert np.all(np.isnan(row)), f"{what} sweep {sweep} edge {e}: device defined, restatement undefined"
                continue
            m, S = o.f2v[e]
            if not np.all(np.isfinite(S)) or np.linalg.cond(S) > 1e10:
                continue
            assert_close(row[:d], m, tol, f"{what} sweep {sweep} f2v mean edge {e}")
            assert_close(row[d:].reshape(d, d), S, tol, f"{what} sweep {sweep} f2v covariance edge {e}")


# ---- flooding-order sweeps, d = 2, 3, 4 (dim > 1 has one iterative schedule, CX_SCHED_FUSED; cx_create refuses CX_SCHED_FLOODING) ----------
@pytest.mark.parametrize("d", [2, 3, 4])
def test_sweeps_on_a_general_chain(hip_lib, d):
    T = 40
    model = AN.chain(T, d)
    dev = _dev(model)
    _per_sweep(dev, MvFloodC(model), model, 8, 1e-8, f"d={d}")
    dev.sweep(T + 3 - 8)
    AN.check_marginals(dev, model, AN.dense_posterior(model), 1e-9, f"d={d} fixed point vs the joint solve")
    dev.residual()
    dev.sweep(2)
    assert dev.residual() < 1e-10


@pytest.mark.parametrize("name,make,total", [("branching b=9 d=3", lambda: AN.branching(91, 3, b=9), 10),
                                             ("multi-sensor d=4", lambda: AN.multi_sensor(12, 4, sensors=3), 16)])
def test_sweeps_with_variables_of_high_degree(hip_lib, name, make, total):
    """inner states of degree 11 (the CSR tail of the slot space: k_big_mv) and a chain of degree-5 states"""
    model = make()
    dev = _dev(model)
    o = MvFloodC(model)
    assert np.diff(o.g.var_off).max() == (11 if "branching" in name else 5)
    _per_sweep(dev, o, model, 6, 1e-8, name)
    dev.sweep(total - 6)
    AN.check_marginals(dev, model, AN.dense_posterior(model), 1e-9, name + " fixed point vs the joint solve")


# ---- chain scan, d = 2, 3, 4 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("general_h", [True, False], ids=["H", "H=I"])
@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("T", [2, 9, 700])
@pytest.mark.parametrize("d", [2, 3, 4])
def test_chain_scan_one_sweep(hip_lib, monkeypatch, d, T, K, general_h):
    monkeypatch.setenv("CX_MVC_K", str(K))
    model = AN.chain(T, d, general_h=general_h)
    dev = _dev(model, L.SCHED_CHAIN_SCAN)
    dev.sweep(1)
    marg = AN.check_marginals(dev, model, AN.chain_posterior(model), 1e-9, f"d={d} T={T} K={K}")
    lazy = _dev(model, L.SCHED_CHAIN_SCAN, marginals_in_sweep=2)
    lazy.sweep(1)
    assert np.array_equal(marg, lazy.get_marginals(model.x_ids)), "marginals on demand: the same bits"


# ---- matrix cores: flooding --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,form", [(7, ""), (16, ""), (20, ""), (32, ""), (33, ""), (64, "w"), (64, "g")])
def test_matrix_core_sweeps_on_a_general_chain(hip_lib, monkeypatch, d, form):
    T = 7
    if form:
        monkeypatch.setenv("CX_RULE64", form)
    model = AN.chain(T, d)
    dev = _dev(model)
    o = MvFlood(model)
    o.sweep(1)            # the matrix-core path evaluates the messages out of observed variables at data injection
    _per_sweep(dev, o, model, T + 1, 1e-7, f"d={d}")
    dev.sweep(2)
    AN.check_marginals(dev, model, AN.chain_posterior(model), 1e-8, f"d={d} fixed point")


@pytest.mark.parametrize("d", [16, 24])
def test_native_tiles_equal_the_embedding_in_64_on_a_general_chain(hip_lib, monkeypatch, d):
    T = 7
    model = AN.chain(T, d)
    a = _dev(model)
    monkeypatch.setenv("CX_MFMA_DIM", "64")
    b = _dev(model)
    monkeypatch.delenv("CX_MFMA_DIM")
    xs = set(int(v) for v in model.x_ids)
    keep = np.array([int(v) in xs for v in model.edge_var])
    ev, ef = model.edge_var[keep], model.edge_fac[keep]
    for sweep in range(T + 2):
        a.sweep(1); b.sweep(1)
        ma, mb = a.get_messages(ev, ef, L.TO_VARIABLE, L.FORM_NATURAL), b.get_messages(ev, ef, L.TO_VARIABLE, L.FORM_NATURAL)
        assert np.array_equal(np.isnan(ma), np.isnan(mb)), f"sweep {sweep}"
        ok = ~np.isnan(ma)
        assert_close(ma[ok], mb[ok], 1e-9, f"d={d} sweep {sweep}: messages, native tiles vs embedded")
    assert_close(a.get_marginals(model.x_ids), b.get_marginals(model.x_ids), 1e-9, f"d={d}: marginals, native tiles vs embedded")
    AN.check_marginals(a, model, AN.chain_posterior(model), 1e-8, f"d={d} native tiles")


# ---- matrix cores: chain scan ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,T,K,fan", [(7, 9, 0, 0), (16, 9, 0, 0), (32, 9, 0, 0), (64, 9, 0, 0), (64, 40, 3, 3)])
def test_matrix_core_chain_scan_one_sweep(hip_lib, monkeypatch, d, T, K, fan):
    if K:
        monkeypatch.setenv("CX_MVC64_K", str(K))
        monkeypatch.setenv("CX_MVC64_FAN", str(fan))
    model = AN.chain(T, d)
    dev = _dev(model, L.SCHED_CHAIN_SCAN)
    dev.sweep(1)
    AN.check_marginals(dev, model, AN.chain_posterior(model), 1e-8, f"d={d} T={T}")
    if K:
        assert dev.chain_plan_stats()["levels"] >= 2


# ---- tree schedule -----------------------------------------------------------------------------------------------------------------------
TREES = [(f"comb {n} x {t} d={d}", (lambda d=d, n=n, t=t: AN.comb(n, d, teeth=t))) for d, n, t in AN.TREE_COMBS] + \
        [(f"branching {n} b={b} d={d}", (lambda d=d, b=b, n=n: AN.branching(n, d, b=b))) for d, b, n in AN.TREE_BRANCHING]


@pytest.mark.parametrize("heavy_paths", ["0", "1"])
@pytest.mark.parametrize("name,make", TREES, ids=[t[0] for t in TREES])
def test_tree_schedule_one_sweep(hip_lib, monkeypatch, name, make, heavy_paths):
    monkeypatch.setenv("CX_TREE_HP", heavy_paths)
    model = make()
    dev = _dev(model, L.SCHED_TREE)
    dev.sweep(1)
    launches = dev.tree_heavy_path_stats()["launches"]
    assert launches == 0 if heavy_paths == "0" else (launches > 0 or "comb" not in name)
    AN.check_marginals(dev, model, AN.dense_posterior(model), _tols(model.dim)[1], f"{name} heavy paths {heavy_paths}")


# ---- reference order ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 4, 64])
def test_reference_order_one_call_on_a_general_chain(hip_lib, d):
    T = 60
    model = AN.chain(T, d)
    dev = _dev(model, L.SCHED_REFERENCE)
    dev.sweep(1)
    st = dev.ref_plan_stats()
    assert st["messages"] == 5 * T - 4 and st["executions"] == 6 * T - 4
    AN.check_marginals(dev, model, AN.chain_posterior(model), _tols(d)[1], f"d={d} reference order")


@pytest.mark.parametrize("d,T,skips", AN.REF_LOOPY)
def test_reference_order_two_calls_on_a_general_loopy_graph(hip_lib, d, T, skips):
    from tests.test_gpu_reference_mv import check_calls_on_a_loopy_graph

    check_calls_on_a_loopy_graph(AN.loopy(T, d, skips=skips), 2)


# ---- loopy fused sweep -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 4])
def test_fused_sweeps_on_a_general_loopy_graph(hip_lib, d):
    """every state on cycles, two different transition sets; seeded like the reference order's loopy cases.  Six sweeps message by
    message, then the fixed point (the C checker alone reaches it in AN.LOOPY_SWEEPS sweeps: tests/test_anisotropic_checkers.py), where
    the MEANS of Gaussian BP are exact"""
    model = AN.loopy(AN.LOOPY_T, d, skips=AN.LOOPY_SKIPS)
    dev = _dev(model, seed_variance=AN.LOOPY_SEED_VARIANCE)
    o = MvFloodC(model)
    o.seed(0.0, AN.LOOPY_SEED_VARIANCE)
    _per_sweep(dev, o, model, 6, 1e-8, f"loopy d={d}")
    dev.sweep(AN.LOOPY_SWEEPS - 6)
    dev.residual()
    dev.sweep(2)
    assert dev.residual() < 1e-10
    em, _ = AN.dense_posterior(model)
    marg = dev.get_marginals(model.x_ids)
    assert_close(marg[:, :d], em, 1e-9, f"loopy d={d}: means at the fixed point vs the joint solve")
    o.sweep(AN.LOOPY_SWEEPS - 4)
    mm, SS_, ok = o.marginals()
    xi = np.searchsorted(o.g.var_ids, model.x_ids)
    assert_close(marg[:, d:].reshape(-1, d, d), SS_[xi], 1e-9, f"loopy d={d}: covariances at the fixed point vs the C checker's")


# ---- readers -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reader_case():
    """per (d, shape): the model, its GModel and every reference number, computed once and left unchanged"""
    cache = {}

    def get(d, shape):
        if (d, shape) not in cache:
            model = AN.chain(60, d) if shape == "chain" else AN.comb(15, d, teeth=1)
            gm = E.gmodel(model)
            fids, sets = LS.pset_groups(model)
            T = len(model.x_ids)
            a, k = model.x_ids[T // 3], 3
            eye = np.eye(d)
            window = (model.x_ids[5:15], np.full((10, d), 0.1))
            fs = [window] + [([a], eye[i:i + 1]) for i in range(d)] + [([model.x_ids[T // 3 + k]], eye[i:i + 1]) for i in range(d)]
            f2v = F.forest_bp(gm)
            cache[(d, shape)] = dict(model=model, gm=gm, log_z=AN.joint_solve(model)[3], dense=LS.dense_posterior(gm),
                                     beliefs=LS.dense_factor_beliefs(gm), stats=LS.grouped_statistics(gm, fids, sets, 2), n_factors=len(fids),
                                     loo=P.dense_loo_all(gm), causal=P.predictive_from_messages(gm, f2v, mode=P.CAUSAL),
                                     functionals=fs, moments=F.dense_moments(gm, fs))
        return cache[(d, shape)]
    return get


SCHEDULES = {"tree": L.SCHED_TREE, "reference": L.SCHED_REFERENCE, "fused": L.SCHED_FUSED, "chain-scan": L.SCHED_CHAIN_SCAN}
READERS = [(d, shape, s) for d in (2, 3, 4) for shape in ("chain", "comb") for s in SCHEDULES if shape == "chain" or s != "chain-scan"]


@pytest.mark.parametrize("d,shape,sched", READERS, ids=[f"d{d}-{shape}-{s}" for d, shape, s in READERS])
def test_readers_on_general_models(hip_lib, reader_case, d, shape, sched):
    """log_evidence, factor_beliefs, factor_statistics, predictive (both modes), sample_posterior and linear_moments from the messages each
    schedule leaves, against the dense numbers of the support modules (pinned on these models against the joint solve on the CPU)"""
    schedule = SCHEDULES[sched]
    c = reader_case(d, shape)
    model, gm = c["model"], c["gm"]
    what = f"d={d} {shape} {sched}"
    fused = schedule == L.SCHED_FUSED
    dev = _dev(model, schedule, seed_variance=1e6 if fused else None)
    dev.sweep(200 if fused else 1)
    # evidence (test_gpu_evidence.py: 1e-9 relative)
    got, cnt = dev.log_evidence()
    assert cnt["undefined"] == 0 and cnt["not_positive_definite"] == 0, (what, cnt)
    assert abs(got - c["log_z"]) <= 1e-9 * abs(c["log_z"]), (what, got, c["log_z"])
    # factor beliefs and EM statistics (test_gpu_factor_statistics.py: 1e-9, matrices by their largest entry)
    fids = gm.groups[2]["fid"]
    gm_, gc_ = dev.factor_beliefs(fids)
    wm, wc = c["beliefs"]
    _close(gm_, wm, 1e-9, what + " belief means")
    _close(gc_, wc, 1e-9 * max(1.0, float(np.max(np.abs(wc)))), what + " belief covariances")
    st, scnt = dev.factor_statistics(n_groups=2)
    for key in LS.KEYS:
        scale = max(1.0, float(np.max(np.abs(c["stats"][key])))) if key in ("S_xx", "sum_x") else 1.0
        _close(st[key], c["stats"][key], 1e-9 * scale, f"{what} {key}")
    assert scnt == {"factors": c["n_factors"], "groups": 2, "undefined": 0, "not_positive_definite": 0}, (what, scnt)
    # predictive rows (test_gpu_predictive.py: EXACT = 1e-9)
    P.assert_rows_close(dev.predictive("loo"), c["loo"], 1e-9, what + " loo")
    P.assert_rows_close(dev.predictive("causal"), c["causal"], 1e-9, what + " causal")
    if fused:
        return          # (the samplers and the functionals read forests from the exact schedules)
    # samples (test_gpu_posterior_samples.py: 1e-9)
    mean, Sig, _ = c["dense"]
    nv = len(gm.var_ids)
    x0, scnt = dev.sample_posterior(1, noise=np.zeros((1, nv, d)))
    _close(x0[0], mean, 1e-9, what + " sample mean")
    assert scnt["undefined"] == 0 and scnt["not_positive_definite"] == 0, (what, scnt)
    eps = SS.identity_noise(gm)
    x, _ = dev.sample_posterior(len(eps), noise=eps)
    B = SS.samples_to_b(x, mean, gm)
    assert np.max(np.abs(B @ B.T - Sig)) <= 1e-9 * np.max(np.abs(Sig)), what + " B B'"
    # linear functionals: a window mean and the lag-3 cross covariance (functional_support.REL_TOL)
    fm, fc, fcnt = dev.linear_moments(c["functionals"])
    em, ec = F.rel_errors(fm, fc, *c["moments"])
    assert fcnt["failed"] == 0 and em <= F.REL_TOL and ec <= F.REL_TOL, (what, em, ec, fcnt)
    lag = fc[1:1 + d, 1 + d:]
    assert np.max(np.abs(lag)) > 1e-3 * np.max(np.abs(fc)) and not np.allclose(lag, lag.T, rtol=1e-3), "the lag-3 cross covariance is a general matrix"
    dev.close()


# ---- rank-deficient observation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", [L.SCHED_FUSED, L.SCHED_CHAIN_SCAN, L.SCHED_TREE], ids=["fused", "chain-scan", "tree"])
@pytest.mark.parametrize("d", [2, 4])
def test_rank_deficient_observation_matrix(hip_lib, d, schedule):
    """constant-velocity model, positions observed: H has zero rows for the velocities, so every likelihood message has the singular
    precision H' R^-1 H — improper alone, proper once a neighbour's message is added (natural form: nothing inverts it alone).  The
    marginals equal the exact smoother under every schedule."""
    T = 12
    model = AN.velocity_chain(T, d)
    dev = _dev(model, schedule)
    dev.sweep(T + 3 if schedule == L.SCHED_FUSED else 1)
    AN.check_marginals(dev, model, AN.chain_posterior(model), 1e-9, f"d={d} schedule {schedule}")
