"""-m gpu: cx_set_factor_offsets — x_out = A x_in + b + N(0, Q) at dim 2, 3, 4, a b per factor — under every schedule and through every
reader, on the general models of tests/anisotropic.py at the sizes tests/test_gpu_anisotropic.py found to reach each kernel path.

References: the joint solve with offsets and the GModel with offsets (tests/offsets_support.py, pinned against each other on the CPU in
tests/test_offsets_checker.py), and device against device through the shift equivalence: with b_a = s_out - A s_in the model is the
zero-offset model in x' = x - s, so every message obeys Lambda' = Lambda, eta' = eta - Lambda s after every sweep.
Tolerances are those of tests/test_gpu_anisotropic.py for the same models: 1e-8 per sweep, 1e-9 at a fixed point, the readers at their
support modules' constants; the batch items against the closed formulas at 1e-10.

The dim > 1 chain scan refuses a chain with a forecast tail (tests/test_gpu_missing_data.py pins that): the tail with offsets runs under
the tree schedule here, the chain with unobserved states under the chain scan."""
import dataclasses

import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from cortex.jl_amd import learn
from tests import anisotropic as AN
from tests import evidence_support as E
from tests import learning_support as LS
from tests import missing_data as MD
from tests import offsets_support as O
from tests import predictive_support as P
from tests.helpers import assert_close_by_max as assert_close
from tests.gpu_support import code_of, run_demo
from tests.learning_support import assert_rel_close as _close

pytestmark = pytest.mark.gpu


def _dev(model, schedule=L.SCHED_FUSED, b=None, seed_variance=None, loader=None, **kw):
    dev = cx.DeviceGraph(dim=model.dim, schedule=schedule, **kw)
    if loader is None:
        cx.synth.load_into_device(model, dev, seed_variance)
    else:
        loader(model, dev)
    if b is not None:
        dev.set_factor_offsets(*O.arrays(b))
    return dev


def _chain_case(d, T, general_h=True):
    def make():
        model = AN.chain(T, d, general_h=general_h)
        b = O.with_offsets(model, 1)
        return model, b, O.dense_posterior_offsets(model, b)
    return O.ref(("chain", d, T, general_h), make)


# ---- 1. fused sweeps on a chain -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 3, 4])
def test_fused_sweeps_on_a_chain_with_offsets(hip_lib, d):
    T = 40
    model, b, ref = _chain_case(d, T)
    dev, plain = _dev(model, b=b), _dev(model)
    dev.sweep(T + 3)
    plain.sweep(T + 3)
    marg = AN.check_marginals(dev, model, ref, 1e-9, f"d={d} fixed point vs the joint solve with offsets")
    # the offsets move no precision: the precision part of every message into a latent variable is the no-offset handle's, bit for bit
    ma, mp = O.messages(dev, model), O.messages(plain, model)
    assert np.array_equal(np.isnan(ma), np.isnan(mp))
    assert np.array_equal(ma[:, d:], mp[:, d:], equal_nan=True), "precisions differ from the handle without offsets"
    assert np.nanmax(np.abs(ma[:, :d] - mp[:, :d])) > 0.1, "the offsets did not reach the messages"
    pm = plain.get_marginals(model.x_ids)
    assert np.array_equal(marg[:, d:], pm[:, d:]), "covariances differ from the handle without offsets"
    # ... and the means differ by what the joint solve says
    assert_close(marg[:, :d] - pm[:, :d], ref[0] - AN.dense_posterior(model)[0], 1e-9, f"d={d}: the shift of the means")
    dev.residual()
    dev.sweep(2)
    assert dev.residual() < 1e-10


# ---- 2. shift equivalence after every sweep -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 3, 4])
def test_every_sweep_is_the_shifted_twins(hip_lib, d):
    model = AN.chain(40, d)
    b, s = O.consistent_offsets(model, 2)
    twin, to_twin = O.shifted_twin(model, b, s)
    dev, tw = _dev(model, b=b), _dev(twin)
    ev, _ = O.latent_edges(model)
    for sweep in range(8):
        dev.sweep(1)
        tw.sweep(1)
        ma, mt = O.messages(dev, model), O.messages(tw, twin)
        assert np.array_equal(np.isnan(ma), np.isnan(mt)), f"sweep {sweep}: not the same messages undefined"
        ok = ~np.isnan(mt[:, d])
        assert ok.any()
        assert np.array_equal(ma[ok, d:], mt[ok, d:]), f"sweep {sweep}: precisions"
        assert_close(to_twin(ev[ok], ma[ok])[:, :d], mt[ok, :d], 1e-8, f"d={d} sweep {sweep}: eta' = eta - Lambda s")


# ---- 3. variables of high degree --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,make,total", [("branching b=9 d=3", lambda: AN.branching(91, 3, b=9), 10),
                                             ("multi-sensor d=4", lambda: AN.multi_sensor(12, 4, sensors=3), 16)])
def test_fused_sweeps_with_variables_of_high_degree(hip_lib, name, make, total):
    """inner states of degree 11 (the CSR tail: k_big_mv) and a chain of degree-5 states (the eight-message instance)"""
    model = make()
    b = O.with_offsets(model, 3)
    dev = _dev(model, b=b)
    dev.sweep(total)
    AN.check_marginals(dev, model, O.dense_posterior_offsets(model, b), 1e-9, name + " fixed point vs the joint solve with offsets")


# ---- 4. chain scan ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("T", [2, 9, 700])
@pytest.mark.parametrize("d", [2, 3, 4])
def test_chain_scan_one_sweep(hip_lib, monkeypatch, d, T, K):
    monkeypatch.setenv("CX_MVC_K", str(K))
    model, b, ref = _chain_case(d, T)
    dev = _dev(model, L.SCHED_CHAIN_SCAN, b=b)
    dev.sweep(1)
    marg = AN.check_marginals(dev, model, ref, 1e-9, f"d={d} T={T} K={K}")
    lazy = _dev(model, L.SCHED_CHAIN_SCAN, b=b, marginals_in_sweep=2)
    lazy.sweep(1)
    assert np.array_equal(marg, lazy.get_marginals(model.x_ids)), "marginals on demand: the same bits"
    # messages on demand: the walks run again, with the offsets
    if T == 9:
        fused = _dev(model, b=b)
        fused.sweep(T + 3)
        ma, mf = O.messages(dev, model), O.messages(fused, model)
        assert_close(ma, mf, 1e-9, f"d={d} K={K}: chain messages on demand vs the fused fixed point")


@pytest.mark.parametrize("d", [2, 4])
def test_chain_scan_with_unobserved_states(hip_lib, d):
    """every second state without a datum: side sums that are exactly zero, the links' offsets all there is between two data"""
    model = MD.make("gen", 40, d, "alt")
    b = O.with_offsets(model, 4)
    dev = _dev(model, L.SCHED_CHAIN_SCAN, b=b, loader=MD.load)
    dev.sweep(1)
    AN.check_marginals(dev, model, O.dense_posterior_offsets(model, b), 1e-9, f"d={d} chain scan, every second state unobserved")


# ---- 5. tree schedule ---------------------------------------------------------------------------------------------------------------------
TREES = [(f"comb {n} x {t} d={d}", (lambda d=d, n=n, t=t: AN.comb(n, d, teeth=t))) for d, n, t in AN.TREE_COMBS if d <= 4] + \
        [(f"branching {n} b={b} d={d}", (lambda d=d, b=b, n=n: AN.branching(n, d, b=b))) for d, b, n in AN.TREE_BRANCHING if d <= 4]


@pytest.mark.parametrize("heavy_paths", ["0", "1"])
@pytest.mark.parametrize("name,make", TREES, ids=[t[0] for t in TREES])
def test_tree_schedule_sweeps_follow_the_offsets(hip_lib, monkeypatch, name, make, heavy_paths):
    monkeypatch.setenv("CX_TREE_HP", heavy_paths)
    model, b1, ref1, b2, ref2 = O.tree_case(name, make)
    dev = _dev(model, L.SCHED_TREE, b=b1)
    dev.sweep(1)
    launches = dev.tree_heavy_path_stats()["launches"]
    assert launches == 0 if heavy_paths == "0" else (launches > 0 or "comb" not in name)
    AN.check_marginals(dev, model, ref1, 1e-9, f"{name} heavy paths {heavy_paths}")
    dev.sweep(1)                # the captured sweep, replayed
    AN.check_marginals(dev, model, ref1, 1e-9, f"{name} heavy paths {heavy_paths}, second sweep")
    dev.set_factor_offsets(*O.arrays(b2))
    dev.sweep(1)
    AN.check_marginals(dev, model, ref2, 1e-9, f"{name} heavy paths {heavy_paths}, new offsets")


@pytest.mark.parametrize("heavy_paths", ["0", "1"])
def test_a_forecast_tail_accumulates_the_offsets(hip_lib, monkeypatch, heavy_paths):
    monkeypatch.setenv("CX_TREE_HP", heavy_paths)
    d, T, h = 2, 40, 5
    model = MD.make("gen", T, d, "alt", h)
    b = O.with_offsets(model, 7)
    dev = _dev(model, L.SCHED_TREE, b=b, loader=MD.load)
    dev.sweep(1)
    marg = AN.check_marginals(dev, model, O.dense_posterior_offsets(model, b), 1e-9, f"tail, heavy paths {heavy_paths}")
    A = model.psets[0][0]
    for k, f in enumerate(model.factor_ids[-h:].tolist()):      # the tail's transitions, in time order
        want = A @ marg[T - 1 + k, :d] + b[f]
        assert_close(marg[T + k, :d], want, 1e-9, f"forecast step {k}: mean = A mean + b")


# ---- 6. loopy graphs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,T", [(3, 20), (4, AN.LOOPY_T)])
def test_fused_sweeps_on_a_loopy_graph(hip_lib, d, T):
    """general offsets, no shift behind them: the means of Gaussian BP are exact at convergence, the covariances are those of the handle
    without offsets; damping reaches the same fixed point"""
    model = AN.loopy(T, d)
    b = O.with_offsets(model, 8)
    em, _ = O.dense_posterior_offsets(model, b)
    dev, plain = _dev(model, b=b, seed_variance=AN.LOOPY_SEED_VARIANCE), _dev(model, seed_variance=AN.LOOPY_SEED_VARIANCE)
    for h in (dev, plain):
        h.sweep(AN.LOOPY_SWEEPS)
        h.residual()
        h.sweep(2)
    assert dev.residual() < 1e-10
    marg, pm = dev.get_marginals(model.x_ids), plain.get_marginals(model.x_ids)
    assert_close(marg[:, :d], em, 1e-9, f"loopy d={d}: means at the fixed point vs the joint solve with offsets")
    assert np.array_equal(marg[:, d:], pm[:, d:]), "covariances differ from the handle without offsets"
    # the Bethe evidence from the device's own messages, with the offsets in the factors
    gm = O.gmodel_offsets(model, b)
    f2v, opq = E.device_messages(gm, dev)
    want = E.bethe_log_z(gm, f2v, opq)
    got, cnt = dev.log_evidence()
    assert cnt["undefined"] == 0 and cnt["not_positive_definite"] == 0, cnt
    assert abs(got - want) <= 1e-9 * abs(want), (got, want)
    damped = _dev(model, b=b, seed_variance=AN.LOOPY_SEED_VARIANCE)
    damped.set_damping(0.3)
    n, r = damped.sweep_until(1e-11, 2000, 20)
    assert r < 1e-10, (n, r)
    assert_close(damped.get_marginals(model.x_ids), marg, 1e-9, f"loopy d={d}: the damped fixed point")


# ---- 7. batch items ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 3, 4])
def test_batch_message_items_through_factors_with_offsets(hip_lib, d):
    model = O.hub_model(d)
    (A, Q), (H, R) = model.psets[0], model.psets[1]
    Qi, Ri = np.linalg.inv(Q), np.linalg.inv(R)
    b = O.with_offsets(model, 10)
    u, y = model.data_y
    dev = _dev(model, b=b)
    M2V, M2F = L.ITEM_MESSAGE_TO_VARIABLE, L.ITEM_MESSAGE_TO_FACTOR

    def nat(v, f):
        m = dev.get_messages([v], [f], L.TO_VARIABLE, L.FORM_NATURAL)[0]
        return m[:d], m[d:].reshape(d, d)

    def close(got, want, what):
        err = float(np.max(np.abs(got - want)) / max(1.0, float(np.max(np.abs(want)))))
        assert err <= 1e-10, (what, err)

    # observed senders: eta_p = g_p + B y — forward N(A u + b, Q) into x, backward H' R^-1 (y - c) into x
    dev.update_batch([M2V, M2V], [2, 2], [10, 11])
    e10, l10 = nat(2, 10)
    close(l10, Qi, "forward, observed sender: precision")
    close(e10, Qi @ b[10] + Qi @ A @ u, "forward, observed sender: eta")
    e11, l11 = nat(2, 11)
    close(l11, H.T @ Ri @ H, "backward, observed sender: precision")
    close(e11, -H.T @ Ri @ b[11] + H.T @ Ri @ y, "backward, observed sender: eta")
    # a free sender, forward: x -> z through factor 12
    dev.update_batch([M2F], [2], [12])
    dev.update_batch([M2V], [4], [12])
    es, ls = e10 + e11, l10 + l11
    g_out, g_in = Qi @ b[12], -A.T @ Qi @ b[12]
    P_, B_, C_ = A.T @ Qi @ A, Qi @ A, Qi
    e, l = nat(4, 12)
    close(l, C_ - B_ @ np.linalg.solve(ls + P_, B_.T), "forward, free sender: precision")
    close(e, g_out + B_ @ np.linalg.solve(ls + P_, es + g_in), "forward, free sender: eta")
    # a free sender, backward: the leaf z sends what the caller stored
    rng = np.random.default_rng([d, 94])
    ez, lz = rng.standard_normal(d), AN._spd(rng, d, np.linspace(0.5, 2.0, d))
    dev.set_messages([4], [12], L.TO_FACTOR, L.FORM_NATURAL, np.concatenate([ez, lz.reshape(-1)]))
    dev.update_batch([M2V], [2], [12])
    P_, B_, C_ = Qi, A.T @ Qi, A.T @ Qi @ A
    e, l = nat(2, 12)
    close(l, C_ - B_ @ np.linalg.solve(lz + P_, B_.T), "backward, free sender: precision")
    close(e, g_in + B_ @ np.linalg.solve(lz + P_, ez + g_out), "backward, free sender: eta")


# ---- 8. the readers on forests ----------------------------------------------------------------------------------------------------------
def _reader_case(d, shape):
    def build():
        model = AN.chain(60, d) if shape == "chain" else AN.comb(15, d, teeth=1)
        b = O.with_offsets(model, 11)
        gm = O.gmodel_offsets(model, b)
        fids, sets = LS.pset_groups(model)
        return dict(model=model, b=b, gm=gm, log_z=O.joint_solve_offsets(model, b)[3], beliefs=LS.dense_factor_beliefs(gm),
                    stats=LS.grouped_statistics(gm, fids, sets, 2), n_factors=len(fids), loo=P.dense_loo_all(gm))
    return O.ref(("readers", d, shape), build)


@pytest.mark.parametrize("d,shape,sched", [(d, shape, s) for d in (2, 4) for shape, s in (("chain", "chain-scan"), ("chain", "tree"), ("comb", "tree"))])
def test_readers_on_forests_with_offsets(hip_lib, d, shape, sched):
    c = _reader_case(d, shape)
    model, gm, what = c["model"], c["gm"], f"d={d} {shape} {sched}"
    dev = _dev(model, L.SCHED_CHAIN_SCAN if sched == "chain-scan" else L.SCHED_TREE, b=c["b"])
    dev.sweep(1)
    got, cnt = dev.log_evidence()
    assert cnt["undefined"] == 0 and cnt["not_positive_definite"] == 0, (what, cnt)
    assert abs(got - c["log_z"]) <= 1e-9 * abs(c["log_z"]), (what, got, c["log_z"])
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
    P.assert_rows_close(dev.predictive("loo"), c["loo"], 1e-9, what + " loo")
    if shape == "chain":
        # the innovations sum to the evidence.  The first state has a flat prior, so the first datum's predictive is improper and no row
        # of the total; in the evidence it is the integral of N(y_1; H x_1 + c, R) over x_1 = 1 / |det H| (general H: 0.9 at d = 2)
        res = dev.predictive("causal")
        assert res["counts"]["improper"] == 1 and res["counts"]["undefined"] == 0, (what, res["counts"])
        first = -np.linalg.slogdet(model.psets[1][0])[1]
        assert abs(res["total"] + first - got) <= 1e-9 * abs(got), (what, res["total"], first, got)
    dev.close()


# ---- 9. never ignored -------------------------------------------------------------------------------------------------------------------
def test_readers_that_do_not_take_offsets_say_so(hip_lib):
    """cx_sample_posterior, cx_linear_moments and cx_causal_marginals refuse while any offset is non-zero, and work again — as on a handle
    without offsets — once all are zero"""
    d = 2
    model, b, _ = _chain_case(d, 40)
    dev, plain = _dev(model, L.SCHED_CHAIN_SCAN, b=b), _dev(model, L.SCHED_CHAIN_SCAN)
    dev.sweep(1)
    plain.sweep(1)
    nv = dev.stats()["n_variables"]
    noise = np.random.default_rng(12).standard_normal((2, nv, d))
    fs = [(model.x_ids[5:15], np.full((10, d), 0.1)), ([model.x_ids[3]], np.eye(d)[:1])]
    calls = {"sample_posterior": lambda h: h.sample_posterior(2, noise=noise)[0], "linear_moments": lambda h: np.concatenate([x.reshape(-1) for x in h.linear_moments(fs)[:2]]),
             "causal_marginals": lambda h: h.causal_marginals("filtered", 2)["mean"]}
    for name, call in calls.items():
        code, msg = code_of(lambda: call(dev))
        assert code == L.ERR_UNSUPPORTED and "cx_set_factor_offsets" in msg, (name, code, msg)
    ids, bb = O.arrays(b)
    dev.set_factor_offsets(ids, np.zeros_like(bb))
    dev.sweep(1)
    for name, call in calls.items():
        assert np.array_equal(call(dev), call(plain)), name


# ---- 10. changes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule,sweeps", [(L.SCHED_FUSED, 43), (L.SCHED_CHAIN_SCAN, 1), (L.SCHED_TREE, 1)], ids=["fused", "chain-scan", "tree"])
def test_changes_after_the_offsets(hip_lib, schedule, sweeps):
    d, T = 3, 40
    model, b, ref = _chain_case(d, T)
    dev = _dev(model, schedule, b=b)
    dev.sweep(sweeps)
    AN.check_marginals(dev, model, ref, 1e-9, "offsets")
    # new matrices under the same offsets: the linear terms follow (A, Q)
    A, Q = model.psets[0]
    dev.set_factor_matrices(0, 0.5 * A, 2.0 * Q)
    changed = dataclasses.replace(model, psets={**model.psets, 0: (0.5 * A, 2.0 * Q)})
    dev.sweep(sweeps)
    AN.check_marginals(dev, changed, O.dense_posterior_offsets(changed, b), 1e-9, "offsets, then new matrices")
    # all offsets back to zero: a fresh handle without offsets, bit for bit
    ids, bb = O.arrays(b)
    dev.set_factor_offsets(ids, np.zeros_like(bb))
    dev.sweep(sweeps)
    fresh = _dev(changed, schedule)
    fresh.sweep(sweeps)
    assert np.array_equal(dev.get_marginals(model.x_ids), fresh.get_marginals(model.x_ids))
    assert np.array_equal(O.messages(dev, model), O.messages(fresh, model), equal_nan=True)


@pytest.mark.parametrize("schedule,sweeps", [(L.SCHED_FUSED, 5), (L.SCHED_CHAIN_SCAN, 1), (L.SCHED_TREE, 1)], ids=["fused", "chain-scan", "tree"])
def test_zero_offsets_equal_a_handle_that_never_called(hip_lib, schedule, sweeps):
    d = 4
    model = AN.chain(40, d)
    zero, never = _dev(model, schedule), _dev(model, schedule)
    zero.set_factor_offsets([], np.zeros((0, d)))      # n == 0: no offset changes, the handle has offsets from now on
    for h in (zero, never):
        h.sweep(sweeps)
    assert np.array_equal(zero.get_marginals(model.x_ids), never.get_marginals(model.x_ids), equal_nan=True)
    assert np.array_equal(O.messages(zero, model), O.messages(never, model), equal_nan=True)


# ---- 11. checkpoint ---------------------------------------------------------------------------------------------------------------------
def test_checkpoint_carries_the_offsets_in_its_fingerprint(hip_lib):
    d = 3
    model = AN.loopy(20, d)
    b, other = O.with_offsets(model, 13), O.with_offsets(model, 14)
    a = _dev(model, b=b, seed_variance=AN.LOOPY_SEED_VARIANCE)
    a.sweep(7)
    blob = a.export_state()
    twin = _dev(model, b=b, seed_variance=AN.LOOPY_SEED_VARIANCE)
    twin.import_state(blob)
    a.sweep(1)
    twin.sweep(1)
    assert np.array_equal(O.messages(a, model), O.messages(twin, model), equal_nan=True)
    assert np.array_equal(a.get_marginals(model.x_ids), twin.get_marginals(model.x_ids), equal_nan=True)
    for wrong in (_dev(model, b=other), _dev(model)):
        code, msg = code_of(lambda: wrong.import_state(blob))
        assert code == L.ERR_INVALID_ARGUMENT and "different graph" in msg
    # without offsets the fingerprint is what it was: such blobs go round as before, and not into a handle that has offsets
    p, q = _dev(model, seed_variance=AN.LOOPY_SEED_VARIANCE), _dev(model)
    p.sweep(3)
    plain_blob = p.export_state()
    q.import_state(plain_blob)
    p.sweep(1)
    q.sweep(1)
    assert np.array_equal(O.messages(p, model), O.messages(q, model), equal_nan=True)
    assert code_of(lambda: twin.import_state(plain_blob))[0] == L.ERR_INVALID_ARGUMENT


# ---- 12. EM -----------------------------------------------------------------------------------------------------------------------------
def test_em_learns_a_planted_drift(hip_lib):
    T, d = 400, 2
    model = cx.synth.lgssm_chain(T, d=d, seed=15)
    (A, Q), (H, R) = model.psets[0], model.psets[1]
    b_true = np.array([0.8, -0.5])
    rng = np.random.default_rng(16)
    Lq, Lr = np.linalg.cholesky(Q), np.linalg.cholesky(R)
    x = np.zeros((T, d))
    x[0] = np.linalg.solve(np.eye(d) - A, b_true)
    for t in range(1, T):
        x[t] = A @ x[t - 1] + b_true + Lq @ rng.standard_normal(d)
    y = x @ np.asarray(H).T + rng.standard_normal((T, d)) @ Lr.T
    model = dataclasses.replace(model, data_y=y)
    sets = {0: (A, Q), 1: (H, R)}
    dev = _dev(model, L.SCHED_CHAIN_SCAN)
    trace, params, offs = learn.em(dev, sets, 15, learn=("A", "b", "Q"), offsets={0: np.zeros(d), 1: np.zeros(d)})
    assert len(trace) == 16 and set(offs) == {0, 1}
    for i in range(15):
        assert trace[i + 1] >= trace[i] - 1e-9 * abs(trace[i]), (i, trace[i], trace[i + 1])
    plain = _dev(model, L.SCHED_CHAIN_SCAN)
    trace0, _ = learn.em(plain, sets, 15, learn=("A", "Q"))
    assert trace[-1] > trace0[-1], (trace[-1], trace0[-1])
    assert np.linalg.norm(offs[0] - b_true) < np.linalg.norm(b_true), (offs[0], b_true)


# ---- 13. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(hip_lib):
    d = 2
    model = AN.chain(9, d)
    f0 = int(O.linear_factors(model)[0])
    one = np.ones((1, d))
    who = "cx_set_factor_offsets"
    # dim 1: b is a factor parameter there
    s = cx.DeviceGraph(schedule=L.SCHED_FUSED)
    cx.synth.load_into_device(cx.synth.ssm_chain_linear(6, seed=1), s)
    rc = s.lib.cx_set_factor_offsets(s.h, 0, None, None)
    assert rc == L.ERR_STATE and "dim 1 factors carry b in their parameters" in s.lib.cx_last_error(s.h).decode()
    # dim 5 .. 64, other families
    big = cx.DeviceGraph(dim=8)
    rc = big.lib.cx_set_factor_offsets(big.h, 0, None, None)
    assert rc == L.ERR_UNSUPPORTED and who in big.lib.cx_last_error(big.h).decode()
    nat2 = cx.DeviceGraph(family=L.FAMILY_NATURAL2)
    rc = nat2.lib.cx_set_factor_offsets(nat2.h, 0, None, None)
    assert rc == L.ERR_UNSUPPORTED and who in nat2.lib.cx_last_error(nat2.h).decode()
    # no graph
    empty = cx.DeviceGraph(dim=d)
    code, msg = code_of(lambda: empty.set_factor_offsets([f0], one))
    assert code == L.ERR_STATE and who in msg and "no graph" in msg
    # a factor of another kind, an unknown id, bad arguments
    top = int(max(model.edge_var.max(), model.edge_fac.max())) + 1
    with_prior = dataclasses.replace(model, edge_var=np.append(model.edge_var, model.x_ids[0]), edge_fac=np.append(model.edge_fac, top),
                                     edge_role=np.append(model.edge_role, L.ROLE_OUT).astype(np.int32), factor_ids=np.append(model.factor_ids, top),
                                     factor_kind=np.append(model.factor_kind, L.FACTOR_OPAQUE).astype(np.int32), factor_var=np.append(model.factor_var, 0.0))
    dev = _dev(with_prior)
    code, msg = code_of(lambda: dev.set_factor_offsets([top], one))
    assert code == L.ERR_UNSUPPORTED and who in msg and f"factor {top}" in msg
    code, msg = code_of(lambda: dev.set_factor_offsets([f0, 10 ** 9], np.ones((2, d))))
    assert code == L.ERR_NOT_FOUND and who in msg and str(10 ** 9) in msg
    for bad in (np.nan, np.inf):
        code, msg = code_of(lambda: dev.set_factor_offsets([f0], np.array([[0.0, bad]])))
        assert code == L.ERR_INVALID_ARGUMENT and who in msg
    ids = np.array([f0], np.int64)
    p64, pd = L.C.POINTER(L.C.c_int64), L.C.POINTER(L.C.c_double)
    assert dev.lib.cx_set_factor_offsets(dev.h, -1, ids.ctypes.data_as(p64), one.ctypes.data_as(pd)) == L.ERR_INVALID_ARGUMENT
    assert dev.lib.cx_set_factor_offsets(dev.h, 1, None, one.ctypes.data_as(pd)) == L.ERR_INVALID_ARGUMENT
    assert dev.lib.cx_set_factor_offsets(dev.h, 1, ids.ctypes.data_as(p64), None) == L.ERR_INVALID_ARGUMENT
    # nothing of that changed the handle: it never got offsets, and a blob of a plain handle still imports
    dev.import_state(_dev(with_prior).export_state())
    # a stream under capture (relaxed mode: the refusal's own runtime queries do not void the capture)
    hip = L.C.CDLL([ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln][0])
    stream, graph = L.C.c_void_p(), L.C.c_void_p()
    assert hip.hipStreamCreate(L.C.byref(stream)) == 0
    dev.set_stream(stream.value)
    assert hip.hipStreamBeginCapture(stream, 2) == 0
    rc = dev.lib.cx_set_factor_offsets(dev.h, 1, ids.ctypes.data_as(p64), one.ctypes.data_as(pd))
    assert hip.hipStreamEndCapture(stream, L.C.byref(graph)) == 0
    if graph.value:
        hip.hipGraphDestroy(graph)
    dev.set_stream(None)
    assert hip.hipStreamDestroy(stream) == 0
    assert rc == L.ERR_STATE and "captured" in dev.lib.cx_last_error(dev.h).decode()
    dev.set_factor_offsets([f0], one)           # and the handle works on
    # the reference order, wired or not
    ref = _dev(model, L.SCHED_REFERENCE)
    code, msg = code_of(lambda: ref.set_factor_offsets([f0], one))
    assert code == L.ERR_UNSUPPORTED and who in msg and "CX_SCHED_REFERENCE" in msg
    wired = cx.DeviceGraph(dim=d, schedule=L.SCHED_REFERENCE)
    for k, (A, Q) in model.psets.items():
        wired.set_factor_matrices(k, A, Q)
    wired.graph_create(model.edge_var, model.edge_fac, model.factor_ids, model.factor_kind, model.factor_var, edge_role=model.edge_role)
    wired.graph_wire(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0, np.int32))      # (wired right after graph_create, as the reference wires)
    code, msg = code_of(lambda: wired.set_factor_offsets([f0], one))
    assert code == L.ERR_UNSUPPORTED and "cx_graph_wire" in msg
    # partitions, in either order
    halo = _dev(model)
    halo.halo_configure_state([], [], [], [])
    code, msg = code_of(lambda: halo.set_factor_offsets([f0], one))
    assert code == L.ERR_UNSUPPORTED and who in msg and "partitioned" in msg
    block = _dev(model, L.SCHED_CHAIN_SCAN)
    block.halo_configure([], [], [], [])        # a chain's time block
    assert code_of(lambda: block.set_factor_offsets([f0], one))[0] == L.ERR_UNSUPPORTED
    for schedule, call in ((L.SCHED_FUSED, lambda h: h.halo_configure_state([], [], [], [])), (L.SCHED_CHAIN_SCAN, lambda h: h.halo_configure([], [], [], [])),
                           (L.SCHED_CHAIN_SCAN, lambda h: h.chain_block_maps())):
        h = _dev(model, schedule, b={f0: np.ones(d)})
        code, msg = code_of(lambda: call(h))
        assert code == L.ERR_UNSUPPORTED and who in msg


# ---- 14. the C++ client -----------------------------------------------------------------------------------------------------------------
def test_cpp_host_class_factor_offsets(hip_lib, tmp_path):
    """tests/cpp/offsets_demo.cpp: a d = 2 chain with a control input on every transition and an observation mean, through
    cortex::Handle::set_factor_offsets; its marginals against DeviceGraph's on the same model and the joint solve with offsets"""
    out_lines = run_demo("offsets_demo", tmp_path)
    rows = np.array([[float(x) for x in line.split()[1:]] for line in out_lines if line.startswith("marginal")])
    T, d = 12, 2
    A, Q = np.array([[0.9, 0.2], [-0.1, 0.8]]), np.array([[0.3, 0.05], [0.05, 0.2]])
    H, R = np.array([[1.0, 0.5], [0.0, 1.0]]), np.array([[0.5, 0.1], [0.1, 0.4]])
    xs, ys = np.arange(1, T + 1), np.arange(T + 1, 2 * T + 1)
    lik, tr = np.arange(2 * T + 1, 3 * T + 1), np.arange(3 * T + 1, 4 * T)
    IN, OUT = L.ROLE_IN, L.ROLE_OUT
    model = cx.synth.Model(edge_var=np.concatenate([np.stack([ys, xs], 1).reshape(-1), np.stack([xs[:-1], xs[1:]], 1).reshape(-1)]).astype(np.int64),
                           edge_fac=np.concatenate([np.repeat(lik, 2), np.repeat(tr, 2)]).astype(np.int64),
                           edge_role=np.concatenate([np.tile([OUT, IN], T), np.tile([IN, OUT], T - 1)]).astype(np.int32),
                           factor_ids=np.concatenate([lik, tr]).astype(np.int64), factor_kind=np.full(2 * T - 1, L.FACTOR_GAUSS_LINEAR, np.int32),
                           factor_var=np.concatenate([np.ones(T), np.zeros(T - 1)]), x_ids=xs.astype(np.int64), data_var=ys.astype(np.int64),
                           data_fac=lik.astype(np.int64), data_y=np.array([[0.5 * t + (7 * t) % 5, 1.0 - 0.25 * t] for t in range(1, T + 1)]), dim=d,
                           psets={0: (A, Q), 1: (H, R)}, meta={"kind": "demo"})
    b = {int(f): np.array([0.3, -0.2]) for f in lik}
    b.update({int(f): np.array([[0.1, 0.0], [0.0, 0.2]]) @ np.array([np.sin(0.7 * (t + 1)), 1.0]) for t, f in enumerate(tr)})
    assert rows.shape == (T, 1 + d + d * d) and np.array_equal(rows[:, 0], xs)
    dev = _dev(model, L.SCHED_CHAIN_SCAN, b=b)
    dev.sweep(1)
    marg = dev.get_marginals(xs)
    assert_close(rows[:, 1:], marg, 1e-12, "the C++ client's marginals vs DeviceGraph's")
    em, ec = O.dense_posterior_offsets(model, b)
    assert_close(marg[:, :d], em, 1e-9, "means vs the joint solve with offsets")
    assert_close(marg[:, d:].reshape(T, d, d), ec, 1e-9, "covariances vs the joint solve with offsets")
