"""-m gpu: cx_set_factor_offsets_mfma — x_out = A x_in + b + N(0, Q) at dim 5..64, a b per factor — under every schedule and through the
readers that take it, on the general models of tests/general_mfma_support.py and tests/anisotropic.py at the smallest sizes that reach
every kernel instance: dim 5 (embedded in 16), 16 (1 x 1 tiles), 17 (2 x 2, embedded), 32, 64 (4 x 4: the buffer-descriptor walks and
the pair-of-waves composition); chains of 2, 3 and 9 states under the plans CX_MVC64_K / CX_MVC64_FAN = (0, 4) and (2, 2).

References: the joint solve with offsets and the GModel with offsets (tests/offsets_support.py; pinned on the CPU at these dims in
tests/test_offsets_mfma_checker.py), and device against device through the shift equivalence: with b_a = s_out - A s_in the model is the
zero-offset model in x' = x - s, so every message obeys Lambda' = Lambda, eta' = eta - Lambda s after every sweep.

Tolerances are those of the no-offset tests of the same kernels on the same model families, none new: marginals after a chain scan 1e-9
(test_gpu_mv64_chain.py, test_gpu_native_tiles_chain.py), after fused sweeps at their fixed point and after a tree sweep 1e-8 and one
application of the rule 1e-7 (test_gpu_anisotropic.py on the matrix cores, test_gpu_native_tiles_chain.py's tree case), the evidence 1e-9
relative (test_gpu_evidence_mfma.py), belief means 1e-9, belief covariances and statistics 1e-9 max(1, max |want|)
(test_gpu_learn_mfma.py), the twin identity 1e-8 with equal precisions (test_gpu_factor_offsets.py).  Every check prints what it saw.

The dim > 1 chain scan refuses a chain with a forecast tail (tests/test_gpu_missing_data.py pins that): the tail with offsets runs under
the tree schedule here, the chain with unobserved states under the chain scan."""
import dataclasses
import math

import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from cortex.jl_amd import learn
from tests import anisotropic as AN
from tests import general_mfma_support as G
from tests import learning_support as LS
from tests import missing_data as MD
from tests import offsets_support as O
from tests.helpers import assert_close as _assert_close
from tests.gpu_support import code_of
from tests.learn_mfma_support import assert_within as _close
from tests.learn_mfma_support import bound_of as _scale

pytestmark = pytest.mark.gpu

DIMS = (5, 16, 17, 32, 64)
PLANS = ((0, 4), (2, 2))
WHO = "cx_set_factor_offsets_mfma"


def assert_close(a, b, rtol, what=""):
    a, b = np.asarray(a, float), np.asarray(b, float)
    print(f"{what}: largest error {float(np.max(np.abs(a - b))) / max(float(np.max(np.abs(b))), 1e-300):.3e} of the largest entry (bound {rtol:.0e})")
    return _assert_close(a, b, rtol, what, scale_by="max")


def _dev(model, schedule=L.SCHED_FUSED, b=None, seed_variance=None, loader=None, **kw):
    dev = cx.DeviceGraph(dim=model.dim, schedule=schedule, **kw)
    if loader is None:
        cx.synth.load_into_device(model, dev, seed_variance)
    else:
        loader(model, dev)
    if b is not None:
        dev.set_factor_offsets_mfma(*O.arrays(b))
    return dev


def _chain_case(d, T):
    def make():
        model = AN.chain(T, d)
        b = O.with_offsets(model, 1)      # scale 1: the means stay at the data's scale
        return model, b, O.dense_posterior_offsets(model, b)
    return O.ref(("chain", d, T), make)


def _set_plan(monkeypatch, K, fan):
    if K:
        monkeypatch.setenv("CX_MVC64_K", str(K))
    monkeypatch.setenv("CX_MVC64_FAN", str(fan))


# ---- 1. fused sweeps on a chain ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
def test_fused_sweeps_on_a_chain_with_offsets(hip_lib, d):
    T = 6
    model, b, ref = _chain_case(d, T)
    dev, plain = _dev(model, b=b), _dev(model)
    dev.sweep(T + 3)
    plain.sweep(T + 3)
    marg = AN.check_marginals(dev, model, ref, 1e-8, f"d={d} fixed point vs the joint solve with offsets", close=assert_close)
    # the offsets move no precision: the precision part of every message into a latent variable is the no-offset handle's, bit for bit
    ma, mp = O.messages(dev, model), O.messages(plain, model)
    assert np.array_equal(np.isnan(ma), np.isnan(mp))
    assert np.array_equal(ma[:, d:], mp[:, d:], equal_nan=True), "precisions differ from the handle without offsets"
    assert np.nanmax(np.abs(ma[:, :d] - mp[:, :d])) > 0.1, "the offsets did not reach the messages"
    pm = plain.get_marginals(model.x_ids)
    assert np.array_equal(marg[:, d:], pm[:, d:]), "covariances differ from the handle without offsets"
    assert_close(marg[:, :d] - pm[:, :d], ref[0] - AN.dense_posterior(model)[0], 1e-8, f"d={d}: the shift of the means")


# ---- 2. every sweep is the shifted twin's ------------------------------------------------------------------------------------------------
SHIFT = [("chain", d) for d in DIMS] + [("ring", 5), ("ring", 16)]


@pytest.mark.parametrize("shape,d", SHIFT, ids=[f"{s}-d{d}" for s, d in SHIFT])
def test_every_sweep_is_the_shifted_twins(hip_lib, shape, d):
    """device against device: after 1, 2 and 5 fused sweeps every stored message of the handle with consistent offsets is the zero-offset
    twin's under Lambda' = Lambda, eta' = eta - Lambda s; the ring is loopy and needs seeded messages: the identity holds from a start that
    is the twin's start shifted, so the twin starts at N(0, v I) and the handle with offsets at (eta, Lambda) = (s / v, I / v)"""
    model = G.chain(d) if shape == "chain" else G.ring(d)
    b, s = O.consistent_offsets(model, 2)
    twin, to_twin = O.shifted_twin(model, b, s)
    seed = None if shape == "chain" else G.RING_SEED_VARIANCE
    dev, tw = _dev(model, b=b, seed_variance=seed), _dev(twin, seed_variance=seed)
    ev, ef = O.latent_edges(model)
    if seed is not None:
        lam = np.eye(d) / seed
        dev.set_messages(ev, ef, L.TO_VARIABLE, L.FORM_NATURAL, np.stack([np.concatenate([lam @ s[int(x)], lam.reshape(-1)]) for x in ev]))
    done = 0
    for upto in (1, 2, 5):
        dev.sweep(upto - done)
        tw.sweep(upto - done)
        done = upto
        ma, mt = O.messages(dev, model), O.messages(tw, twin)
        assert np.array_equal(np.isnan(ma), np.isnan(mt)), f"sweep {upto}: not the same messages undefined"
        ok = ~np.isnan(mt[:, d])
        assert ok.any()
        assert np.array_equal(ma[ok, d:], mt[ok, d:]), f"sweep {upto}: precisions"
        assert_close(to_twin(ev[ok], ma[ok])[:, :d], mt[ok, :d], 1e-8, f"{shape} d={d} sweep {upto}: eta' = eta - Lambda s")


# ---- 3. chain scan ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,fan", PLANS)
@pytest.mark.parametrize("T", [2, 3, 9])
@pytest.mark.parametrize("d", DIMS)
def test_chain_scan_one_sweep(hip_lib, monkeypatch, d, T, K, fan):
    _set_plan(monkeypatch, K, fan)
    model, b, ref = _chain_case(d, T)
    dev = _dev(model, L.SCHED_CHAIN_SCAN, b=b)
    dev.sweep(1)
    if (T, K) == (9, 2):
        assert dev.chain_plan_stats()["levels"] >= 2
    AN.check_marginals(dev, model, ref, 1e-9, f"d={d} T={T} K={K} fan={fan}", close=assert_close)


@pytest.mark.parametrize("d", [7, 16, 64])
def test_chain_scan_with_unobserved_states(hip_lib, monkeypatch, d):
    """every second state without a datum: side sums that are exactly zero, the links' offsets all there is between two data"""
    _set_plan(monkeypatch, 2, 2)
    model = MD.make("gen", 12, d, "alt")
    b = O.with_offsets(model, 4)
    dev = _dev(model, L.SCHED_CHAIN_SCAN, b=b, loader=MD.load)
    dev.sweep(1)
    AN.check_marginals(dev, model, O.dense_posterior_offsets(model, b), 1e-9, f"d={d} chain scan, every second state unobserved", close=assert_close)


# ---- 4. tree schedule ---------------------------------------------------------------------------------------------------------------------
TREES = [(f"comb d={d}", (lambda d=d: G.comb(d))) for d in (5, 16, 64)] + [(f"forest d={d}", (lambda d=d: G.forest(d))) for d in (5, 17)]


@pytest.mark.parametrize("heavy_paths", ["0", "1"])
@pytest.mark.parametrize("name,make", TREES, ids=[t[0] for t in TREES])
def test_tree_schedule_sweeps_follow_the_offsets(hip_lib, monkeypatch, name, make, heavy_paths):
    monkeypatch.setenv("CX_TREE_HP", heavy_paths)
    model, b1, ref1, b2, ref2 = O.tree_case(name, make)
    dev = _dev(model, L.SCHED_TREE, b=b1)
    dev.sweep(1)
    launches = dev.tree_heavy_path_stats()["launches"]
    assert launches == 0 if heavy_paths == "0" else launches > 0, launches
    AN.check_marginals(dev, model, ref1, 1e-8, f"{name} heavy paths {heavy_paths}", close=assert_close)
    dev.sweep(1)                # the captured sweep, replayed
    AN.check_marginals(dev, model, ref1, 1e-8, f"{name} heavy paths {heavy_paths}, second sweep", close=assert_close)
    dev.set_factor_offsets_mfma(*O.arrays(b2))
    dev.sweep(1)
    AN.check_marginals(dev, model, ref2, 1e-8, f"{name} heavy paths {heavy_paths}, new offsets", close=assert_close)


@pytest.mark.parametrize("heavy_paths", ["0", "1"])
def test_a_forecast_tail_accumulates_the_offsets(hip_lib, monkeypatch, heavy_paths):
    monkeypatch.setenv("CX_TREE_HP", heavy_paths)
    d, T, h = 16, 12, 3
    model = MD.make("gen", T, d, "alt", h)
    b = O.with_offsets(model, 7)
    dev = _dev(model, L.SCHED_TREE, b=b, loader=MD.load)
    dev.sweep(1)
    marg = AN.check_marginals(dev, model, O.dense_posterior_offsets(model, b), 1e-8, f"tail, heavy paths {heavy_paths}", close=assert_close)
    A = model.psets[0][0]
    for k, f in enumerate(model.factor_ids[-h:].tolist()):      # the tail's transitions, in time order
        want = A @ marg[T - 1 + k, :d] + b[f]
        assert_close(marg[T + k, :d], want, 1e-8, f"forecast step {k}: mean = A mean + b")


# ---- 5. a sender of degree 5, batch items ------------------------------------------------------------------------------------------------
def test_fused_sweeps_with_a_sender_of_degree_five(hip_lib):
    """a chain of states with three sensors each: the inner states have degree 5, their messages go through k_v2f64's stored sums (the
    "fixed" sender of the rule record), which take g of the sender's slot like any other"""
    d = 16
    model = AN.multi_sensor(4, d, sensors=3)
    b = O.with_offsets(model, 3)
    dev = _dev(model, b=b)
    dev.sweep(8)
    AN.check_marginals(dev, model, O.dense_posterior_offsets(model, b), 1e-8, "multi-sensor d=16 fixed point vs the joint solve with offsets", close=assert_close)


@pytest.mark.parametrize("d", [5, 16])
def test_batch_message_items_through_factors_with_offsets(hip_lib, d):
    """cx_update_batch's message items against the closed formulas, one application of the rule each (1e-7: the per-sweep bound on the
    matrix cores)"""
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

    # observed senders: eta_p = g_p + B y — forward N(A u + b, Q) into x, backward H' R^-1 (y - c) into x
    dev.update_batch([M2V, M2V], [2, 2], [10, 11])
    e10, l10 = nat(2, 10)
    assert_close(l10, Qi, 1e-7, "forward, observed sender: precision")
    assert_close(e10, Qi @ b[10] + Qi @ A @ u, 1e-7, "forward, observed sender: eta")
    e11, l11 = nat(2, 11)
    assert_close(l11, H.T @ Ri @ H, 1e-7, "backward, observed sender: precision")
    assert_close(e11, -H.T @ Ri @ b[11] + H.T @ Ri @ y, 1e-7, "backward, observed sender: eta")
    # a free sender, forward: x -> z through factor 12
    dev.update_batch([M2F], [2], [12])
    dev.update_batch([M2V], [4], [12])
    es, ls = e10 + e11, l10 + l11
    g_out, g_in = Qi @ b[12], -A.T @ Qi @ b[12]
    P_, B_, C_ = A.T @ Qi @ A, Qi @ A, Qi
    e, l = nat(4, 12)
    assert_close(l, C_ - B_ @ np.linalg.solve(ls + P_, B_.T), 1e-7, "forward, free sender: precision")
    assert_close(e, g_out + B_ @ np.linalg.solve(ls + P_, es + g_in), 1e-7, "forward, free sender: eta")
    # a free sender, backward: the leaf z sends what the caller stored
    rng = np.random.default_rng([d, 94])
    ez, lz = rng.standard_normal(d), AN._spd(rng, d, np.linspace(0.5, 2.0, d))
    dev.set_messages([4], [12], L.TO_FACTOR, L.FORM_NATURAL, np.concatenate([ez, lz.reshape(-1)]))
    dev.update_batch([M2V], [2], [12])
    P_, B_, C_ = Qi, A.T @ Qi, A.T @ Qi @ A
    e, l = nat(2, 12)
    assert_close(l, C_ - B_ @ np.linalg.solve(lz + P_, B_.T), 1e-7, "backward, free sender: precision")
    assert_close(e, g_in + B_ @ np.linalg.solve(lz + P_, ez + g_out), 1e-7, "backward, free sender: eta")


# ---- 6. the readers that take the offsets ---------------------------------------------------------------------------------------------------
def _reader_case(shape, d):
    def build():
        model = {"chain": G.chain, "comb": G.comb, "clamped": G.clamped}[shape](d)
        b = O.with_offsets(model, 11)
        gm = O.gmodel_offsets(model, b)
        fids, sets = LS.pset_groups(model)
        beliefs = LS.dense_factor_beliefs(gm, fids)
        return dict(model=model, b=b, gm=gm, log_z=O.joint_solve_offsets(model, b)[3], fids=fids, beliefs=beliefs,
                    stats=LS.grouped_statistics(gm, fids, sets, 2, beliefs=beliefs))
    return O.ref(("readers", shape, d), build)


READERS = [(shape, d, "tree") for shape in ("chain", "comb") for d in (5, 16, 17, 64)] + [("chain", 16, "chain-scan"), ("chain", 64, "chain-scan"),
                                                                                           ("clamped", 16, "tree"), ("clamped", 5, "tree")]


@pytest.mark.parametrize("shape,d,sched", READERS, ids=[f"{s}-d{d}-{k}" for s, d, k in READERS])
def test_readers_after_an_exact_sweep(hip_lib, shape, d, sched):
    """log_evidence_mfma, factor_beliefs_mfma and factor_statistics_mfma (r = x_out - A x_in - b, every factor its own b).  The chain and
    the comb have factors with two free ends and with the OUT end observed (the likelihoods); the clamped chain adds a factor with both
    ends observed, a transition with its OUT end observed and one with its IN end observed"""
    c = _reader_case(shape, d)
    model, what = c["model"], f"{shape} d={d} {sched}"
    dev = _dev(model, L.SCHED_CHAIN_SCAN if sched == "chain-scan" else L.SCHED_TREE, b=c["b"])
    dev.sweep(1)
    got, cnt = dev.log_evidence_mfma()
    print(f"{what} log-evidence: got {got!r} want {c['log_z']!r} relative error {abs(got - c['log_z']) / abs(c['log_z']):.3e} (bound 1e-09) {cnt}")
    assert cnt["undefined"] == 0 and cnt["not_positive_definite"] == 0, (what, cnt)
    assert abs(got - c["log_z"]) <= 1e-9 * abs(c["log_z"]), (what, got, c["log_z"])
    gm_, gc_ = dev.factor_beliefs_mfma(c["fids"])
    _close(gm_, c["beliefs"][0], 1e-9, what + " belief means")
    _close(gc_, c["beliefs"][1], _scale(c["beliefs"][1]), what + " belief covariances")
    st, scnt = dev.factor_statistics_mfma(n_groups=2)
    for key in LS.KEYS:
        _close(st[key], c["stats"][key], _scale(c["stats"][key]), f"{what} {key}")
    assert scnt == {"factors": len(c["fids"]), "groups": 2, "undefined": 0, "not_positive_definite": 0}, (what, scnt)
    # the offsets are in the numbers: the handle without them gives another evidence
    plain = _dev(model, L.SCHED_TREE)
    plain.sweep(1)
    assert abs(plain.log_evidence_mfma()[0] - got) > 0.1


@pytest.mark.parametrize("d", G.FOREST_DIMS)
def test_components_sum_to_the_total(hip_lib, d):
    model = G.forest(d)
    b = O.with_offsets(model, 12)
    dev = _dev(model, L.SCHED_TREE, b=b)
    dev.sweep(1)
    total, cnt = dev.log_evidence_mfma()
    values, comp_counts, _ = dev.log_evidence_components_mfma()
    want = O.joint_solve_offsets(model, b)[3]
    assert len(values) == 3 and cnt["undefined"] == 0 and cnt["not_positive_definite"] == 0
    gap, scale = abs(math.fsum(values.tolist()) - total), float(np.sum(np.abs(values)))
    print(f"forest d={d}: |fsum(values) - log_evidence_mfma| = {gap:.3e}, sum |values| = {scale:.6e} (bound 1e-12 relative); total relative error "
          f"{abs(total - want) / abs(want):.3e} (bound 1e-9)")
    assert gap <= 1e-12 * scale, (gap, scale)
    assert abs(total - want) <= 1e-9 * abs(want), (total, want)


# ---- 7. zero offsets are no offsets ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule,sweeps", [(L.SCHED_FUSED, 5), (L.SCHED_CHAIN_SCAN, 1), (L.SCHED_TREE, 1)], ids=["fused", "chain-scan", "tree"])
@pytest.mark.parametrize("d", [16, 64])
def test_zero_offsets_equal_a_handle_that_never_called(hip_lib, monkeypatch, d, schedule, sweeps):
    _set_plan(monkeypatch, 2, 2)
    model = AN.chain(9, d)
    zero, never = _dev(model, schedule), _dev(model, schedule)
    zero.set_factor_offsets_mfma([], np.zeros((0, d)))      # n == 0: no offset changes, the handle has offsets from now on
    for h in (zero, never):
        h.sweep(sweeps)
    assert np.array_equal(zero.get_marginals(model.x_ids), never.get_marginals(model.x_ids), equal_nan=True)
    assert np.array_equal(O.messages(zero, model), O.messages(never, model), equal_nan=True)
    if schedule != L.SCHED_FUSED:      # (after five fused sweeps some messages are still undefined: no evidence yet)
        assert zero.log_evidence_mfma()[0] == never.log_evidence_mfma()[0]
        fids = LS.pset_groups(model)[0]
        for a, c in zip(zero.factor_beliefs_mfma(fids), never.factor_beliefs_mfma(fids)):
            assert np.array_equal(a, c)
        sa, sc = zero.factor_statistics_mfma(n_groups=2)[0], never.factor_statistics_mfma(n_groups=2)[0]
        assert all(np.array_equal(sa[k], sc[k]) for k in LS.KEYS)


# ---- 8. changes afterwards ---------------------------------------------------------------------------------------------------------------
def _refusing_calls(model, d):
    noise = lambda h: np.random.default_rng(12).standard_normal((2, h.stats()["n_variables"], d))      # noqa: E731
    fs = [(model.x_ids[1:4], np.full((3, d), 0.1)), ([model.x_ids[3]], np.eye(d)[:1])]
    return {"cx_predictive_mfma": lambda h: h.predictive_mfma("loo", rows=False)["total"],
            "cx_predictive_rows_mfma": lambda h: h.predictive_rows_mfma(),
            "cx_causal_marginals_mfma": lambda h: h.causal_marginals_mfma("filtered", 2)["mean"],
            "cx_sample_posterior_mfma": lambda h: h.sample_posterior_mfma(2, noise=noise(h))[0],
            "cx_linear_moments_mfma": lambda h: np.concatenate([x.reshape(-1) for x in h.linear_moments_mfma(fs)[:2]])}


@pytest.mark.parametrize("schedule,sweeps", [(L.SCHED_FUSED, 12), (L.SCHED_CHAIN_SCAN, 1), (L.SCHED_TREE, 1)], ids=["fused", "chain-scan", "tree"])
def test_changes_after_the_offsets(hip_lib, monkeypatch, schedule, sweeps):
    _set_plan(monkeypatch, 2, 2)
    d, T = 16, 9
    tol = 1e-9 if schedule == L.SCHED_CHAIN_SCAN else 1e-8
    model, b, ref = _chain_case(d, T)
    dev = _dev(model, schedule, b=b)
    dev.sweep(sweeps)
    AN.check_marginals(dev, model, ref, tol, "offsets", close=assert_close)
    # new matrices under the same offsets: g and kappa follow (A, Q)
    A, Q = model.psets[0]
    dev.set_factor_matrices(0, 0.5 * A, 2.0 * Q)
    changed = dataclasses.replace(model, psets={**model.psets, 0: (0.5 * A, 2.0 * Q)})
    dev.sweep(sweeps)
    AN.check_marginals(dev, changed, O.dense_posterior_offsets(changed, b), tol, "offsets, then new matrices", close=assert_close)
    want = O.joint_solve_offsets(changed, b)[3]
    got = dev.log_evidence_mfma()[0]
    print(f"evidence after new matrices: relative error {abs(got - want) / abs(want):.3e} (bound 1e-9)")
    assert abs(got - want) <= 1e-9 * abs(want), (got, want)
    # some offsets replaced: the others keep theirs
    ids, bb = O.arrays(b)
    b2 = dict(b)
    for f in ids[::2].tolist():
        b2[f] = -2.0 * b[f]
    dev.set_factor_offsets_mfma(ids[::2], np.stack([b2[int(f)] for f in ids[::2]]))
    dev.sweep(sweeps)
    AN.check_marginals(dev, changed, O.dense_posterior_offsets(changed, b2), tol, "some offsets replaced", close=assert_close)
    # all offsets back to zero: a fresh handle without offsets, bit for bit, and the readers that refused work again
    calls = _refusing_calls(model, d)
    if schedule == L.SCHED_CHAIN_SCAN:
        for name, call in calls.items():
            code, msg = code_of(lambda: call(dev))
            assert code == L.ERR_UNSUPPORTED and WHO in msg, (name, code, msg)
    dev.set_factor_offsets_mfma(ids, np.zeros_like(bb))
    dev.sweep(sweeps)
    fresh = _dev(changed, schedule)
    fresh.sweep(sweeps)
    assert np.array_equal(dev.get_marginals(model.x_ids), fresh.get_marginals(model.x_ids))
    assert np.array_equal(O.messages(dev, model), O.messages(fresh, model), equal_nan=True)
    if schedule == L.SCHED_CHAIN_SCAN:
        for name, call in calls.items():
            assert np.array_equal(call(dev), call(fresh)), name


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(hip_lib):
    d = 16
    model = AN.chain(9, d)
    f0 = int(O.linear_factors(model)[0])
    one = np.ones((1, d))
    # dim 1 .. 4: the other function's
    for small in (cx.DeviceGraph(schedule=L.SCHED_FUSED), cx.DeviceGraph(dim=2)):
        rc = small.lib.cx_set_factor_offsets_mfma(small.h, 0, None, None)
        msg = small.lib.cx_last_error(small.h).decode()
        assert rc == L.ERR_UNSUPPORTED and WHO in msg and "cx_set_factor_offsets;" in msg.replace("cx_set_factor_offsets_mfma", ""), msg
    nat2 = cx.DeviceGraph(family=L.FAMILY_NATURAL2)
    rc = nat2.lib.cx_set_factor_offsets_mfma(nat2.h, 0, None, None)
    assert rc == L.ERR_UNSUPPORTED and WHO in nat2.lib.cx_last_error(nat2.h).decode()
    # no graph
    empty = cx.DeviceGraph(dim=d)
    code, msg = code_of(lambda: empty.set_factor_offsets_mfma([f0], one))
    assert code == L.ERR_STATE and WHO in msg and "no graph" in msg
    # a factor of another kind, an unknown id, bad arguments
    top = int(max(model.edge_var.max(), model.edge_fac.max())) + 1
    with_prior = dataclasses.replace(model, edge_var=np.append(model.edge_var, model.x_ids[0]), edge_fac=np.append(model.edge_fac, top),
                                     edge_role=np.append(model.edge_role, L.ROLE_OUT).astype(np.int32), factor_ids=np.append(model.factor_ids, top),
                                     factor_kind=np.append(model.factor_kind, L.FACTOR_OPAQUE).astype(np.int32), factor_var=np.append(model.factor_var, 0.0))
    dev = _dev(with_prior)
    code, msg = code_of(lambda: dev.set_factor_offsets_mfma([top], one))
    assert code == L.ERR_UNSUPPORTED and WHO in msg and f"factor {top}" in msg
    code, msg = code_of(lambda: dev.set_factor_offsets_mfma([f0, 10 ** 9], np.ones((2, d))))
    assert code == L.ERR_NOT_FOUND and WHO in msg and str(10 ** 9) in msg
    for bad in (np.nan, np.inf):
        row = np.zeros((1, d))
        row[0, d - 1] = bad
        code, msg = code_of(lambda: dev.set_factor_offsets_mfma([f0], row))
        assert code == L.ERR_INVALID_ARGUMENT and WHO in msg
    ids = np.array([f0], np.int64)
    p64, pd = L.C.POINTER(L.C.c_int64), L.C.POINTER(L.C.c_double)
    assert dev.lib.cx_set_factor_offsets_mfma(dev.h, -1, ids.ctypes.data_as(p64), one.ctypes.data_as(pd)) == L.ERR_INVALID_ARGUMENT
    assert dev.lib.cx_set_factor_offsets_mfma(dev.h, 1, None, one.ctypes.data_as(pd)) == L.ERR_INVALID_ARGUMENT
    assert dev.lib.cx_set_factor_offsets_mfma(dev.h, 1, ids.ctypes.data_as(p64), None) == L.ERR_INVALID_ARGUMENT
    # nothing of that changed the handle: it never got offsets, and a blob of a plain handle still imports
    dev.import_state(_dev(with_prior).export_state())
    # a stream under capture (relaxed mode: the refusal's own runtime queries do not void the capture)
    hip = L.C.CDLL([ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln][0])
    stream, graph = L.C.c_void_p(), L.C.c_void_p()
    assert hip.hipStreamCreate(L.C.byref(stream)) == 0
    dev.set_stream(stream.value)
    assert hip.hipStreamBeginCapture(stream, 2) == 0
    rc = dev.lib.cx_set_factor_offsets_mfma(dev.h, 1, ids.ctypes.data_as(p64), one.ctypes.data_as(pd))
    assert hip.hipStreamEndCapture(stream, L.C.byref(graph)) == 0
    if graph.value:
        hip.hipGraphDestroy(graph)
    dev.set_stream(None)
    assert hip.hipStreamDestroy(stream) == 0
    assert rc == L.ERR_STATE and "captured" in dev.lib.cx_last_error(dev.h).decode()
    dev.set_factor_offsets_mfma([f0], one)           # and the handle works on
    # the readers that do not take offsets, with ONE non-zero offset
    dev.sweep(1)
    for name, call in _refusing_calls(with_prior, d).items():
        code, msg = code_of(lambda: call(dev))
        assert code == L.ERR_UNSUPPORTED and WHO in msg and name in msg, (name, code, msg)
    # the dim 2 - 4 entry keeps refusing these dims, and em keeps refusing offsets there
    assert dev.lib.cx_set_factor_offsets(dev.h, 0, None, None) == L.ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="offsets"):
        learn.em(dev, dict(model.psets), n_iter=1, offsets={0: np.zeros(d)})
    # the reference order
    ref = _dev(model, L.SCHED_REFERENCE)
    code, msg = code_of(lambda: ref.set_factor_offsets_mfma([f0], one))
    assert code == L.ERR_UNSUPPORTED and WHO in msg and "CX_SCHED_REFERENCE" in msg
    # partitions, in either order
    halo = _dev(model)
    halo.halo_configure_state([], [], [], [])
    code, msg = code_of(lambda: halo.set_factor_offsets_mfma([f0], one))
    assert code == L.ERR_UNSUPPORTED and WHO in msg and "partitioned" in msg
    for schedule, call in ((L.SCHED_FUSED, lambda h: h.halo_configure_state([], [], [], [])), (L.SCHED_CHAIN_SCAN, lambda h: h.halo_configure([], [], [], []))):
        h = _dev(model, schedule, b={f0: np.ones(d)})
        code, msg = code_of(lambda: call(h))
        assert code == L.ERR_UNSUPPORTED and "cx_set_factor_offsets" in msg
    m64 = AN.chain(3, 64)
    h = _dev(m64, L.SCHED_CHAIN_SCAN, b={int(O.linear_factors(m64)[0]): np.ones(64)})
    code, msg = code_of(lambda: h.chain_block_maps())
    assert code == L.ERR_UNSUPPORTED and "cx_set_factor_offsets" in msg


# ---- 10. checkpoint ------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_carries_the_offsets_in_its_fingerprint(hip_lib):
    d = 16
    model = G.ring(d)
    b, other = O.with_offsets(model, 13), O.with_offsets(model, 14)
    a = _dev(model, b=b, seed_variance=G.RING_SEED_VARIANCE)
    a.sweep(4)
    blob = a.export_state()
    twin = _dev(model, b=b, seed_variance=G.RING_SEED_VARIANCE)
    twin.import_state(blob)
    a.sweep(1)
    twin.sweep(1)
    assert np.array_equal(O.messages(a, model), O.messages(twin, model), equal_nan=True)
    assert np.array_equal(a.get_marginals(model.x_ids), twin.get_marginals(model.x_ids), equal_nan=True)
    for wrong in (_dev(model, b=other), _dev(model)):
        code, msg = code_of(lambda: wrong.import_state(blob))
        assert code == L.ERR_INVALID_ARGUMENT and "different graph" in msg
    p = _dev(model, seed_variance=G.RING_SEED_VARIANCE)
    p.sweep(2)
    assert code_of(lambda: twin.import_state(p.export_state()))[0] == L.ERR_INVALID_ARGUMENT


# ---- 11. EM ------------------------------------------------------------------------------------------------------------------------------
def test_em_learns_a_planted_drift(hip_lib):
    """the chain starts at rest and drifts to its level (I - A)^-1 b: started AT that level the states are nearly constant, A times the
    level and b are told apart by the noise alone, and EM's b wanders along that ridge (the numpy EM on the dense posterior does the same)"""
    T, d, n_iter = 200, 8, 10
    model = cx.synth.lgssm_chain(T, d=d, seed=15)
    (A, Q), (H, R) = model.psets[0], model.psets[1]
    rng = np.random.default_rng(16)
    b_true = 0.6 * rng.standard_normal(d)
    Lq, Lr = np.linalg.cholesky(Q), np.linalg.cholesky(R)
    x = np.zeros((T, d))
    for t in range(1, T):
        x[t] = A @ x[t - 1] + b_true + Lq @ rng.standard_normal(d)
    y = x @ np.asarray(H).T + rng.standard_normal((T, d)) @ Lr.T
    model = dataclasses.replace(model, data_y=y)
    dev = _dev(model, L.SCHED_CHAIN_SCAN)
    trace, params, offs = learn.em_mfma(dev, {0: (A, Q), 1: (H, R)}, n_iter, learn={0: ("A", "b", "Q"), 1: ()}, offsets={0: 0})
    print("trace", trace, "b", offs[0], "planted", b_true)
    assert len(trace) == n_iter + 1 and set(offs) == {0}
    for i in range(n_iter):
        assert trace[i + 1] >= trace[i] - 1e-9 * abs(trace[i]), (i, trace[i], trace[i + 1])
    assert np.linalg.norm(offs[0] - b_true) < np.linalg.norm(b_true), (offs[0], b_true)
    assert np.array_equal(params[1][0], H) and np.array_equal(params[1][1], R)
