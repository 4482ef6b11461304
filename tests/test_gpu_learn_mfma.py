"""-m gpu: cx_factor_beliefs_mfma / cx_factor_statistics_mfma and learn.em at the matrix-core dims (cx_create dim 5 .. 64)
against the dense posterior, the dense residual statistics, the RTS smoother, Shumway–Stoffer EM and the numpy restatement of the
kernel's algebra on the device's own messages (tests/learn_mfma_support.py, pinned on the CPU by tests/test_learn_mfma_checker.py).
Bounds: those of tests/test_gpu_factor_statistics.py for the same comparisons at dim 2 .. 4 — means 1e-9, covariances and statistics
1e-9 max(1, max|want|)."""
import ctypes as C
import math

import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from cortex.jl_amd import learn
from tests import evidence_mfma_support as EM
from tests import evidence_support as E
from tests import learn_mfma_support as M
from tests import learning_support as S
from tests import missing_data as MD
from tests.gpu_support import HANDLE_CASES, STREAM_CASES, assert_reader_refusals, code_of, demo_chain, run_demo, swept_device, under_capture
from tests.learn_mfma_support import assert_within as _close
from tests.learn_mfma_support import bound_of as _scale

pytestmark = pytest.mark.gpu


def _check_beliefs(dev, gm, what, fids=None, want=None):
    fids = gm.groups[2]["fid"] if fids is None else fids
    got_m, got_c = dev.factor_beliefs_mfma(fids)
    want_m, want_c = S.dense_factor_beliefs(gm, fids) if want is None else want
    _close(got_m, want_m, 1e-9, what + " means")
    _close(got_c, want_c, _scale(want_c), what + " covariances")
    return got_m, got_c


def _check_stats(got, cnt, want, n_counted, n_groups_used, what):
    for k in S.KEYS:
        _close(got[k], want[k], _scale(want[k]), f"{what} {k}")
    assert cnt == {"factors": n_counted, "groups": n_groups_used, "undefined": 0, "not_positive_definite": 0}, (what, cnt)


def _set_groups(model, gm):
    sets = {int(f): int(s) for f, s in zip(*S.pset_groups(model))}
    fids = gm.groups[2]["fid"]
    return fids, np.array([sets[int(f)] for f in fids])


# ---- 1, 2. beliefs and default-grouping statistics against the dense posterior, after every exact schedule --------------------------
@pytest.mark.parametrize("shape", ["chain", "comb"])
@pytest.mark.parametrize("d", M.DIMS)
def test_beliefs_and_statistics_match_the_dense_posterior(hip_lib, d, shape):
    name, model, chain = [m for m in M.small_models(d) if m[0] == shape][0]
    gm = E.gmodel(model)
    fids, groups = _set_groups(model, gm)
    want_b = S.dense_factor_beliefs(gm, fids)
    want_s = S.grouped_statistics(gm, fids, groups, 3)
    for s in [L.SCHED_TREE, L.SCHED_REFERENCE] + ([L.SCHED_CHAIN_SCAN] if chain else []):
        dev = swept_device(model, s)
        _check_beliefs(dev, gm, f"d {d} {name} schedule {s}", want=want_b)
        got, cnt = dev.factor_statistics_mfma(n_groups=3)                      # set 2 unused: a zero row
        _check_stats(got, cnt, want_s, len(fids), 2, f"d {d} {name} schedule {s}")
        assert got["n"][2] == 0 and not np.any(got["S_rr"][2])
        for k in (0, 1):      # the M-step on them against one written out in numpy: A alone, then Q alone (five factors do not determine both at d = 64)
            A = np.asarray(model.psets[k][0], float)
            want_k = {key: v[k] for key, v in want_s.items()}
            wantA, wantQ = M.numpy_m_step(want_k, A, learn=("A",))[0], M.numpy_m_step(want_k, A, learn=())[1]
            _close(learn.m_step(learn.group(got, k), A, learn=("A",))["A"], wantA, 1e-7 * max(1.0, float(np.max(np.abs(wantA)))), f"d {d} {name} M-step A of set {k}")
            _close(learn.m_step(learn.group(got, k), A, learn=("Q",))["Q"], wantQ, 1e-7 * max(1.0, float(np.max(np.abs(wantQ)))), f"d {d} {name} M-step Q of set {k}")
        dev.close()


# ---- 3. explicit groups and every argument error ------------------------------------------------------------------------------------------
def test_explicit_groups_and_argument_errors(hip_lib):
    d = 20
    model = cx.synth.lgssm_chain(9, d=d, seed=51)
    gm = E.gmodel(model)
    fids, sets = _set_groups(model, gm)
    dev = swept_device(model, L.SCHED_TREE)
    # the transitions split into two groups by parity, a few factors skipped, the likelihoods in group 3; the caller's order is free
    rng = np.random.default_rng(d)
    groups = np.where(sets == 0, 1 + (np.arange(len(fids)) % 2), 3)
    groups[[2, 7, 12]] = -1
    perm = rng.permutation(len(fids))
    got, cnt = dev.factor_statistics_mfma(fids[perm], groups[perm], n_groups=5)
    want = S.grouped_statistics(gm, fids, groups, 5)
    _check_stats(got, cnt, want, int((groups >= 0).sum()), 3, "explicit groups")
    assert got["n"][0] == 0 and got["n"][4] == 0 and not np.any(got["S_xx"][0])
    # the cached lists serve the same arrays again, and another grouping replaces them
    again, _ = dev.factor_statistics_mfma(fids[perm], groups[perm], n_groups=5)
    assert all(np.array_equal(got[k], again[k]) for k in S.KEYS)
    by_set, cnt = dev.factor_statistics_mfma(n_groups=2)
    _check_stats(by_set, cnt, S.grouped_statistics(gm, fids, sets, 2), len(fids), 2, "sets after explicit")
    # errors
    tr, lik = fids[sets == 0], fids[sets == 1]
    who = "cx_factor_statistics_mfma"
    code, msg = code_of(dev.factor_statistics_mfma, [tr[0], lik[0]], [0, 0], n_groups=1)
    assert code == L.ERR_INVALID_ARGUMENT and who in msg and "do not share" in msg
    code, msg = code_of(dev.factor_statistics_mfma, [tr[0], tr[0]], [0, 0], n_groups=1)
    assert code == L.ERR_INVALID_ARGUMENT and "listed twice" in msg
    code, msg = code_of(dev.factor_statistics_mfma, [tr[0]], [3], n_groups=2)
    assert code == L.ERR_INVALID_ARGUMENT and "not in -1" in msg
    code, msg = code_of(dev.factor_statistics_mfma, [10 ** 6], [0], n_groups=1)
    assert code == L.ERR_NOT_FOUND and who in msg
    code, msg = code_of(dev.factor_statistics_mfma, n_groups=1)
    assert code == L.ERR_INVALID_ARGUMENT and "n_groups must exceed" in msg
    out, c4 = np.zeros(10 ** 4), (np.zeros(4, np.int64))
    assert dev.lib.cx_factor_statistics_mfma(dev.h, 0, None, None, 0, out.ctypes.data_as(C.POINTER(C.c_double)), c4.ctypes.data_as(C.POINTER(C.c_int64))) == L.ERR_INVALID_ARGUMENT
    assert dev.lib.cx_factor_statistics_mfma(dev.h, 0, None, None, 2, None, None) == L.ERR_INVALID_ARGUMENT
    f1 = np.array([tr[0]], np.int64)
    assert dev.lib.cx_factor_statistics_mfma(dev.h, 1, f1.ctypes.data_as(C.POINTER(C.c_int64)), None, 2, out.ctypes.data_as(C.POINTER(C.c_double)),
                                             c4.ctypes.data_as(C.POINTER(C.c_int64))) == L.ERR_INVALID_ARGUMENT
    assert b"go together" in dev.lib.cx_last_error(dev.h)
    code, msg = code_of(dev.factor_beliefs_mfma, [10 ** 6])
    assert code == L.ERR_NOT_FOUND and "cx_factor_beliefs_mfma" in msg
    assert dev.lib.cx_factor_beliefs_mfma(dev.h, 1, None, None) == L.ERR_INVALID_ARGUMENT
    m, c = dev.factor_beliefs_mfma(np.zeros(0, np.int64))
    assert m.shape == (0, 2 * d) and c.shape == (0, 2 * d, 2 * d)
    dev.close()
    # an opaque message is no factor of the list; by parameter set it is simply not counted
    model, opq = EM.prior_chain(16)
    dev = cx.DeviceGraph(dim=16, schedule=L.SCHED_TREE)
    cx.synth.load_into_device(model, dev)
    EM.set_opaque(dev, opq)
    dev.sweep(1)
    code, msg = code_of(dev.factor_beliefs_mfma, opq[1])
    assert code == L.ERR_UNSUPPORTED and str(int(opq[1][0])) in msg and "CX_FACTOR_GAUSS_LINEAR" in msg
    code, msg = code_of(dev.factor_statistics_mfma, opq[1], [0], n_groups=1)
    assert code == L.ERR_UNSUPPORTED and str(int(opq[1][0])) in msg
    dev.close()


# ---- 4. observed ends -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", M.OBSERVED_DIMS)
def test_observed_ends(hip_lib, d):
    model = EM.clamped_middle(d)      # a factor with both ends observed, one with its OUT end, one with its IN end observed
    gm = E.gmodel(model)
    fids, groups = _set_groups(model, gm)
    dev = swept_device(model, L.SCHED_TREE)
    _, got_c = _check_beliefs(dev, gm, f"clamped middle d {d}")
    obs = gm.obs[gm.groups[2]["vars"]]
    for r in range(len(fids)):      # zero rows and columns on the observed ends, exactly
        for e in range(2):
            if obs[r, e]:
                assert not np.any(got_c[r, e * d:(e + 1) * d, :]) and not np.any(got_c[r, :, e * d:(e + 1) * d])
    got, cnt = dev.factor_statistics_mfma(n_groups=2)
    _check_stats(got, cnt, S.grouped_statistics(gm, fids, groups, 2), len(fids), 2, f"clamped middle d {d}")
    dev.close()


# ---- 5. missing data and a forecast tail ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", EM.FORECAST_DIMS)
def test_missing_data_and_a_forecast_tail(hip_lib, d):
    model, _ = EM.forecast_chain(d)
    gm = E.gmodel(model)
    fids, groups = _set_groups(model, gm)
    dev = cx.DeviceGraph(dim=d, schedule=L.SCHED_TREE)
    MD.load(model, dev)                    # the flat message on the last state's one edge
    dev.sweep(1)
    _check_beliefs(dev, gm, f"forecast tail d {d}")
    got, cnt = dev.factor_statistics_mfma(n_groups=2)
    _check_stats(got, cnt, S.grouped_statistics(gm, fids, groups, 2), len(fids), 2, f"forecast tail d {d}")
    # the last transition alone: its OUT end is the latent leaf, Λ_out = 0, K = 0 and Cov(r) = M⁻¹ = Q to the rounding of one inverse
    last = fids[np.argmax(fids)]
    one, _ = dev.factor_statistics_mfma([last], [0], n_groups=1)
    Q = np.asarray(model.psets[0][1], float)
    cov_r = one["S_rr"][0] - np.outer(one["sum_r"][0], one["sum_r"][0])
    _close(cov_r, Q, 1e-12 * float(np.max(np.abs(Q))), f"Cov(r) = Q behind the flat leaf, d {d}")
    dev.close()


# ---- 6. an opaque prior -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", EM.OPAQUE_DIMS)
def test_opaque_prior(hip_lib, d):
    model, opq = EM.prior_chain(d)
    gm = E.gmodel(model, opaque=opq)
    fids, groups = _set_groups(model, gm)
    dev = cx.DeviceGraph(dim=d, schedule=L.SCHED_TREE)
    cx.synth.load_into_device(model, dev)
    EM.set_opaque(dev, opq)
    dev.sweep(1)
    _check_beliefs(dev, gm, f"prior chain d {d}")
    got, cnt = dev.factor_statistics_mfma(n_groups=2)
    _check_stats(got, cnt, S.grouped_statistics(gm, fids, groups, 2), len(fids), 2, f"prior chain d {d}")
    dev.close()


# ---- 7. a loop: the Bethe beliefs of the device's own messages ----------------------------------------------------------------------------
@pytest.mark.parametrize("d", EM.RING_DIMS)
def test_loop_matches_the_restatement_on_the_device_messages(hip_lib, d):
    model = EM.ring(d)
    gm = E.gmodel(model)
    dev = swept_device(model, L.SCHED_FUSED, EM.RING_SWEEPS)
    f2v, opq = E.device_messages(gm, dev)
    want_m, want_c, status = M.beliefs(gm, f2v, opq)
    assert np.all(status == M.OK)
    _, got_c = _check_beliefs(dev, gm, f"ring d {d}", want=(want_m, want_c))
    exact_c = S.dense_factor_beliefs(gm, gm.groups[2]["fid"])[1]
    assert np.max(np.abs(got_c - exact_c)) > 1e-6 * np.max(np.abs(exact_c))      # the Bethe beliefs, not the exact ones
    fids, groups = _set_groups(model, gm)
    got, cnt = dev.factor_statistics_mfma(n_groups=2)
    want, _ = M.statistics(gm, f2v, fids, groups, 2, opq)
    _check_stats(got, cnt, want, len(fids), 2, f"ring d {d}")
    dev.close()


# ---- 8. undefined, then exact, then new parameters ------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [8, 32])
def test_undefined_then_exact_then_new_parameters(hip_lib, d):
    model = cx.synth.lgssm_chain(7, d=d, seed=81 + d)
    gm = E.gmodel(model)
    fids, groups = _set_groups(model, gm)
    dev = cx.DeviceGraph(dim=d, schedule=L.SCHED_TREE)
    cx.synth.load_into_device(model, dev)
    got, cnt = dev.factor_statistics_mfma(n_groups=2)                     # before any sweep
    assert cnt["undefined"] > 0 and cnt["not_positive_definite"] == 0 and cnt["factors"] == len(fids), cnt
    assert np.isnan(got["S_rr"][0]).all() and np.isnan(got["sum_x"][0]).all() and got["n"][0] == 6
    m, c = dev.factor_beliefs_mfma(fids[groups == 0])
    assert np.isnan(m).all() and np.isnan(c).all()
    dev.sweep(1)
    _check_beliefs(dev, gm, f"d {d} old (A, Q)")
    first, cnt = dev.factor_statistics_mfma(n_groups=2)
    _check_stats(first, cnt, S.grouped_statistics(gm, fids, groups, 2), len(fids), 2, f"d {d} old (A, Q)")
    A, Q = model.psets[0]
    A2, Q2 = 0.9 * np.asarray(A), 2.0 * np.asarray(Q)
    dev.set_factor_matrices(0, A2, Q2)
    dev.sweep(1)
    psets = dict(model.psets)
    psets[0] = (A2, Q2)
    gm2 = E.gmodel(model, psets=psets)
    _check_beliefs(dev, gm2, f"d {d} new (A, Q)")
    second, cnt = dev.factor_statistics_mfma(n_groups=2)                  # the A table followed (r = x_out - A x_in under the NEW A)
    _check_stats(second, cnt, S.grouped_statistics(gm2, fids, groups, 2), len(fids), 2, f"d {d} new (A, Q)")
    assert np.max(np.abs(second["S_rr"][0] - first["S_rr"][0])) > 1e-3
    dev.close()


# ---- 9. not positive definite ---------------------------------------------------------------------------------------------------------------
def test_a_factorisation_that_fails_counts_as_not_positive_definite(hip_lib):
    # test_gpu_evidence_mfma's construction: every stored message defined, then the prior on x_2 becomes negative definite WITHOUT a
    # sweep.  The transition out of x_2 fails in its second stage, the one into it in its FIRST stage, x_2's likelihood in its only one.
    d = 16
    base = cx.synth.lgssm_chain(5, d=d, seed=77)
    model, f = EM._with_opaque(base, base.x_ids[1:2])
    opq = (base.x_ids[1:2], f, np.zeros((1, d)), np.eye(d)[None])
    gm = E.gmodel(model, opaque=opq)
    dev = cx.DeviceGraph(dim=d, schedule=L.SCHED_TREE)
    cx.synth.load_into_device(model, dev)
    EM.set_opaque(dev, opq)
    dev.sweep(1)
    _check_beliefs(dev, gm, "proper prior on x_2")
    EM.set_opaque(dev, (opq[0], opq[1], opq[2], -100.0 * opq[3]))
    fids = gm.groups[2]["fid"]
    touches = np.array([int(gm.var_ids[v[0]] == base.x_ids[1] or gm.var_ids[v[1]] == base.x_ids[1]) for v in gm.groups[2]["vars"]])
    assert touches.sum() == 3
    _, sets = _set_groups(model, gm)
    groups = 2 * (1 - touches) + sets      # 0, 1: the transitions and the likelihood on x_2; 2, 3: the other transitions and likelihoods
    got, cnt = dev.factor_statistics_mfma(fids, groups, n_groups=4)
    assert cnt["undefined"] == 0 and cnt["not_positive_definite"] == 3 and cnt["factors"] == len(fids) and cnt["groups"] == 4, cnt
    assert got["n"][0] == 2 and got["n"][1] == 1
    for g in (0, 1):
        assert all(np.isnan(got[k][g]).all() for k in S.KEYS if k != "n")
    for g in (2, 3):
        assert all(np.isfinite(got[k][g]).all() for k in S.KEYS)
    m, c = dev.factor_beliefs_mfma(fids)
    bad = np.isnan(m).all(axis=1)
    assert np.array_equal(bad, touches.astype(bool)) and np.isfinite(c[~bad]).all() and np.isnan(c[bad]).all()
    dev.close()


# ---- 10. the embedded-dim rule --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [8, 20])
def test_embedded_dims_give_the_real_models_values_at_any_tile_size(hip_lib, d, monkeypatch):
    model = cx.synth.lgssm_chain(5, d=d, seed=90 + d)
    gm = E.gmodel(model)
    fids, groups = _set_groups(model, gm)
    want = S.grouped_statistics(gm, fids, groups, 2)
    dev = swept_device(model, L.SCHED_TREE)
    nat_b = _check_beliefs(dev, gm, f"d {d}, native tile")
    nat_s, cnt = dev.factor_statistics_mfma(n_groups=2)
    _check_stats(nat_s, cnt, want, len(fids), 2, f"d {d}, native tile")
    dev.close()
    monkeypatch.setenv("CX_MFMA_DIM", "64")
    dev = swept_device(model, L.SCHED_TREE)
    monkeypatch.delenv("CX_MFMA_DIM")
    for_b = _check_beliefs(dev, gm, f"d {d}, 4 x 4 tiles")
    for_s, cnt = dev.factor_statistics_mfma(n_groups=2)
    _check_stats(for_s, cnt, want, len(fids), 2, f"d {d}, 4 x 4 tiles")
    dev.close()
    for a, b, what in [(for_b[0], nat_b[0], "means"), (for_b[1], nat_b[1], "covariances")] + [(for_s[k], nat_s[k], k) for k in S.KEYS]:
        _close(a, b, 1e-12 * max(1.0, float(np.max(np.abs(b)))), f"d {d} forced against native, {what}")


# ---- 11. several partials per group ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,d", M.LONG)
def test_long_chains_against_the_rts_smoother(hip_lib, T, d):
    model = cx.synth.lgssm_chain(T, d=d, seed=33)
    dev = swept_device(model, L.SCHED_CHAIN_SCAN)
    got, cnt = dev.factor_statistics_mfma(n_groups=2)
    _check_stats(got, cnt, M.rts_statistics(model), 2 * T - 1, 2, f"d = {d}, T = {T}")
    again, _ = dev.factor_statistics_mfma(n_groups=2)
    assert all(got[k].tobytes() == again[k].tobytes() for k in S.KEYS)      # two calls on one state of one handle: bit-identical
    # a long list of beliefs goes through in chunks: the last transition's row is the smoother's
    fids, sets = S.pset_groups(model)
    tr = np.sort(fids[sets == 0])
    m, c = dev.factor_beliefs_mfma(tr)
    A, Q, R = model.meta["A"], model.meta["Q"], model.meta["R"]
    _, ms, Ps, Pc = S.rts(A, Q, np.eye(d), R, np.asarray(model.data_y, float).reshape(T, d))
    want_m = np.concatenate([ms[1:], ms[:-1]], axis=1)
    want_c = np.block([[Ps[1:], Pc], [np.swapaxes(Pc, 1, 2), Ps[:-1]]])
    _close(m, want_m, 1e-9, f"d = {d}, T = {T} belief means of every transition")
    _close(c, want_c, _scale(want_c), f"d = {d}, T = {T} belief covariances of every transition")
    dev.close()


def test_more_partials_than_waves(hip_lib):
    # 2,549 partials for the 2,048 waves of a launch at 1 x 1 tiles: a wave walks several partials (each with a row, counters and a reset of
    # its own), and the groups of 500 and 400 factors are cut into partials of two
    T, d = M.MANY
    model = cx.synth.lgssm_chain(T, d=d, seed=33)
    groups, n_groups = M.many_groups(T)
    fids, sets = S.pset_groups(model)
    tr, lik = np.sort(fids[sets == 0]), np.sort(fids[sets == 1])      # ids ascend in time
    dev = swept_device(model, L.SCHED_CHAIN_SCAN)
    ids, grp = np.concatenate([tr, lik]), np.concatenate([groups[0], groups[1]])
    got, cnt = dev.factor_statistics_mfma(ids, grp, n_groups=n_groups)
    _check_stats(got, cnt, M.rts_statistics(model, groups, n_groups), 2 * T - 1, n_groups, f"d = {d}, T = {T}, {n_groups} groups")
    again, _ = dev.factor_statistics_mfma(ids, grp, n_groups=n_groups)
    assert all(got[k].tobytes() == again[k].tobytes() for k in S.KEYS)
    # new parameters keep the lists (they follow the graph and the arrays alone) and move the numbers
    A, Q = model.psets[0]
    dev.set_factor_matrices(0, A, 2.0 * np.asarray(Q))
    dev.sweep(1)
    third, cnt = dev.factor_statistics_mfma(ids, grp, n_groups=n_groups)
    m2 = cx.synth.lgssm_chain(T, d=d, seed=33)
    m2.meta["Q"] = 2.0 * np.asarray(Q)
    _check_stats(third, cnt, M.rts_statistics(m2, groups, n_groups), 2 * T - 1, n_groups, f"d = {d}, T = {T}, {n_groups} groups, 2 Q")
    dev.close()


# ---- 12. moves nothing ------------------------------------------------------------------------------------------------------------------
def test_moves_nothing(hip_lib):
    model = cx.synth.lgssm_chain(8, d=16, seed=72)
    fids, _ = S.pset_groups(model)
    for s in (L.SCHED_CHAIN_SCAN, L.SCHED_REFERENCE, L.SCHED_TREE):
        dev = swept_device(model, s)
        if s == L.SCHED_CHAIN_SCAN:      # (another reader first: every reader of the messages brings them to their slots)
            dev.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE)
        blob, marg = dev.export_state(), dev.get_marginals(model.x_ids)
        plan = dev.ref_plan_stats() if s == L.SCHED_REFERENCE else None
        sweeps = dev.stats()["sweeps_done"]
        dev.factor_statistics_mfma(n_groups=2)          # the FIRST call: it builds the lists
        dev.factor_beliefs_mfma(fids)
        assert np.array_equal(blob, dev.export_state())
        assert np.array_equal(marg, dev.get_marginals(model.x_ids))
        dev.factor_statistics_mfma(n_groups=2)
        assert np.array_equal(blob, dev.export_state())
        if plan is not None:
            assert plan == dev.ref_plan_stats()
        assert sweeps == dev.stats()["sweeps_done"]
        dev.close()
    # fused: the next sweeps are those of a twin handle that never called them, bit for bit
    a, b = swept_device(model, L.SCHED_FUSED, 5), swept_device(model, L.SCHED_FUSED, 5)
    assert a.residual() == b.residual()
    a.factor_statistics_mfma(n_groups=2)
    a.factor_beliefs_mfma(fids)
    a.sweep(3); b.sweep(3)
    ra, rb = a.residual(), b.residual()
    assert math.isfinite(ra) and ra == rb, (ra, rb)
    assert np.array_equal(a.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE), b.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE),
                          equal_nan=True)
    assert np.array_equal(a.get_marginals(model.x_ids), b.get_marginals(model.x_ids))
    a.close(); b.close()


# ---- 13. EM -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [8, 16])
def test_em_matches_shumway_stoffer(hip_lib, d):
    T = 200
    model = cx.synth.lgssm_chain(T, d=d, seed=260 + d)
    rng = np.random.default_rng(d)
    A0 = model.meta["A"] + 0.05 * rng.standard_normal((d, d)) / math.sqrt(d)
    Q0, C0, R0 = 2.0 * model.meta["Q"], np.eye(d) + 0.05 * rng.standard_normal((d, d)) / math.sqrt(d), 0.5 * model.meta["R"]
    y = np.asarray(model.data_y).reshape(T, d)
    want_trace, want_params = S.ss_em(y, A0, Q0, C0, R0, n_iter=8)
    dev = cx.DeviceGraph(dim=d, schedule=L.SCHED_CHAIN_SCAN)
    cx.synth.load_into_device(model, dev)
    trace, params = learn.em(dev, {0: (A0, Q0), 1: (C0, R0)}, n_iter=8, learn=("A", "Q"))
    print("trace", trace, "want", want_trace)
    assert np.all(np.diff(trace) >= -1e-9 * abs(trace[-1])), np.diff(trace)
    got, want = np.asarray(trace), np.asarray(want_trace)
    err = float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1.0)))
    print(f"d {d} EM trace: max relative error {err:.3e} (bound 1e-7)")
    assert err <= 1e-7, err
    with pytest.raises(ValueError, match="offsets"):
        learn.em(dev, {0: (A0, Q0), 1: (C0, R0)}, n_iter=1, offsets={0: np.zeros(d)})
    with pytest.raises(ValueError, match="by_component"):
        learn.em(dev, {0: (A0, Q0), 1: (C0, R0)}, n_iter=1, by_component=True)
    dev.close()


# ---- 14. refusals ---------------------------------------------------------------------------------------------------------------------
P64, PD = C.POINTER(C.c_int64), C.POINTER(C.c_double)


def _raw_beliefs(dev, ids, bel):
    return dev.lib.cx_factor_beliefs_mfma(dev.h, len(ids), ids.ctypes.data_as(P64), bel.ctypes.data_as(PD))


def _raw_statistics(dev, st, c4):
    return dev.lib.cx_factor_statistics_mfma(dev.h, 0, None, None, 2, st.ctypes.data_as(PD), c4.ctypes.data_as(P64))


# what assert_reader_refusals asks of the two readers (factor 13: a likelihood of its dim 4 chain, the first transition of its dim 16 one)
_COMMON = (dict(who="cx_factor_beliefs_mfma", small="cx_factor_beliefs", call=lambda dev: dev.factor_beliefs_mfma([13]),
                small_call=lambda dev: dev.factor_beliefs([13]),
                raw=lambda dev: _raw_beliefs(dev, np.array([13], np.int64), np.zeros((1, 2 * 16 + 4 * 256)))),
           dict(who="cx_factor_statistics_mfma", small="cx_factor_statistics", call=lambda dev: dev.factor_statistics_mfma(n_groups=2),
                small_call=lambda dev: dev.factor_statistics(n_groups=2),
                raw=lambda dev: _raw_statistics(dev, np.zeros((2, 1 + 2 * 16 + 3 * 256)), np.zeros(4, np.int64))))


def test_refusals(hip_lib):
    for reader in _COMMON:
        assert_reader_refusals(**reader, cases=HANDLE_CASES)


def test_refusals_of_a_captured_stream_and_of_parameter_sets_never_set(hip_lib):
    for reader in _COMMON:
        assert_reader_refusals(**reader, cases=STREAM_CASES)
    d = 16
    model = cx.synth.lgssm_chain(5, d=d, seed=93)
    fids, _ = S.pset_groups(model)
    dev = swept_device(model, L.SCHED_TREE)
    want_s, _ = dev.factor_statistics_mfma(n_groups=2)
    want_b = dev.factor_beliefs_mfma(fids)
    ids = np.asarray(fids, np.int64)
    bel, st, c4 = np.zeros((len(ids), 2 * d + 4 * d * d)), np.zeros((2, 1 + 2 * d + 3 * d * d)), np.zeros(4, np.int64)
    rc, msg = under_capture(dev, lambda: _raw_beliefs(dev, ids, bel))
    assert rc == L.ERR_STATE and msg.startswith("cx_factor_beliefs_mfma") and "captured" in msg, (rc, msg)
    rc, msg = under_capture(dev, lambda: _raw_statistics(dev, st, c4))
    assert rc == L.ERR_STATE and msg.startswith("cx_factor_statistics_mfma") and "captured" in msg, (rc, msg)
    assert not bel.any() and not st.any()                      # nothing was written
    got_s, _ = dev.factor_statistics_mfma(n_groups=2)          # and the handle works on, bit for bit
    got_b = dev.factor_beliefs_mfma(fids)
    assert all(np.array_equal(got_s[k], want_s[k]) for k in S.KEYS) and np.array_equal(got_b[0], want_b[0]) and np.array_equal(got_b[1], want_b[1])
    dev.close()


# ---- 15. the C++ host class -------------------------------------------------------------------------------------------------------------
def test_cpp_host_class_factor_statistics_mfma(hip_lib, tmp_path):
    rows = {line.split()[0]: line.split()[1:] for line in run_demo("learn_mfma_demo", tmp_path)}
    T, d = 12, 16
    A, Q, R, y = demo_chain(T, d)

    class _Chain:      # what rts_statistics reads of a model
        dim, data_y, meta = d, y, {"T": T, "A": A, "Q": Q, "R": R}

    want = M.rts_statistics(_Chain)
    assert int(rows["before"][2]) > 0 and rows["counts"] == [str(2 * T - 1), "2", "0", "0"]
    flat = np.concatenate([np.concatenate([[want["n"][g]]] + [want[k][g].ravel() for k in S.KEYS[1:]]) for g in range(2)])
    _close(np.array(rows["stats"], float), flat, _scale(flat), "C++ statistics")
    _, ms, Ps, Pc = S.rts(A, Q, np.eye(d), R, y)
    belief = np.concatenate([ms[1], ms[0], np.block([[Ps[1], Pc[0]], [Pc[0].T, Ps[0]]]).ravel()])
    _close(np.array(rows["belief"], float), belief, _scale(belief), "C++ belief")
