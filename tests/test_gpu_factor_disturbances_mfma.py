"""-m gpu: cx_factor_disturbances_mfma / cx_factor_disturbance_rows_mfma — the smoothed disturbance E[r | data],
Cov(r | data), t = E[r'Q⁻¹r | data] and q = E[r]'Q⁻¹E[r] of every two-variable factor at the matrix-core dims — against the dense joint
posterior, the RTS smoother and the numpy restatement of the kernel's algebra on the device's own messages
(tests/disturbances_mfma_support.py, pinned on the CPU by tests/test_disturbances_mfma_checker.py).
Bounds: those of tests/test_gpu_learn_mfma.py for the same kernel's outputs — means 1e-9, covariances 1e-9 max(1, max|want|), Cov(r) = Q
behind a flat leaf 1e-12 max|Q|, a forced tile size against the native one 1e-12 max(1, max|want|).  t and q against the same sums
formed in numpy from the device's OWN rows and the model's Q: the rounding of a d²-term sum, 4 d² ε Σ|term|."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from cortex.jl_amd import learn
from tests import disturbances_mfma_support as D
from tests import evidence_mfma_support as EM
from tests import evidence_support as E
from tests import general_mfma_support as G
from tests import learn_mfma_support as M
from tests import learning_support as S
from tests import missing_data as MD
from tests import offsets_support as O
from tests.gpu_support import HANDLE_CASES, STREAM_CASES, assert_reader_refusals, code_of, demo_chain, run_demo, under_capture
from tests.learn_mfma_support import assert_within as _close
from tests.learn_mfma_support import bound_of as _scale

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float64).eps)
WHO = "cx_factor_disturbances_mfma"
KEYS = ("mean", "cov", "expected_mahalanobis", "mahalanobis")


def _dev(model, schedule, sweeps=1, b=None, loader=None):
    dev = cx.DeviceGraph(dim=model.dim, schedule=schedule)
    if loader is None:
        cx.synth.load_into_device(model, dev, seed_variance=1e6 if schedule == L.SCHED_FUSED else None)
    else:
        loader(model, dev)
    if b is not None:
        dev.set_factor_offsets_mfma(*O.arrays(b))
    dev.sweep(sweeps)
    return dev


def _check_scores(res, Q, what):
    """t and q against the same sums in numpy from the device's own rows; t = s + q, so t >= q when Cov(r) is positive semi-definite"""
    d = res["mean"].shape[1]
    t, q, mag = D.scores(res["mean"], res["cov"], Q)
    for got, want, name in ((res["expected_mahalanobis"], t, "t"), (res["mahalanobis"], q, "q")):
        ratio = float(np.max(np.abs(got - want) / np.maximum(4 * d * d * EPS * mag, 1e-300))) if len(t) else 0.0
        print(f"{what} {name}: largest error / (4 d² ε Σ|term|) = {ratio:.3e}")
        assert np.all(np.isfinite(got)) and ratio <= 1.0, (what, name, ratio)
    assert np.all(res["expected_mahalanobis"] >= res["mahalanobis"] - 4 * d * d * EPS * mag), what


def _check(dev, model, want, what, ids=None):
    """rows and scores of `ids` (default: every row) against `want` (support rows in ascending id); returns the device's dict"""
    res = dev.factor_disturbances_mfma(ids)
    assert np.array_equal(res["factor_ids"], want["factor_ids"]), what
    n = len(want["factor_ids"])
    assert res["counts"] == {"rows": n, "finite": n, "undefined": 0, "not_positive_definite": 0}, (what, res["counts"])
    _close(res["mean"], want["mean"], 1e-9, what + " means")
    _close(res["cov"], want["cov"], _scale(want["cov"]), what + " covariances")
    _check_scores(res, D.factor_Q(model, res["factor_ids"]), what)
    tot = float(np.sum(res["expected_mahalanobis"]))
    assert abs(res["total"] - tot) <= 4 * max(n, 1) * EPS * float(np.sum(np.abs(res["expected_mahalanobis"]))), (what, res["total"], tot)
    return res


def _check_trace(res, model, want_cov, what):
    """Σ_f (t_f - q_f) = d x (non-observed variables), to n_factors d² max|Q⁻¹| times the covariance bound"""
    n, d = res["mean"].shape
    Qi = np.linalg.inv(D.factor_Q(model, res["factor_ids"]))
    got, want = float(np.sum(res["expected_mahalanobis"] - res["mahalanobis"])), D.latent_dims(model)
    tol = n * d * d * float(np.max(np.abs(Qi))) * _scale(want_cov)
    print(f"{what}: Σ (t - q) = {got:.12g}, latent components {want} (bound {tol:.3e})")
    assert abs(got - want) <= tol, (what, got, want)


def _bits(a, b, keys=KEYS):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in keys)


# ---- 1, 2. the dense posterior on forests; the rows add up to the statistics -------------------------------------------------------------
@pytest.mark.parametrize("shape", ["chain", "comb"])
@pytest.mark.parametrize("d", M.DIMS)
def test_rows_match_the_dense_posterior_and_add_up_to_the_statistics(hip_lib, d, shape):
    name, model, chain = [m for m in M.small_models(d) if m[0] == shape][0]
    want = D.dense(model)
    sets = {int(f): int(s) for f, s in zip(*S.pset_groups(model))}
    for s in [L.SCHED_TREE] + ([L.SCHED_CHAIN_SCAN] if chain else []):
        dev = _dev(model, s)
        what = f"d {d} {name} schedule {s}"
        res = _check(dev, model, want, what)
        _check_trace(res, model, want["cov"], what)
        # the rows, added per parameter set in numpy, are sum_r and S_rr of the statistics on the same handle: two orders of one f64 sum
        st, cnt = dev.factor_statistics_mfma(n_groups=2)
        assert cnt["factors"] == len(res["factor_ids"]) and cnt["undefined"] == 0 and cnt["not_positive_definite"] == 0
        grp = np.array([sets[int(f)] for f in res["factor_ids"]])
        for k in (0, 1):
            m, c = res["mean"][grp == k], res["cov"][grp == k]
            terms = c + m[:, :, None] * m[:, None, :]
            for got, t, key in ((st["sum_r"][k], m, "sum_r"), (st["S_rr"][k], terms, "S_rr")):
                bound = 4 * len(m) * EPS * np.sum(np.abs(t), axis=0)
                ratio = float(np.max(np.abs(got - t.sum(axis=0)) / np.maximum(bound, 1e-300)))
                print(f"{what} set {k} {key}: largest error / (4 n ε Σ|term|) = {ratio:.3e}")
                assert ratio <= 1.0, (what, k, key, ratio)
        dev.close()


# ---- 3. observed ends -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offsets", [False, True])
@pytest.mark.parametrize("d", M.OBSERVED_DIMS)
def test_observed_ends(hip_lib, d, offsets):
    model = G.clamped(d)      # a factor with both ends observed, one with its OUT end, one with its IN end observed
    b = O.with_offsets(model, 5) if offsets else None
    dev = _dev(model, L.SCHED_TREE, b=b)
    res = _check(dev, model, D.dense(model, b), f"clamped d {d} offsets {offsets}")
    gm = E.gmodel(model)
    g = gm.groups[2]
    obs = {int(f): tuple(bool(x) for x in gm.obs[v]) for f, v in zip(g["fid"], g["vars"])}
    assert {(True, False), (False, True), (True, True), (False, False)} <= set(obs.values())
    for i, f in enumerate(res["factor_ids"].tolist()):
        if obs[f] != (True, True):
            assert np.any(res["cov"][i])
            continue
        # r is a number: y_o - A y_i - b to the rounding of a d-term sum, exact zeros for its covariance, t = q
        fi = int(np.nonzero(g["fid"] == f)[0][0])
        A, yo, yi = -g["C"][fi, 1], gm.y[g["vars"][fi][0]], gm.y[g["vars"][fi][1]]
        bf = np.zeros(d) if b is None else b[f]
        _close(res["mean"][i], yo - A @ yi - bf, float(np.max(4 * d * EPS * (np.abs(yo) + np.abs(A) @ np.abs(yi) + np.abs(bf)))), f"d {d} both ends observed: mean")
        assert not np.any(res["cov"][i])
        assert res["expected_mahalanobis"][i] == res["mahalanobis"][i]
    dev.close()


# ---- 4. flat leaves: missing data, a forecast tail; an opaque prior ------------------------------------------------------------------------
@pytest.mark.parametrize("d", EM.FORECAST_DIMS)
def test_missing_data_and_a_forecast_tail(hip_lib, d):
    model, _ = EM.forecast_chain(d)
    dev = _dev(model, L.SCHED_TREE, loader=MD.load)      # the flat message on the last state's one edge
    want = D.dense(model)
    res = _check(dev, model, want, f"forecast tail d {d}")
    _check_trace(res, model, want["cov"], f"forecast tail d {d}")
    # the last transition: its OUT end is the latent leaf, Λ_out = 0, K = 0: Cov(r) = M⁻¹ = Q to the rounding of one inverse, mean 0, t = d
    last = int(np.argmax(res["factor_ids"]))
    Q = D.factor_Q(model, res["factor_ids"])[last]
    qtol = 1e-12 * float(np.max(np.abs(Q)))
    _close(res["cov"][last], Q, qtol, f"Cov(r) = Q behind the flat leaf, d {d}")
    _close(res["mean"][last], 0.0, 1e-9, f"E[r] = 0 behind the flat leaf, d {d}")
    _close(res["expected_mahalanobis"][last], d, d * d * float(np.max(np.abs(np.linalg.inv(Q)))) * qtol + 1e-18, f"t = d behind the flat leaf, d {d}")
    z = learn.auxiliary_residuals(res, D.factor_Q(model, res["factor_ids"]))
    assert np.isnan(z[last]).all() and np.isfinite(z[0]).all()
    dev.close()


@pytest.mark.parametrize("d", EM.OPAQUE_DIMS)
def test_opaque_prior(hip_lib, d):
    model, opq = EM.prior_chain(d)

    def load(m, dev):
        cx.synth.load_into_device(m, dev)
        EM.set_opaque(dev, opq)
    dev = _dev(model, L.SCHED_TREE, loader=load)
    _check(dev, model, D.dense(model, opaque=opq), f"prior chain d {d}")      # (the prior is no factor of the sum: no trace identity here)
    dev.close()


# ---- 5. offsets ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["chain", "comb"])
@pytest.mark.parametrize("d", [16, 40])
def test_offsets(hip_lib, d, shape):
    name, model, chain = [m for m in M.small_models(d) if m[0] == shape][0]
    b = O.with_offsets(model, 3)
    want = D.dense(model, b)
    dev = _dev(model, L.SCHED_CHAIN_SCAN if chain else L.SCHED_TREE, b=b)
    res = _check(dev, model, want, f"d {d} {name} with offsets")
    _check_trace(res, model, want["cov"], f"d {d} {name} with offsets")
    assert np.max(np.abs(res["mean"] - D.dense(model)["mean"])) > 1e-3      # r uses the factor's own b
    dev.close()
    # all-zero offsets: the bits of a handle that never called set_factor_offsets_mfma
    zero = _dev(model, L.SCHED_TREE, b={int(f): np.zeros(d) for f in O.linear_factors(model)})
    never = _dev(model, L.SCHED_TREE)
    a, c = zero.factor_disturbances_mfma(), never.factor_disturbances_mfma()
    assert _bits(a, c) and a["total"] == c["total"] and a["counts"] == c["counts"]
    zero.close(); never.close()


# ---- 6. a loop: the Bethe beliefs of the device's own messages ----------------------------------------------------------------------------
@pytest.mark.parametrize("d", EM.RING_DIMS)
def test_loop_matches_the_restatement_on_the_device_messages(hip_lib, d):
    model = EM.ring(d)
    gm = E.gmodel(model)
    dev = _dev(model, L.SCHED_FUSED, EM.RING_SWEEPS)
    f2v, opq = E.device_messages(gm, dev)
    res = _check(dev, model, D.restated(gm, f2v, opq), f"ring d {d}")
    exact = D.dense(model)["cov"]
    assert np.max(np.abs(res["cov"] - exact)) > 1e-6 * np.max(np.abs(exact))      # the Bethe beliefs, not the exact ones
    dev.close()


# ---- 7. undefined, then exact, then new parameters, then another observed variable; not positive definite -----------------------------
@pytest.mark.parametrize("d", [8, 32])
def test_undefined_then_exact_then_new_parameters(hip_lib, d):
    model = cx.synth.lgssm_chain(7, d=d, seed=81 + d)
    dev = cx.DeviceGraph(dim=d, schedule=L.SCHED_TREE)
    cx.synth.load_into_device(model, dev)
    res = dev.factor_disturbances_mfma()                     # before any sweep
    cnt, n = res["counts"], len(res["factor_ids"])
    assert n == 13 and cnt["rows"] == n and cnt["undefined"] > 0 and cnt["not_positive_definite"] == 0 and cnt["finite"] + cnt["undefined"] == n, cnt
    bad = np.isnan(res["expected_mahalanobis"])
    assert bad.sum() == cnt["undefined"] and np.isnan(res["mean"][bad]).all() and np.isnan(res["cov"][bad]).all() and np.isnan(res["mahalanobis"][bad]).all()
    assert np.isfinite(res["mean"][~bad]).all() and np.isfinite(res["cov"][~bad]).all()
    dev.sweep(1)
    first = _check(dev, model, D.dense(model), f"d {d} old (A, Q)")
    A, Q = model.psets[0]
    A2, Q2 = 0.9 * np.asarray(A), 2.0 * np.asarray(Q)
    dev.set_factor_matrices(0, A2, Q2)
    dev.sweep(1)
    m2 = dataclasses.replace(model, psets={**model.psets, 0: (A2, Q2)})
    second = _check(dev, m2, D.dense(m2), f"d {d} new (A, Q)")      # A, Q⁻¹ and the messages followed
    assert np.max(np.abs(second["cov"] - first["cov"])) > 1e-3
    # another variable is observed: the rows are rebuilt (the transition into x_4 has an observed OUT end now)
    x = m2.x_ids[3]
    facs = np.asarray(m2.edge_fac)[np.asarray(m2.edge_var) == x]
    value = np.random.default_rng(84).standard_normal(d)
    dev.set_messages(np.full(len(facs), x), facs, L.TO_FACTOR, L.FORM_POINT, np.tile(value, (len(facs), 1)))
    dev.sweep(1)
    m3 = dataclasses.replace(m2, data_var=np.concatenate([m2.data_var, np.full(len(facs), x)]), data_fac=np.concatenate([m2.data_fac, facs]),
                             data_y=np.vstack([m2.data_y, np.tile(value, (len(facs), 1))]))
    third = _check(dev, m3, D.dense(m3), f"d {d} x_4 observed")
    assert sum(1 for c in third["cov"] if not np.any(c)) == 1      # its likelihood: both ends observed
    dev.close()


def test_a_factorisation_that_fails_counts_as_not_positive_definite(hip_lib):
    # tests/test_gpu_learn_mfma.py's construction: every stored message defined, then the prior on x_2 becomes negative definite WITHOUT a
    # sweep.  The transition out of x_2 fails in its second stage, the one into it in its first, x_2's likelihood in its only one.
    d = 16
    base = cx.synth.lgssm_chain(5, d=d, seed=77)
    model, f = EM._with_opaque(base, base.x_ids[1:2])
    opq = (base.x_ids[1:2], f, np.zeros((1, d)), np.eye(d)[None])
    dev = cx.DeviceGraph(dim=d, schedule=L.SCHED_TREE)
    cx.synth.load_into_device(model, dev)
    EM.set_opaque(dev, opq)
    dev.sweep(1)
    _check(dev, model, D.dense(model, opaque=opq), "proper prior on x_2")
    EM.set_opaque(dev, (opq[0], opq[1], opq[2], -100.0 * opq[3]))
    res = dev.factor_disturbances_mfma()
    x2 = int(base.x_ids[1])
    touches = np.array([x2 in np.asarray(model.edge_var)[np.asarray(model.edge_fac) == fid].tolist() for fid in res["factor_ids"]])
    assert touches.sum() == 3
    assert res["counts"] == {"rows": len(touches), "finite": len(touches) - 3, "undefined": 0, "not_positive_definite": 3}, res["counts"]
    for k in KEYS:
        assert np.isnan(res[k][touches]).all() and np.isfinite(res[k][~touches]).all(), k
    _close(res["total"], np.sum(res["expected_mahalanobis"][~touches]), 1e-12 * float(np.sum(res["expected_mahalanobis"][~touches])), "the total of the finite rows")
    dev.close()


# ---- 8. determinism and selection -----------------------------------------------------------------------------------------------------
def test_determinism_and_selection(hip_lib):
    d = 20
    model = cx.synth.lgssm_chain(9, d=d, seed=51)
    dev = _dev(model, L.SCHED_TREE)
    full = dev.factor_disturbances_mfma()
    ids = full["factor_ids"]
    assert np.array_equal(ids, np.sort(S.pset_groups(model)[0])) and np.array_equal(ids, dev.factor_disturbance_rows_mfma())
    again = dev.factor_disturbances_mfma()
    assert _bits(full, again) and full["total"] == again["total"]                     # two calls: bit-identical
    alone = dev.factor_disturbances_mfma(rows=False)
    assert "mean" not in alone and "cov" not in alone
    assert _bits(full, alone, KEYS[2:]) and full["total"] == alone["total"] and full["counts"] == alone["counts"]      # out = NULL: the same bits
    for i in (0, 7, len(ids) - 1):                                                      # one factor alone: the bits it has in the full list
        one = dev.factor_disturbances_mfma([ids[i]])
        assert all(one[k][0].tobytes() == full[k][i].tobytes() for k in KEYS) and one["total"] == full["expected_mahalanobis"][i]
    perm = np.random.default_rng(d).permutation(len(ids))
    pick = np.concatenate([perm[:11], perm[:2]])                                        # the caller's order; an id may repeat
    some = dev.factor_disturbances_mfma(ids[pick])
    assert np.array_equal(some["factor_ids"], ids[pick]) and some["counts"]["rows"] == len(pick)
    assert all(some[k].tobytes() == full[k][pick].tobytes() for k in KEYS)
    sc = dev.factor_disturbances_mfma(ids[pick], rows=False)
    assert _bits(some, sc, KEYS[2:]) and some["total"] == sc["total"]
    # the row list honours cap
    n, got = C.c_int64(), np.full(5, -1, np.int64)
    assert dev.lib.cx_factor_disturbance_rows_mfma(dev.h, 3, got.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(n)) == L.OK
    assert n.value == len(ids) and np.array_equal(got[:3], ids[:3]) and np.all(got[3:] == -1)
    assert dev.lib.cx_factor_disturbance_rows_mfma(dev.h, 3, None, C.byref(n)) == L.ERR_INVALID_ARGUMENT
    # an empty list
    none = dev.factor_disturbances_mfma(np.zeros(0, np.int64))
    assert none["mean"].shape == (0, d) and none["counts"]["rows"] == 0 and none["total"] == 0.0
    dev.close()
    # opaque messages are not rows, and the list skips them
    model, opq = EM.prior_chain(16)
    dev = cx.DeviceGraph(dim=16, schedule=L.SCHED_TREE)
    cx.synth.load_into_device(model, dev)
    EM.set_opaque(dev, opq)
    dev.sweep(1)
    assert int(opq[1][0]) not in dev.factor_disturbance_rows_mfma().tolist()
    assert np.array_equal(dev.factor_disturbance_rows_mfma(), O.linear_factors(model))
    dev.close()


def test_auxiliary_residuals_find_a_planted_outlier_on_its_observation_factor(hip_lib):
    d, T, at = 16, 60, 20
    base = cx.synth.lgssm_chain(T, d=d, seed=17)
    y = np.array(base.data_y, float).reshape(T, d)
    y[at] += 8.0 * np.sqrt(np.diag(np.asarray(base.psets[1][1])))      # eight standard deviations of the observation noise
    model = dataclasses.replace(base, data_y=y)
    dev = _dev(model, L.SCHED_CHAIN_SCAN)
    res = _check(dev, model, D.dense(model), "planted outlier")
    z = learn.auxiliary_residuals(res, D.factor_Q(model, res["factor_ids"]))
    assert np.isfinite(z).all()
    big = np.max(np.abs(z), axis=1)
    assert int(res["factor_ids"][int(np.argmax(big))]) == int(np.asarray(base.data_fac)[at]), (int(np.argmax(big)), float(big.max()))
    print(f"largest |z| {big.max():.2f} on the observation factor of y_{at}; the next {np.sort(big)[-2]:.2f}")
    dev.close()


# ---- 9. more rows than waves of a launch and than one chunk of the payload ------------------------------------------------------------------
@pytest.mark.parametrize("T,d", [(600, 64), (8000, 16)])
def test_more_rows_than_waves_and_than_one_chunk(hip_lib, T, d):
    waves, per_chunk = (1024 if d == 64 else 2048), (32 << 20) // (8 * (d + d * d))
    assert 2 * T - 1 > waves and 2 * T - 1 > per_chunk and per_chunk == (1008 if d == 64 else 15420)
    model = cx.synth.lgssm_chain(T, d=d, seed=33)
    dev = _dev(model, L.SCHED_CHAIN_SCAN)
    res = dev.factor_disturbances_mfma()
    n = 2 * T - 1
    assert res["counts"] == {"rows": n, "finite": n, "undefined": 0, "not_positive_definite": 0}, res["counts"]
    fids, sets = S.pset_groups(model)
    mom = M.rts_factor_moments(model)
    for k in (0, 1):      # ids ascend in time within a set
        mine = np.isin(res["factor_ids"], fids[sets == k])
        er, err = mom[k][0], mom[k][2]
        want_c = err - er[:, :, None] * er[:, None, :]
        _close(res["mean"][mine], er, 1e-9, f"d {d} T {T} set {k} means")
        _close(res["cov"][mine], want_c, _scale(want_c), f"d {d} T {T} set {k} covariances")
    _check_scores(res, D.factor_Q(model, res["factor_ids"]), f"d {d} T {T}")
    alone = dev.factor_disturbances_mfma(rows=False)
    assert alone["total"] == res["total"] and _bits(res, alone, KEYS[2:])      # one launch against one per chunk: the same bits
    assert abs(res["total"] - float(np.sum(res["expected_mahalanobis"]))) <= 4 * n * EPS * float(np.sum(res["expected_mahalanobis"]))
    dev.close()


# ---- 10. the embedded-dim rule --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [8, 20])
def test_embedded_dims_give_the_real_models_values_at_any_tile_size(hip_lib, d, monkeypatch):
    model = cx.synth.lgssm_chain(5, d=d, seed=90 + d)
    want = D.dense(model)
    dev = _dev(model, L.SCHED_TREE)
    nat = _check(dev, model, want, f"d {d}, native tile")
    dev.close()
    monkeypatch.setenv("CX_MFMA_DIM", "64")
    dev = _dev(model, L.SCHED_TREE)
    monkeypatch.delenv("CX_MFMA_DIM")
    forced = _check(dev, model, want, f"d {d}, 4 x 4 tiles")
    dev.close()
    for k in KEYS:
        _close(forced[k], nat[k], 1e-12 * max(1.0, float(np.max(np.abs(nat[k])))), f"d {d} forced against native, {k}")


# ---- 11. moves nothing ------------------------------------------------------------------------------------------------------------------
def test_moves_nothing(hip_lib):
    model = cx.synth.lgssm_chain(8, d=16, seed=72)
    fids, _ = S.pset_groups(model)
    want = D.dense(model)
    for s in (L.SCHED_CHAIN_SCAN, L.SCHED_REFERENCE, L.SCHED_TREE):
        dev = _dev(model, s)
        if s == L.SCHED_CHAIN_SCAN:      # (another reader first: every reader of the messages brings them to their slots)
            dev.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE)
        blob, marg, health = dev.export_state(), dev.get_marginals(model.x_ids), dev.message_health()
        st, _ = dev.factor_statistics_mfma(n_groups=2)
        bel = dev.factor_beliefs_mfma(fids)
        plan = dev.ref_plan_stats() if s == L.SCHED_REFERENCE else None
        sweeps = dev.stats()["sweeps_done"]
        _check(dev, model, want, f"schedule {s}")          # the FIRST call: it builds the rows; it works after every schedule
        dev.factor_disturbances_mfma(fids[::-1][:5], rows=False)
        assert np.array_equal(blob, dev.export_state())
        assert np.array_equal(marg, dev.get_marginals(model.x_ids)) and health == dev.message_health()
        st2, _ = dev.factor_statistics_mfma(n_groups=2)      # the statistics between which it was called: bit-identical
        bel2 = dev.factor_beliefs_mfma(fids)
        assert all(st[k].tobytes() == st2[k].tobytes() for k in S.KEYS) and bel[0].tobytes() == bel2[0].tobytes() and bel[1].tobytes() == bel2[1].tobytes()
        assert np.array_equal(blob, dev.export_state())
        if plan is not None:
            assert plan == dev.ref_plan_stats()
        assert sweeps == dev.stats()["sweeps_done"]
        dev.close()
    # fused: the next sweeps are those of a twin handle that never called it, bit for bit
    a, b = _dev(model, L.SCHED_FUSED, 5), _dev(model, L.SCHED_FUSED, 5)
    a.factor_disturbances_mfma()
    a.sweep(3); b.sweep(3)
    assert a.residual() == b.residual()
    assert np.array_equal(a.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE), b.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE), equal_nan=True)
    assert np.array_equal(a.get_marginals(model.x_ids), b.get_marginals(model.x_ids))
    a.close(); b.close()


# ---- 12. refusals -----------------------------------------------------------------------------------------------------------------------
P64, PD = C.POINTER(C.c_int64), C.POINTER(C.c_double)


def _raw(dev, out, sc, tot, c4):
    """every row through the C ABI; the status"""
    return dev.lib.cx_factor_disturbances_mfma(dev.h, 0, None, out.ctypes.data_as(PD), sc.ctypes.data_as(PD), C.byref(tot), c4.ctypes.data_as(P64))


# what assert_reader_refusals asks of this reader.  call: without ids the binding asks cx_factor_disturbance_rows_mfma first; factor 13 is a
# likelihood of its dim 4 chain and the first transition of its dim 16 one.  raw: that chain has 7 rows.  "small call" is skipped: the
# disturbances have no dim 1 .. 4 call (the refusal names cx_factor_statistics, whose sums they are), so none can keep refusing dim 16
_COMMON = dict(who=WHO, small="cx_factor_statistics", call=lambda dev: dev.factor_disturbances_mfma([13]), small_call=None,
               raw=lambda dev: _raw(dev, np.zeros((7, 16 + 256)), np.zeros((7, 2)), C.c_double(), np.zeros(4, np.int64)), skip=("small call",))


def test_refusals(hip_lib):
    assert_reader_refusals(**_COMMON, cases=HANDLE_CASES)
    m2 = cx.synth.lgssm_chain(5, d=2, seed=91)
    m16 = cx.synth.lgssm_chain(4, d=16, seed=92)
    dev = _dev(m2, L.SCHED_TREE)      # dim 2 as well as the helper's dim 4; the row list refuses under its own name
    code, msg = code_of(dev.factor_disturbances_mfma, [1])
    assert code == L.ERR_UNSUPPORTED and msg.startswith(WHO) and "cx_factor_statistics" in msg.replace(WHO, "") and "5 .. 64" in msg, msg
    code, msg = code_of(dev.factor_disturbance_rows_mfma)
    assert code == L.ERR_UNSUPPORTED and msg.startswith("cx_factor_disturbance_rows_mfma"), msg
    dev.close()
    dev = _dev(m16, L.SCHED_TREE)
    code, msg = code_of(dev.factor_disturbances_mfma, [10 ** 6])
    assert code == L.ERR_NOT_FOUND and msg.startswith(WHO) and str(10 ** 6) in msg, msg
    tot, sc = C.c_double(), np.zeros((7, 2))
    assert dev.lib.cx_factor_disturbances_mfma(dev.h, 0, None, None, sc.ctypes.data_as(C.POINTER(C.c_double)), C.byref(tot), None) == L.ERR_INVALID_ARGUMENT
    assert dev.lib.cx_last_error(dev.h).decode().startswith(WHO) and "counts4" in dev.lib.cx_last_error(dev.h).decode()
    one, c4 = np.array([S.pset_groups(m16)[0][0]], np.int64), np.zeros(4, np.int64)
    assert dev.lib.cx_factor_disturbances_mfma(dev.h, -1, one.ctypes.data_as(C.POINTER(C.c_int64)), None, None, None, c4.ctypes.data_as(C.POINTER(C.c_int64))) == L.ERR_INVALID_ARGUMENT
    assert not sc.any()
    dev.close()
    # an opaque factor's id
    model, opq = EM.prior_chain(16)
    dev = cx.DeviceGraph(dim=16, schedule=L.SCHED_TREE)
    cx.synth.load_into_device(model, dev)
    EM.set_opaque(dev, opq)
    dev.sweep(1)
    code, msg = code_of(dev.factor_disturbances_mfma, opq[1])
    assert code == L.ERR_UNSUPPORTED and msg.startswith(WHO) and str(int(opq[1][0])) in msg and "CX_FACTOR_GAUSS_LINEAR" in msg, msg
    dev.close()


def test_refusals_of_a_captured_stream_and_of_parameter_sets_never_set(hip_lib):
    assert_reader_refusals(**_COMMON, cases=STREAM_CASES)
    d = 16
    model = cx.synth.lgssm_chain(5, d=d, seed=93)
    dev = _dev(model, L.SCHED_TREE)
    want = dev.factor_disturbances_mfma()
    n = len(want["factor_ids"])
    out, sc, tot, c4 = np.zeros((n, d + d * d)), np.zeros((n, 2)), C.c_double(), np.zeros(4, np.int64)
    rc, msg = under_capture(dev, lambda: _raw(dev, out, sc, tot, c4))
    assert rc == L.ERR_STATE and msg.startswith(WHO) and "captured" in msg, (rc, msg)
    assert not out.any() and not sc.any() and not c4.any()      # nothing was written
    got = dev.factor_disturbances_mfma()                        # and the handle works on, bit for bit
    assert _bits(want, got) and want["total"] == got["total"]
    dev.close()


# ---- 13. the C++ host class -------------------------------------------------------------------------------------------------------------
def test_cpp_host_class_factor_disturbances_mfma(hip_lib, tmp_path):
    rows = {line.split()[0]: line.split()[1:] for line in run_demo("disturbances_mfma_demo", tmp_path)}
    T, d = 12, 16
    A, Q, R, y = demo_chain(T, d)

    class _Chain:      # what rts_factor_moments reads of a model
        dim, data_y, meta = d, y, {"T": T, "A": A, "Q": Q, "R": R}

    mom = M.rts_factor_moments(_Chain)      # ids: the likelihoods 2T+1 .. 3T, then the transitions 3T+1 .. 4T-1
    er = np.concatenate([mom[1][0], mom[0][0]])
    cr = np.concatenate([mom[1][2], mom[0][2]]) - er[:, :, None] * er[:, None, :]
    Qs = np.concatenate([np.broadcast_to(R, (T, d, d)), np.broadcast_to(Q, (T - 1, d, d))])
    t, q, _ = D.scores(er, cr, Qs)
    n = 2 * T - 1
    assert int(rows["before"][2]) > 0 and rows["counts"] == [str(n), str(n), "0", "0"]
    assert [int(x) for x in rows["ids"]] == list(range(2 * T + 1, 4 * T))
    want = np.concatenate([er, cr.reshape(n, -1)], axis=1).ravel()
    _close(np.array(rows["rows"], float), want, _scale(want), "C++ rows")
    _close(np.array(rows["scores"], float), np.stack([t, q], axis=1).ravel(), 1e-9 * max(1.0, float(np.max(t))), "C++ scores")
    _close(float(rows["total"][0]), float(np.sum(t)), 1e-9 * float(np.sum(t)), "C++ total")
    _close(np.array(rows["one"], float), [t[n - 1], q[n - 1]], 1e-9 * max(1.0, float(t[n - 1])), "C++ scores of the last transition alone")
