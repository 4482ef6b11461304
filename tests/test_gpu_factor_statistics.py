"""-m gpu: cx_factor_beliefs / cx_factor_statistics and learn.em against the dense posterior, the RTS smoother,
central differences of cx_log_evidence (Fisher's identity) and Shumway–Stoffer EM (tests/learning_support.py, pinned by
tests/test_learning_checker.py)."""

import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from cortex.jl_amd import learn
from tests import evidence_support as E
from tests import learning_support as S
from tests.gpu_support import code_of, iterative_device, run_demo
from tests.learning_support import assert_rel_close as _close

pytestmark = pytest.mark.gpu


def _pair_fids(gm):
    return gm.groups[2]["fid"]


def _check_beliefs(dev, gm, what):
    fids = _pair_fids(gm)
    got_m, got_c = dev.factor_beliefs(fids)
    want_m, want_c = S.dense_factor_beliefs(gm, fids)
    _close(got_m, want_m, 1e-9, what + " means")
    _close(got_c, want_c, 1e-9 * max(1.0, float(np.max(np.abs(want_c)))), what + " covariances")


def _pairwise_tree(seed):
    """a tree_model whose factors all have two variables (ADDITIVE / LINEAR), with observed leaves and opaque priors"""
    return cx.synth.tree_model(50, seed=seed, k_choices=(1,), observe=0.2)


DIM1 = [("ssm_chain_linear", lambda: cx.synth.ssm_chain_linear(80, seed=201), 300, True),
        ("tree_model", lambda: _pairwise_tree(202), 200, False)]


@pytest.mark.parametrize("name,make,n_iter,chain", DIM1, ids=[c[0] for c in DIM1])
def test_dim1_beliefs_match_the_dense_posterior(hip_lib, name, make, n_iter, chain):
    model = make()
    gm = E.gmodel(model)
    assert set(gm.groups) == {2}
    for s in [L.SCHED_TREE, L.SCHED_REFERENCE, L.SCHED_FUSED] + ([L.SCHED_CHAIN_SCAN] if chain else []):
        dev = iterative_device(model, s, n_iter)
        _check_beliefs(dev, gm, f"{name} schedule {s}")
        dev.close()


@pytest.mark.parametrize("d", [2, 3, 4])
def test_dims_2_to_4_beliefs_match_the_dense_posterior(hip_lib, d):
    models = [("lgssm_chain", cx.synth.lgssm_chain(40, d=d, seed=210 + d), True), ("lgssm_comb", cx.synth.lgssm_comb(10, d=d, teeth=1, seed=220 + d), False)]
    for name, model, chain in models:
        gm = E.gmodel(model)
        for s in [L.SCHED_TREE, L.SCHED_REFERENCE, L.SCHED_FUSED] + ([L.SCHED_CHAIN_SCAN] if chain else []):
            dev = iterative_device(model, s, 200)
            _check_beliefs(dev, gm, f"d {d} {name} schedule {s}")
            dev.close()


def _check_stats(got, cnt, want, n_counted, n_groups_used, what):
    for k in S.KEYS:
        scale = max(1.0, float(np.max(np.abs(want[k])))) if k in ("S_xx", "sum_x") else 1.0
        _close(got[k], want[k], 1e-9 * scale, f"{what} {k}")
    assert cnt == {"factors": n_counted, "groups": n_groups_used, "undefined": 0, "not_positive_definite": 0}, (what, cnt)


@pytest.mark.parametrize("d", [2, 3, 4])
def test_statistics_by_parameter_set_and_by_explicit_groups(hip_lib, d):
    model = cx.synth.lgssm_chain(50, d=d, seed=230 + d)
    gm = E.gmodel(model)
    fids, sets = S.pset_groups(model)
    for s in (L.SCHED_CHAIN_SCAN, L.SCHED_TREE):
        dev = iterative_device(model, s)
        got, cnt = dev.factor_statistics(n_groups=3)                         # set 2 unused: a zero row
        want = S.grouped_statistics(gm, fids, sets, 3)
        _check_stats(got, cnt, want, len(fids), 2, f"d {d} sets schedule {s}")
        assert got["n"][2] == 0 and not np.any(got["S_rr"][2])
        # explicit: the transitions split into two groups by parity, every third factor skipped, the likelihoods in group 3
        rng = np.random.default_rng(d)
        groups = np.where(sets == 0, 1 + (np.arange(len(fids)) % 2), 3)
        groups[rng.random(len(fids)) < 0.3] = -1
        perm = rng.permutation(len(fids))                                   # the caller's order does not matter
        got, cnt = dev.factor_statistics(fids[perm], groups[perm], n_groups=5)
        want = S.grouped_statistics(gm, fids, groups, 5)
        _check_stats(got, cnt, want, int((groups >= 0).sum()), 3, f"d {d} explicit schedule {s}")
        dev.close()


def test_dim1_statistics_with_explicit_groups(hip_lib):
    model = cx.synth.ssm_chain_linear(60, seed=240)
    gm = E.gmodel(model)
    T = 60
    lik, tr = np.arange(2 * T + 1, 3 * T + 1), np.arange(3 * T + 1, 4 * T)
    dev = iterative_device(model, L.SCHED_CHAIN_SCAN)
    # the likelihoods (ADDITIVE) share (kind, 1, 0); each transition has its own (a, b): one group each, a few skipped
    fids = np.concatenate([lik, tr])
    groups = np.concatenate([np.zeros(T, np.int64), 1 + np.arange(T - 1)])
    groups[T + 3] = groups[T + 10] = -1
    got, cnt = dev.factor_statistics(fids, groups, n_groups=T)
    want = S.grouped_statistics(gm, fids, groups, T)
    _check_stats(got, cnt, want, 2 * T - 3, T - 2, "dim 1 explicit")
    dev.close()


def test_fisher_identity(hip_lib):
    for d in (2, 3):
        model = cx.synth.lgssm_chain(200, d=d, seed=250 + d)
        A0, Q0 = model.meta["A"] * 0.97, model.meta["Q"] * 1.3
        dev = cx.DeviceGraph(dim=d, schedule=L.SCHED_CHAIN_SCAN)
        cx.synth.load_into_device(model, dev)

        def ll(A, Q):
            dev.set_factor_matrices(0, A, Q)
            dev.sweep(1)
            return dev.log_evidence()[0]

        ll(A0, Q0)
        st, _ = dev.factor_statistics(n_groups=2)
        g = learn.group(st, 0)
        Qi = np.linalg.inv(Q0)
        gA = Qi @ g["S_rx"]
        gQ = 0.5 * Qi @ (g["S_rr"] - g["n"] * Q0) @ Qi
        h = 1e-5
        fdA, fdQ = np.zeros((d, d)), np.zeros((d, d))
        for i in range(d):
            for j in range(d):
                E_ = np.zeros((d, d)); E_[i, j] = h
                fdA[i, j] = (ll(A0 + E_, Q0) - ll(A0 - E_, Q0)) / (2 * h)
                if j >= i:
                    Es = np.zeros((d, d)); Es[i, j] = Es[j, i] = h
                    fdQ[i, j] = fdQ[j, i] = (ll(A0, Q0 + Es) - ll(A0, Q0 - Es)) / (2 * h)
        gQs = gQ + gQ.T - np.diag(np.diag(gQ))                               # d/dQ_ij of a symmetric Q moves Q_ij and Q_ji together
        assert np.max(np.abs(fdA - gA)) <= 1e-5 * np.max(np.abs(gA)), (d, fdA, gA)
        assert np.max(np.abs(fdQ - gQs)) <= 1e-5 * np.max(np.abs(gQs)), (d, fdQ, gQs)
        dev.close()


@pytest.mark.parametrize("d", [2, 4])
def test_em_matches_shumway_stoffer(hip_lib, d):
    T = 2000
    model = cx.synth.lgssm_chain(T, d=d, seed=260 + d)
    rng = np.random.default_rng(d)
    A0 = model.meta["A"] + 0.05 * rng.standard_normal((d, d))
    Q0, C0, R0 = 2.0 * model.meta["Q"], np.eye(d) + 0.05 * rng.standard_normal((d, d)), 0.5 * model.meta["R"]
    y = np.asarray(model.data_y).reshape(T, d)
    want_trace, want_params = S.ss_em(y, A0, Q0, C0, R0, n_iter=20)
    dev = cx.DeviceGraph(dim=d, schedule=L.SCHED_CHAIN_SCAN)
    cx.synth.load_into_device(model, dev)
    trace, params = learn.em(dev, {0: (A0, Q0), 1: (C0, R0)}, n_iter=20)
    assert np.all(np.diff(trace) >= -1e-9 * abs(trace[-1])), np.diff(trace)
    _close(trace, want_trace, 1e-7, "trace")
    A, Q, C, R = want_params[-1]
    scale = lambda M: 1e-7 * max(1.0, float(np.max(np.abs(M))))
    for got, want, what in ((params[0][0], A, "A"), (params[0][1], Q, "Q"), (params[1][0], C, "C"), (params[1][1], R, "R")):
        assert np.max(np.abs(got - want)) <= scale(want), (what, got, want)
    dev.close()


def test_dim1_em_rebuilding_the_handle(hip_lib):
    # ssm_chain: the likelihoods (y_t, x_t) and the transitions are ADDITIVE (no a to learn): r and q only, two groups
    T = 500
    model = cx.synth.ssm_chain(T, seed=270, q=1.0, r=1.0)
    y = np.asarray(model.data_y, float).reshape(T, 1)
    q, r = 3.0, 0.3
    want_trace, want_params = S.ss_em(y, np.eye(1), q * np.eye(1), np.eye(1), r * np.eye(1), n_iter=10, learn=("Q", "R"))
    lik, tr = np.arange(2 * T + 1, 3 * T + 1), np.arange(3 * T + 1, 4 * T)
    fids = np.concatenate([lik, tr])
    groups = np.concatenate([np.zeros(T, np.int64), np.ones(T - 1, np.int64)])
    trace = []
    for it in range(11):
        model.factor_var = np.concatenate([np.full(T, r), np.full(T - 1, q)])
        dev = iterative_device(model, L.SCHED_CHAIN_SCAN)
        trace.append(dev.log_evidence()[0])
        st, cnt = dev.factor_statistics(fids, groups)
        dev.close()
        assert cnt["factors"] == 2 * T - 1 and cnt["groups"] == 2
        if it == 10:
            break
        r = learn.m_step(learn.group(st, 0), [[1.0]], learn=("Q",))["Q"][0, 0]
        q = learn.m_step(learn.group(st, 1), [[1.0]], learn=("Q",))["Q"][0, 0]
    assert np.all(np.diff(trace) >= -1e-9 * abs(trace[-1])), np.diff(trace)
    _close(trace, want_trace, 1e-7, "trace")
    assert abs(q - want_params[-1][1][0, 0]) <= 1e-7 * q and abs(r - want_params[-1][3][0, 0]) <= 1e-7 * r, (q, r, want_params[-1])


def test_determinism_and_no_side_effects(hip_lib):
    model = cx.synth.lgssm_chain(300, d=4, seed=280)
    dev = iterative_device(model, L.SCHED_CHAIN_SCAN)
    before, _ = dev.log_evidence()
    blob = dev.export_state()
    a, ca = dev.factor_statistics(n_groups=2)
    b, cb = dev.factor_statistics(n_groups=2)
    fids = np.asarray(model.factor_ids)
    m1, c1 = dev.factor_beliefs(fids)
    m2, c2 = dev.factor_beliefs(fids)
    for k in S.KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert ca == cb and m1.tobytes() == m2.tobytes() and c1.tobytes() == c2.tobytes()
    assert np.array_equal(blob, dev.export_state())
    after, _ = dev.log_evidence()
    assert np.float64(before).tobytes() == np.float64(after).tobytes()
    dev.close()
    # fused: the next sweeps are those of a twin handle that never called them
    model = cx.synth.tree_model(40, seed=281, k_choices=(1,), observe=0.2)
    x, y = iterative_device(model, L.SCHED_FUSED, 5), iterative_device(model, L.SCHED_FUSED, 5)
    fids = E.gmodel(model).groups[2]["fid"]
    x.factor_beliefs(fids)
    x.factor_statistics(fids, np.arange(len(fids)))                          # (dim 1: one group per factor shares its a trivially)
    x.sweep(3); y.sweep(3)
    assert np.array_equal(x.get_marginals(model.x_ids), y.get_marginals(model.x_ids))
    x.close(); y.close()


def test_undefined_states_are_nan(hip_lib):
    model = cx.synth.lgssm_chain(30, d=2, seed=290)
    dev = cx.DeviceGraph(dim=2, schedule=L.SCHED_TREE)
    cx.synth.load_into_device(model, dev)
    st, cnt = dev.factor_statistics(n_groups=2)                              # before any sweep
    assert cnt["undefined"] > 0 and cnt["factors"] == 59 and cnt["groups"] == 2
    assert np.isnan(st["S_rr"]).all() and np.array_equal(st["n"], [29.0, 30.0])
    m, c = dev.factor_beliefs(model.factor_ids[:3])
    assert np.isnan(m).all() and np.isnan(c).all()
    dev.sweep(1)
    st, cnt = dev.factor_statistics(n_groups=2)
    assert cnt["undefined"] == 0 and np.isfinite(st["S_rr"]).all()
    dev.close()


def test_refusals(hip_lib):
    dev = cx.DeviceGraph(dim=2)
    assert code_of(dev.factor_statistics, n_groups=1)[0] == L.ERR_STATE                                # no graph
    dev.close()
    dev = cx.DeviceGraph(family=L.FAMILY_NATURAL2)
    code, msg = code_of(dev.factor_beliefs, [1])
    assert code == L.ERR_UNSUPPORTED and "Gaussian family" in msg
    dev.close()
    m16 = cx.synth.lgssm_chain(4, d=16, seed=291)
    dev = iterative_device(m16, L.SCHED_FUSED, 2)
    code, msg = code_of(dev.factor_statistics, n_groups=2)
    assert code == L.ERR_UNSUPPORTED and "dim 1, 2, 3 and 4" in msg
    dev.close()
    model = cx.synth.ssm_chain(20, seed=292)
    dev = iterative_device(model, L.SCHED_FUSED, 5)
    code, msg = code_of(dev.factor_statistics, n_groups=2)                                            # dim 1 without groups
    assert code == L.ERR_INVALID_ARGUMENT and "name the factors" in msg
    code, msg = code_of(dev.factor_beliefs, [999])
    assert code == L.ERR_NOT_FOUND and "999" in msg
    dev.halo_configure([1], [2 * 20 + 1], [], [])                                                   # a partitioned handle
    code, msg = code_of(dev.factor_beliefs, [41])
    assert code == L.ERR_UNSUPPORTED and "partitioned" in msg
    dev.close()
    # a group whose factors do not share a
    model = cx.synth.ssm_chain_linear(20, seed=293)
    dev = iterative_device(model, L.SCHED_TREE)
    code, msg = code_of(dev.factor_statistics, [61, 62], [0, 0], n_groups=1)
    assert code == L.ERR_INVALID_ARGUMENT and "61" in msg and "62" in msg
    code, msg = code_of(dev.factor_statistics, [61, 61], [0, 0], n_groups=1)
    assert code == L.ERR_INVALID_ARGUMENT and "twice" in msg
    code, msg = code_of(dev.factor_statistics, [61], [1], n_groups=1)
    assert code == L.ERR_INVALID_ARGUMENT
    dev.close()
    # zero noise
    model = cx.synth.ssm_chain(10, seed=294, q=0.0)
    dev = cx.DeviceGraph(schedule=L.SCHED_TREE)
    cx.synth.load_into_device(model, dev)
    code, msg = code_of(dev.factor_beliefs, [31])
    assert code == L.ERR_UNSUPPORTED and "factor 31" in msg and "zero noise" in msg
    dev.close()
    # dim 2: n_groups too small; a set shared with a factor of more than two variables; a k-ary factor named
    model = cx.synth.lgssm_chain(10, d=2, seed=295)
    dev = iterative_device(model, L.SCHED_TREE)
    code, msg = code_of(dev.factor_statistics, n_groups=1)
    assert code == L.ERR_INVALID_ARGUMENT and "n_groups" in msg
    dev.close()
    # x_2 = A x_1 + w (set 0) next to x_3 = A x_1 + A x_2 + w (a CX_FACTOR_GAUSS_LINEAR_N factor reading set 0 too)
    dev = cx.DeviceGraph(dim=2, schedule=L.SCHED_TREE)
    dev.set_factor_matrices(0, 0.5 * np.eye(2), np.eye(2))
    dev.graph_create(np.array([1, 2, 3, 1, 2]), np.array([10, 10, 11, 11, 11]), np.array([10, 11]),
                     np.array([L.FACTOR_GAUSS_LINEAR, L.FACTOR_GAUSS_LINEAR_N], np.int32), np.array([0.0, 0.0]),
                     edge_role=np.array([L.ROLE_IN, L.ROLE_OUT, L.ROLE_OUT, L.ROLE_IN, L.ROLE_IN], np.int32))
    code, msg = code_of(dev.factor_statistics, n_groups=1)
    assert code == L.ERR_UNSUPPORTED and "more than two variables" in msg
    code, msg = code_of(dev.factor_beliefs, [11])
    assert code == L.ERR_UNSUPPORTED and "factor 11" in msg
    code, msg = code_of(dev.factor_statistics, [11], [0], n_groups=1)
    assert code == L.ERR_UNSUPPORTED and "factor 11" in msg
    dev.close()


def test_cpp_host_class_factor_statistics(hip_lib, tmp_path):
    out_lines = run_demo("learn_demo", tmp_path)
    rows = {line.split()[0]: [float(v) for v in line.split()[1:]] for line in out_lines}
    T = 50
    model = cx.synth.ssm_chain(T, seed=1)
    model.data_y = np.array([0.5 * t + (7 * t) % 5 for t in range(1, T + 1)], dtype=np.float64)
    gm = E.gmodel(model)
    lik, tr = np.arange(2 * T + 1, 3 * T + 1), np.arange(3 * T + 1, 4 * T)
    fids = np.concatenate([lik, tr])
    groups = np.concatenate([np.zeros(T, np.int64), np.ones(T - 1, np.int64)])
    want = S.grouped_statistics(gm, fids, groups, 2)
    flat = np.concatenate([np.concatenate([[want["n"][g]], want["sum_r"][g], want["sum_x"][g], want["S_rr"][g].ravel(),
                                           want["S_rx"][g].ravel(), want["S_xx"][g].ravel()]) for g in range(2)])
    _close(rows["stats"], flat, 1e-9 * max(1.0, float(np.max(np.abs(flat)))), "C++ statistics")
    assert rows["counts"] == [2 * T - 1, 2, 0, 0]
    bm, bc = S.dense_factor_beliefs(gm, [3 * T + 1])
    _close(rows["belief"], np.concatenate([bm[0], bc[0].ravel()]), 1e-9, "C++ belief")
