"""CPU: what cx_set_factor_offsets_mfma (x_out = A x_in + b + N(0, Q) at dim 5..64) makes the device compute, restated in numpy and pinned
against the model-level references of tests/offsets_support.py before any GPU run: the evidence's term table with g and kappa, the shift
equivalence at these dims, the chain-64 plan with the offsets' space executed record by record, and the M-step on exact statistics."""
import numpy as np
import pytest

from cortex.jl_amd import learn
from tests import anisotropic as AN
from tests import evidence_support as E
from tests import general_mfma_support as G
from tests import learning_support as LS
from tests import offsets_mfma_support as OM
from tests import offsets_support as O

TOL = 1e-10


def _close(a, b, what, tol=TOL):
    a, b = np.asarray(a, float), np.asarray(b, float)
    err = float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0)))
    assert err <= tol, (what, err)


MODELS = {"chain": G.chain, "comb": G.comb, "clamped": G.clamped}


@pytest.mark.parametrize("d", [5, 17])
@pytest.mark.parametrize("name", MODELS)
def test_the_term_table_with_offsets_is_the_joint_solves_log_z(name, d):
    """the terms k_evm_terms evaluates (uncentred; kFacFree, kFacObs with either end observed, kFacBoth on the clamped chain) on the
    messages of numpy BP, against the joint solve's log Z at 1e-10 relative"""
    model = MODELS[name](d)
    b = O.with_offsets(model, 21)
    gm = O.gmodel_offsets(model, b)
    f2v = E.numpy_bp(gm)
    got, want = OM.term_table_log_z(gm, f2v), O.joint_solve_offsets(model, b)[3]
    assert abs(got - want) <= TOL * abs(want), (name, d, got, want)
    # the offsets matter, and the table without them is the model without them
    z0 = OM.term_table_log_z(E.gmodel(model), E.numpy_bp(E.gmodel(model)))
    assert abs(z0 - AN.joint_solve(model)[3]) <= TOL * abs(z0) and abs(z0 - want) > 0.1


@pytest.mark.parametrize("d", [5, 17])
@pytest.mark.parametrize("name", ["chain", "ring"])
def test_consistent_offsets_are_a_shift(name, d):
    model = G.chain(d) if name == "chain" else G.ring(d)
    b, s = O.consistent_offsets(model, 7)
    twin, _ = O.shifted_twin(model, b, s)
    mean, S, pos, log_z = O.joint_solve_offsets(model, b)
    tm, tS, tpos, tz = AN.joint_solve(twin)
    assert pos == tpos
    shift = np.concatenate([s[v] for v in sorted(pos, key=pos.get)])
    _close(mean, tm + shift, f"{name} d={d}: the means differ by s")
    _close(S, tS, f"{name} d={d}: covariances")
    _close(log_z, tz, f"{name} d={d}: log Z")


def test_linear_terms_are_the_rule_tables_times_b():
    """g_out = C b of the triple towards OUT, g_in = -B b of the triple towards IN, kappa = b'C b = b'P b of the two: what
    k_offset_terms64 reads from the tables"""
    d = 5
    A, Q, _, _ = AN.general_sets(d, 3)
    b = np.random.default_rng(4).standard_normal(d)
    Qi = np.linalg.inv(Q)
    to_out = (A.T @ Qi @ A, Qi @ A, Qi)          # (P, B, C) of the messages into the OUT end
    to_in = (Qi, A.T @ Qi, A.T @ Qi @ A)
    g_out, g_in, kappa = OM.linear_terms(A, Q, b)
    _close(g_out, to_out[2] @ b, "g_out")
    _close(g_in, -to_in[1] @ b, "g_in")
    _close(kappa, b @ to_out[2] @ b, "kappa from the triple towards OUT")
    _close(kappa, b @ to_in[0] @ b, "kappa from the triple towards IN")


@pytest.mark.parametrize("K0,fan", [(2, 2), (0, 4)])
def test_chain64_plan_with_the_offsets_space(K0, fan):
    """T = 9 at block length 2 and fan 2: three levels of walks (the top walk over 2 groups, the groups' walks over 4 blocks, the blocks'
    links) on two levels of composed potentials; the default block length (4): two blocks and one top walk.  The links' h and c name the g rows of their
    two slots; the executed plan leaves the exact messages of the model with offsets"""
    d, T = 16, 9
    model = AN.chain(T, d)
    b = O.with_offsets(model, 31)
    g = OM.chain_offsets_inputs(model, b)
    plan = OM.OffsetsPlan64(d, g["link_pos"], g["frm"], g["to"], g["tab_fwd"], g["tab_bwd"], g["head_f"], g["head_b"], g["side"], K0=K0, fan=fan)
    if K0 == 2:
        assert plan.levels == 2 and len(plan.walk_launches) == 3 and [len(j) for j in plan.compose_launches] == [4, 2]
    else:
        assert plan.K0 == 4 and plan.levels == 1 and plan.n_pot == 2
    spaces = {OM.split(h)[0] for h in np.concatenate([plan.children[:, 4:6].ravel(), plan.steps[:, 6:8].ravel()])}
    assert "off" in spaces
    mem = {"zero": np.zeros(plan.msg), "f2v": g["f2v"].reshape(-1), "ptab": g["ptab"], "btab": g["btab"],
           "pot": np.full(max(1, plan.n_pot) * plan.pot, np.nan), "ent": np.full(max(1, plan.n_ent) * plan.msg, np.nan), "off": g["goff"].reshape(-1)}
    OM.run_plan_offsets(plan, mem, d)
    f2v, npos, nlinks = g["f2v"], g["npos"], g["nlinks"]
    assert not np.isnan(f2v).any()
    em, ecov = O.dense_posterior_offsets(model, b)
    for t in range(T):
        rows = [f2v[t]] + ([f2v[npos + t - 1]] if t > 0 else []) + ([f2v[npos + nlinks + t]] if t < T - 1 else [])
        eta, lam = sum(r[:d] for r in rows), sum(r[d:].reshape(d, d) for r in rows)
        cov = np.linalg.inv(lam)
        _close(cov, ecov[t], f"covariance of state {t}", 1e-9)
        _close(cov @ eta, em[t], f"mean of state {t}", 1e-9)
    # without offsets the same inputs give the plan as it always was: no record names the space
    plain = OM.H.Plan64(d, g["link_pos"], g["frm"], g["to"], g["tab_fwd"], g["tab_bwd"], g["head_f"], g["head_b"], g["side"], K0=K0, fan=fan)
    assert all(OM.split(h)[0] != "off" for h in np.concatenate([plain.children[:, :9].ravel(), plain.steps[:, :9].ravel()]))
    assert np.array_equal(plain.children[:, :4], plan.children[:, :4]) and np.array_equal(plain.steps[:, :6], plan.steps[:, :6])


def test_m_step_on_exact_statistics_recovers_a_planted_drift_at_d8():
    """the arithmetic em_mfma's loop relies on, at the dim of its GPU test: statistics of n exact (residual, input) pairs taken under
    (A0, b0) when the truth is (A*, b*) — r = x_out - A0 x_in - b0, the form cx_factor_statistics_mfma accumulates — and one
    learn.m_step with ("A", "b", "Q") lands on the truth; "b" alone moves b by the mean residual"""
    rng = np.random.default_rng(43)
    d, n = 8, 199
    A_true, b_true = 0.4 * rng.standard_normal((d, d)), rng.standard_normal(d)
    A0, b0 = A_true + 0.1 * rng.standard_normal((d, d)), 0.3 * rng.standard_normal(d)
    x = rng.standard_normal((n, d))
    z = np.hstack([x, np.ones((n, 1))])
    noise = 0.05 * rng.standard_normal((n, d))
    noise -= z @ np.linalg.lstsq(z, noise, rcond=None)[0]      # orthogonal to [x, 1]: the regression is exact
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


def test_statistics_with_offsets_use_the_factors_own_b():
    """the reference the GPU test compares cx_factor_statistics_mfma with: from the dense beliefs of a chain whose transitions carry
    different b, sum_r of the transitions' group is the sum of E[x_out] - A E[x_in] - b_f, factor by factor"""
    d = 5
    model = G.chain(d)
    b = O.with_offsets(model, 45)
    gm = O.gmodel_offsets(model, b)
    fids, sets = LS.pset_groups(model)
    st = LS.grouped_statistics(gm, fids, sets, 2)
    means, _ = LS.dense_factor_beliefs(gm, fids)
    A = np.asarray(model.psets[0][0])
    want = sum(means[i, :d] - A @ means[i, d:] - b[int(f)] for i, f in enumerate(fids) if sets[i] == 0)
    _close(st["sum_r"][0], want, "sum_r of the transitions")
