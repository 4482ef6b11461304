"""CPU: the checkers of the d-dimensional kernels on GENERAL matrices (tests/anisotropic.py).

The default models are isotropic — A = rho * orthogonal, Q = q I, R = r I, H = I, seeds N(0, s I) — so every covariance any checker or
kernel ever formed on them was a multiple of the identity.  Here: (a) the general models are not vacuous (off-diagonal posterior
covariances, non-normal A, non-symmetric H, cond(Q), cond(R) in [5, 50], an f64 reference good to 1e-13), (b) oracle/mv.py, oracle/mv_flood.c
and the dense numbers of the readers' support modules agree with a joint solve that shares no code with them, (c) a restatement with the
forward covariance A' S A + Q instead of A S A' + Q passes on the default chain and fails on the general one — the gap the GPU cases of
tests/test_gpu_anisotropic.py close —, (d) the loopy reference converges within the sweep count the GPU test uses."""
import functools

import numpy as np
import pytest

import cortex.jl_amd as cx
from oracle import exact
from oracle.mv import MvFlood, MvFloodC
from tests import anisotropic as AN
from tests import evidence_support as E
from tests import functional_support as F
from tests import learning_support as LS
from tests import predictive_support as P
from tests import sampling_support as SS


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(float(np.max(np.abs(b))), 1e-300))


# ---- (a) the generator is not vacuous ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(AN.gpu_models()))
def test_every_model_of_the_gpu_tests_has_off_diagonal_work(name):
    model = AN.gpu_models()[name]()
    d = model.dim
    A, Q, R, H = (model.meta[k] for k in "AQRH")
    _, cov = AN.chain_posterior(model) if model.meta.get("kind") == "lgssm_chain" else AN.dense_posterior(model)
    assert AN.offdiag_ratio(cov) >= 0.1, "posterior covariances are (nearly) diagonal"
    assert np.linalg.norm(A @ A.T - A.T @ A) >= 0.1, "A is (nearly) normal: A S A' and A' S A would agree"
    if not np.array_equal(H, np.eye(d)):
        assert np.linalg.norm(H - H.T) >= 0.1, "H is (nearly) symmetric"
    for M in [Q, R] + [q for k, (_, q) in model.psets.items() if k >= 2]:
        assert 5.0 <= np.linalg.cond(M) <= 50.0
    assert _f64_vs_long_double(d, model.meta["seed"]) <= 1e-13


@functools.lru_cache(maxsize=None)
def _f64_vs_long_double(d, seed):
    """the f64 smoother against the long-double one on a chain of the A, Q, R of (d, seed) (the long-double recursion has no H)"""
    m = AN.chain(20 if d <= 16 else 9, d, seed=seed, general_h=False)
    A, Q, R = (m.meta[k] for k in "AQR")
    m64, c64 = exact.lgssm_posterior(m.data_y, A, Q, R)
    mld, cld = exact.lgssm_posterior_longdouble(m.data_y, A, Q, R)
    return max(_rel(m64, mld), _rel(c64, cld))


@pytest.mark.parametrize("d", [2, 3, 4, 7, 16, 24, 32, 64])
def test_the_recipe_at_every_dimension(d):
    """the acceptance figures of the recipe: singular values and eigenvalues as stated, non-normality 0.5 .. 2.5, and for d >= 3 a
    mid-chain posterior covariance with off-diagonals of 0.15 .. 0.5 of the diagonal"""
    A, Q, R, H = AN.general_sets(d, AN.seed_of(d))
    assert np.allclose(np.linalg.svd(A, compute_uv=False), np.linspace(0.4, 0.95, d)[::-1])
    assert np.allclose(np.linalg.eigvalsh(Q), np.geomspace(0.05, 1.0, d)) and np.allclose(np.linalg.eigvalsh(R), np.geomspace(0.3, 3.0, d))
    assert np.allclose(np.linalg.svd(H, compute_uv=False), np.linspace(0.6, 1.5, d)[::-1])
    assert np.array_equal(Q, Q.T) and np.array_equal(R, R.T)
    assert 0.5 <= np.linalg.norm(A @ A.T - A.T @ A) <= 2.5
    m = AN.chain(9 if d > 16 else 20, d, general_h=False)
    _, cov = AN.chain_posterior(m)
    mid = cov[len(cov) // 2]
    assert 0.15 <= AN.offdiag_ratio(mid[None]) <= 0.5


# ---- (b) the oracles on general matrices ------------------------------------------------------------------------------------------------
def _pin_flood_pair(model, sweeps):
    a, b = MvFlood(model), MvFloodC(model)
    for sweep in range(sweeps):
        a.sweep(1); b.sweep(1)
        for e in range(a.g.ne):
            for name in ("f2v", "v2f"):
                x, y = getattr(a, name)[e], getattr(b, name)[e]
                assert (x is None) == (y is None), f"sweep {sweep} edge {e} {name}: definedness differs"
                if x is None or not np.all(np.isfinite(x[1])) or np.linalg.cond(x[1]) > 1e10:
                    continue     # (improper message towards an observed variable: nobody reads it)
                np.testing.assert_allclose(y[0], x[0], rtol=0, atol=1e-9 * max(1.0, float(np.max(np.abs(x[0])))))
                np.testing.assert_allclose(y[1], x[1], rtol=0, atol=1e-9 * max(1.0, float(np.max(np.abs(x[1])))))
    return b


def _fixed_point_vs_joint(o, model):
    m, S, ok = o.marginals()
    xs = np.searchsorted(o.g.var_ids, model.x_ids)
    assert ok[xs].all()
    em, ecov = AN.dense_posterior(model)
    np.testing.assert_allclose(m[xs], em, rtol=0, atol=1e-9 * np.max(np.abs(em)))
    np.testing.assert_allclose(S[xs], ecov, rtol=0, atol=1e-9 * np.max(np.abs(ecov)))


@pytest.mark.parametrize("d,T", [(2, 7), (3, 9), (4, 9), (7, 5)])
def test_c_checker_equals_numpy_restatement_on_a_general_chain(d, T):
    model = AN.chain(T, d)
    o = _pin_flood_pair(model, T + 2)
    _fixed_point_vs_joint(o, model)
    em, ecov = AN.dense_posterior(model)
    cm, ccov = AN.chain_posterior(model)
    assert _rel(cm, em) <= 1e-12 and _rel(ccov, ecov) <= 1e-12, "block-tridiagonal smoother with H vs the joint solve"


def test_c_checker_on_a_general_branching_tree():
    model = AN.branching(13, 3, b=3)
    o = _pin_flood_pair(model, 8)
    _fixed_point_vs_joint(o, model)


def test_c_checker_on_a_general_multi_sensor_chain_and_a_comb():
    for model, sweeps in ((AN.multi_sensor(6, 4, sensors=3), 9), (AN.comb(6, 2, teeth=1), 10)):
        o = _pin_flood_pair(model, sweeps)
        _fixed_point_vs_joint(o, model)


def _reader_models():
    for d in (2, 3, 4):
        yield f"chain d={d}", AN.chain(60, d), True
        yield f"comb d={d}", AN.comb(15, d, teeth=1), False


def _joint_maps(model, gm):
    """the joint solve of tests/anisotropic.py in the variable order of the GModel: (mean [nv, d], S, fpos as learning_support's, log Z)"""
    d = gm.d
    mean, S, pos, log_z = AN.joint_solve(model)
    free = np.flatnonzero(~gm.obs)
    assert [pos[int(v)] for v in gm.var_ids[free]] == list(range(len(free))), "both order the latent variables by ascending id"
    m = gm.y.copy()
    m[free] = mean.reshape(len(free), d)
    return m, S, log_z


@pytest.mark.parametrize("name,model,is_chain", [pytest.param(n, m, c, id=n) for n, m, c in _reader_models()])
def test_dense_numbers_of_the_reader_support_modules(name, model, is_chain):
    """evidence_support, learning_support, predictive_support, sampling_support and functional_support state their dense numbers over one
    GModel; on general A, Q, R, H each must equal the joint solve assembled straight from the model — each at its own checker's tolerance"""
    gm = E.gmodel(model)
    d = gm.d
    jm, jS, jlz = _joint_maps(model, gm)
    A, Q, R, H = (model.meta[k] for k in "AQRH")
    # evidence: dense log Z, the Bethe formula from exact messages, and on the chain the Kalman filter with observation matrix H
    dense = E.dense_log_z(gm)
    assert abs(dense - jlz) <= 1e-10 * abs(jlz)
    f2v = F.forest_bp(gm)
    assert abs(E.bethe_log_z(gm, f2v) - jlz) <= 1e-10 * abs(jlz)
    if is_chain:
        ll, ms, Ps, Pc = LS.rts(A, Q, H, R, model.data_y)
        assert abs(ll - jlz) <= 1e-10 * abs(jlz)
    # learning: the posterior and every factor belief
    mean, S, fpos = LS.dense_posterior(gm)
    assert _rel(mean, jm) <= 1e-10 and _rel(S, jS) <= 1e-10
    g = gm.groups[2]
    means, covs = LS.dense_factor_beliefs(gm)
    for r, vs in enumerate(g["vars"]):
        assert _rel(means[r], np.concatenate([jm[vs[0]], jm[vs[1]]])) <= 1e-10
        for a in range(2):
            for c in range(2):
                pa, pc = fpos[vs[a]], fpos[vs[c]]
                want = jS[pa * d:(pa + 1) * d, pc * d:(pc + 1) * d] if pa >= 0 and pc >= 0 else np.zeros((d, d))
                assert np.max(np.abs(covs[r, a * d:(a + 1) * d, c * d:(c + 1) * d] - want)) <= 1e-10 * np.max(np.abs(jS))
    if is_chain:
        T = len(model.x_ids)
        tr = {int(f): r for r, f in enumerate(g["fid"])}
        rows = [tr[int(f)] for f in model.factor_ids[T:]]                    # transitions in time order: (out, in) = (x_{t+1}, x_t)
        assert _rel(covs[rows][:, :d, d:], Pc) <= 1e-10 and _rel(covs[rows][:, d:, d:], Ps[:-1]) <= 1e-10
        assert _rel(means[rows][:, :d], ms[1:]) <= 1e-10
    # predictive: the formula from exact messages against the dense leave-one-out solve; causal totals are log Z on a chain
    loo = P.predictive_from_messages(gm, f2v, mode=P.LOO)
    P.assert_rows_close(loo, P.dense_loo_all(gm), 1e-10, name + " loo")
    if is_chain:
        cau = P.predictive_from_messages(gm, f2v, mode=P.CAUSAL)
        # the first row (flat prior on x_1 through an invertible H) is improper; the rest are the Kalman innovations: their sum and
        # -log|det H| make log p(y)
        assert cau["counts"]["improper"] == 1
        assert abs(cau["total"] - np.log(abs(np.linalg.det(H))) - jlz) <= 1e-10 * abs(jlz)
    # sampling: the forest sampler's factor B of the joint covariance
    smean, B, Sig = SS.tree_sampler(gm)
    assert _rel(B @ B.T, jS) <= 1e-10 and _rel(smean, jm) <= 1e-10
    # functionals: the adjoint recursion from the messages, and the dense moments, against W S W'
    fs, _names = F.standard_functionals(gm, seed=5)
    W = F.weight_matrix(gm, fs)
    free = np.flatnonzero(~gm.obs)
    Wf = W[:, free, :].reshape(len(W), -1)
    want_m, want_c = np.einsum("kvi,vi->k", W, jm), Wf @ jS @ Wf.T
    for got in (F.dense_moments(gm, fs), F.adjoint_moments(gm, f2v, fs)):
        em, ec = F.rel_errors(got[0], got[1], want_m, want_c)
        assert em <= F.REL_TOL / 10 and ec <= F.REL_TOL / 10, (name, em, ec)


# ---- (c) the gap ----------------------------------------------------------------------------------------------------------------------------
class TransposedForward(MvFlood):
    """a deliberately WRONG restatement: the forward covariance as A' S A + Q (the mean and everything else as oracle/mv.py)"""

    def _rule(self, e):
        r = super()._rule(e)
        p = int(self.g.partner[e])
        if r is None or self.role[e] != 0:
            return r
        A, Q = self.psets[int(self.pset[e])]
        S = np.zeros_like(Q) if p in self.point else self.v2f[p][1]
        return r[0], A.T @ S @ A + Q


def _marginal_covariances(o, model, sweeps):
    o.sweep(sweeps)
    return np.stack([o.marginal(int(v))[1] for v in np.searchsorted(o.g.var_ids, model.x_ids)])


def test_the_default_chain_cannot_tell_a_transposed_rule_and_the_general_one_can():
    T, d = 12, 3
    iso, gen = cx.synth.lgssm_chain(T, d=d, seed=3), AN.chain(T, d)
    right, wrong = _marginal_covariances(MvFlood(iso), iso, T + 2), _marginal_covariances(TransposedForward(iso), iso, T + 2)
    assert _rel(wrong, right) <= 1e-12, "isotropic model: A' S A == A S A'"
    assert AN.offdiag_ratio(right) <= 1e-12, "every posterior covariance of the default chain is c_t I"
    right, wrong = _marginal_covariances(MvFlood(gen), gen, T + 2), _marginal_covariances(TransposedForward(gen), gen, T + 2)
    assert _rel(wrong, right) > 1e-3, "general model: the transposed rule is visibly wrong"
    assert _rel(right, AN.chain_posterior(gen)[1]) <= 1e-10


# ---- (d) the loopy reference converges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 4])
def test_the_loopy_reference_converges_within_the_gpu_tests_sweep_count(d):
    """loopy Gaussian BP need not converge for every draw: seed, skip and the skip links' scale are chosen so that it does — the C checker
    alone reaches a residual below 1e-12 in AN.LOOPY_SWEEPS sweeps, and its means are then the joint solve's (exact at a fixed point)"""
    model = AN.loopy(AN.LOOPY_T, d, skips=AN.LOOPY_SKIPS)
    o = MvFloodC(model)
    o.seed(0.0, AN.LOOPY_SEED_VARIANCE)
    o.sweep(AN.LOOPY_SWEEPS - 1, use_omp=True)
    before = (o.f2v_m.copy(), o.f2v_S.copy())
    o.sweep(1)
    pe = AN.latent_edges(o.g, model)
    res = max(np.max(np.abs(o.f2v_m[pe] - before[0][pe])), np.max(np.abs(o.f2v_S[pe] - before[1][pe])))
    assert res < 1e-12, res
    m, _S, ok = o.marginals()
    xs = np.searchsorted(o.g.var_ids, model.x_ids)
    em, ecov = AN.dense_posterior(model)
    assert ok[xs].all() and _rel(m[xs], em) <= 1e-10
    assert AN.offdiag_ratio(ecov) >= 0.1


# ---- the rank-deficient observation --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 4])
def test_the_constant_velocity_posterior_is_proper(d):
    """H has zero rows for the velocities: a likelihood message alone is improper, the joint posterior is not — joint_solve's Cholesky
    passes and the block-tridiagonal smoother with H agrees with it"""
    model = AN.velocity_chain(12, d)
    H = model.meta["H"]
    assert np.linalg.matrix_rank(H) == d // 2
    em, ecov = AN.dense_posterior(model)
    cm, ccov = AN.chain_posterior(model)
    assert _rel(cm, em) <= 1e-10 and _rel(ccov, ecov) <= 1e-10
    assert np.all(np.linalg.eigvalsh(ecov) > 0)
