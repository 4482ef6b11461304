"""CPU: every input of tests/test_gpu_general_mfma.py is what that file takes it for (tests/general_mfma_support.py), so that a failure
there means the kernel.

  1. two references that share no code agree on every model: evidence_support.dense_log_z against anisotropic.joint_solve, and
     learning_support.dense_factor_beliefs against learn_mfma_support.beliefs (the restatement of the kernel's algebra) on exact messages;
  2. the models are general where it matters, and synth's are not: this is the gap the GPU file closes, written down;
  3. A' for A and H' for H move the references by a thousand times the GPU tolerances on the general models, and H' for H moves nothing at
     all on an isotropic one;
  4. on the ring the reference alone converges within the GPU test's sweeps, every belief is proper, and Bethe differs from exact;
  5. Shumway-Stoffer EM on the EM case runs with a non-decreasing trace."""
import dataclasses
import math

import numpy as np
import pytest

from cortex.jl_amd import synth
from tests import anisotropic as AN
from tests import evidence_support as E
from tests import general_mfma_support as G
from tests import learn_mfma_support as LM
from tests import learning_support as LS

MODELS = G.gpu_models()


def _joint_log_z(model, opaque):
    """anisotropic.joint_solve's log Z; with a proper opaque prior N^-1(eta, Lambda) on x_1: the model without it (x_1 | data ~ N(m, S)),
    then  log ∫ N(x; m, S) N(x; Lambda^-1 eta, Lambda^-1) dx = log N(m; Lambda^-1 eta, S + Lambda^-1)"""
    if opaque is None:
        return AN.joint_solve(model)[3]
    ov, of, eta, lam = opaque
    assert len(ov) == 1
    d = model.dim
    keep_e, keep_f = ~np.isin(model.edge_fac, of), ~np.isin(model.factor_ids, of)
    base = dataclasses.replace(model, edge_var=model.edge_var[keep_e], edge_fac=model.edge_fac[keep_e], edge_role=model.edge_role[keep_e],
                               factor_ids=model.factor_ids[keep_f], factor_kind=model.factor_kind[keep_f], factor_var=model.factor_var[keep_f])
    mean, S, pos, log_z = AN.joint_solve(base)
    a = pos[int(ov[0])]
    m, S11 = mean[a * d:(a + 1) * d], S[a * d:(a + 1) * d, a * d:(a + 1) * d]
    P = np.linalg.inv(lam[0])
    r = m - P @ eta[0]
    V = S11 + P
    return float(log_z - 0.5 * r @ np.linalg.solve(V, r) - 0.5 * np.linalg.slogdet(2 * np.pi * V)[1])


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODELS))
def test_two_independent_references_agree(name):
    model, opq = MODELS[name]()
    gm = E.gmodel(model, opaque=opq)
    got, want = E.dense_log_z(gm), _joint_log_z(model, opq)
    print(f"{name}: dense_log_z {got!r} joint solve {want!r} relative {abs(got - want) / abs(want):.2e}")
    assert abs(want) >= 1 and abs(got - want) <= 1e-12 * abs(want), (name, got, want)
    if not G.is_forest(name):
        return      # (a loop: belief propagation is not exact there; test 4)
    want_m, want_c = LS.dense_factor_beliefs(gm)
    got_m, got_c, status = LM.beliefs(gm, E.numpy_bp(gm))
    assert np.all(status == LM.OK), (name, status)
    em = float(np.max(np.abs(got_m - want_m)) / np.max(np.abs(want_m)))
    ec = float(np.max(np.abs(got_c - want_c)) / np.max(np.abs(want_c)))
    print(f"{name}: restatement on exact messages against the dense beliefs: means {em:.2e} covariances {ec:.2e}")
    assert em <= 1e-11 and ec <= 1e-11, (name, em, ec)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
def _message_precisions(model):
    """every factor→variable message precision into a latent variable, from the reference's exact messages"""
    gm = E.gmodel(model)
    g = gm.groups[2]
    lam = E.numpy_bp(gm)[2][1]
    free = ~gm.obs[g["vars"]]
    out = lam[free]
    assert len(out) and np.all(np.isfinite(out))
    return out


@pytest.mark.parametrize("d", G.DIMS)
def test_the_models_are_general_and_synths_are_not(d):
    for m in (G.chain(d), G.comb(d)):
        ratio = AN.offdiag_ratio(AN.dense_posterior(m)[1])
        assert ratio >= 0.15, (d, m.meta["kind"], ratio)
        A, H = m.meta["A"], m.meta["H"]
        assert np.linalg.norm(A - A.T) >= 0.1 * np.linalg.norm(A) and np.linalg.norm(H - H.T) >= 0.1 * np.linalg.norm(H)
        for lam in _message_precisions(m):
            off = np.max(np.abs(lam * (1 - np.eye(d))))
            assert off >= 0.05 * np.max(np.diag(lam)), (d, m.meta["kind"], off, np.max(np.diag(lam)))
    A2, _, _, H2 = G.second_sets(d)
    assert np.linalg.norm(A2 - A2.T) >= 0.1 * np.linalg.norm(A2) and np.linalg.norm(H2 - H2.T) >= 0.1 * np.linalg.norm(H2)
    # the gap: on the isotropic chain of the existing tests every message precision is a multiple of the identity
    for lam in _message_precisions(synth.lgssm_chain(6, d=d, seed=30 + d)):
        assert np.max(np.abs(lam - lam[0, 0] * np.eye(d))) <= 1e-12 * abs(lam[0, 0]), d


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
def _moved(model, psets):
    """(relative change of log Z, largest change of a factor belief mean) under other parameter sets"""
    gm, gm2 = E.gmodel(model), E.gmodel(model, psets=psets)
    z, z2 = E.dense_log_z(gm), E.dense_log_z(gm2)
    return abs(z2 - z) / abs(z), float(np.max(np.abs(LS.dense_factor_beliefs(gm2)[0] - LS.dense_factor_beliefs(gm)[0])))


@pytest.mark.parametrize("name", [n for n in MODELS if G.is_recipe(n)])
def test_planted_transpositions_are_visible_on_the_general_models(name):
    model, _ = MODELS[name]()
    (A, Q), (H, R) = model.psets[0], model.psets[1]
    for what, psets in (("A' for A", {0: (A.T, Q), 1: (H, R)}), ("H' for H", {0: (A, Q), 1: (H.T, R)})):
        dz, dm = _moved(model, psets)
        print(f"{name}, {what}: log Z moves by {dz:.2e} relative, the belief means by {dm:.2e}")
        assert dz >= 1e-5 and dm >= 1e-3, (name, what, dz, dm)      # a thousand times the GPU tolerances


@pytest.mark.parametrize("d", G.DIMS)
def test_h_transposed_is_invisible_on_an_isotropic_model(d):
    model = synth.lgssm_chain(6, d=d, seed=30 + d)
    (A, Q), (H, R) = model.psets[0], model.psets[1]
    assert _moved(model, {0: (A, Q), 1: (np.asarray(H).T, R)}) == (0.0, 0.0)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [1e6, 1.0 / G.RING_SEED_VARIANCE], ids=["tight-seed", "device-seed"])
@pytest.mark.parametrize("d", G.RING_DIMS)
def test_ring_reference_converges_and_bethe_is_not_exact(d, prec):
    """from a tight seed N(0, 1e-6 I) and from the device's wide one N(0, 1e6 I): the fixed point does not depend on it"""
    gm = E.gmodel(G.ring(d))
    f150 = E.numpy_bp(gm, max_iter=G.RING_SWEEPS, seed_precision=prec)
    f300 = E.numpy_bp(gm, max_iter=2 * G.RING_SWEEPS, seed_precision=prec)
    b150, b300, exact = E.bethe_log_z(gm, f150), E.bethe_log_z(gm, f300), E.dense_log_z(gm)
    print(f"ring d {d}: Bethe after 150 {b150!r}, after 300 {b300!r}, exact {exact!r}, relative gap {abs(b150 - exact) / abs(exact):.2e}")
    assert math.isfinite(b150) and abs(b150 - b300) <= 1e-12 * abs(b300), (b150, b300)
    _, covs, status = LM.beliefs(gm, f150)
    assert np.all(status == LM.OK)
    free = np.repeat(~gm.obs[gm.groups[2]["vars"]], d, axis=1)
    for c, f in zip(covs, free):
        assert np.linalg.eigvalsh(c[np.ix_(f, f)])[0] > 0
    assert abs(b150 - exact) > 1e-5 * abs(exact), (b150, exact)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
def test_em_reference_runs_with_a_non_decreasing_trace():
    model, A0, Q0, C0, R0 = G.em_case()
    y = np.asarray(model.data_y).reshape(G.EM_T, G.EM_D)
    trace, params = LS.ss_em(y, A0, Q0, C0, R0, n_iter=G.EM_ITER)
    print("trace", trace)
    assert len(trace) == G.EM_ITER + 1 and np.all(np.isfinite(trace)) and np.all(np.diff(trace) >= 0), trace
    assert all(np.linalg.eigvalsh(p[1])[0] > 0 and np.linalg.eigvalsh(p[3])[0] > 0 for p in params)


# ---- the parts do not share data --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", G.DIMS_C)
def test_no_two_components_share_a_datum(d):
    ps, model = G.parts(d)
    assert [len(p.x_ids) for p in ps] == list(G.LENGTHS) and len(model.x_ids) == sum(G.LENGTHS)
    assert all(np.array_equal(p.psets[s][k], ps[0].psets[s][k]) for p in ps for s in (0, 1) for k in (0, 1))
    for m in [model] + ([G.forest(d)] if d in G.FOREST_DIMS else []):
        first = np.asarray(m.data_y).reshape(-1, d)[:, 0]
        assert len(np.unique(first)) == len(first), d
