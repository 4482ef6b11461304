"""CPU: the numpy restatement of cx_linear_moments' recursion (tests/functional_support.adjoint_moments, from the MESSAGES of numpy
belief propagation: functional_support.forest_bp, itself pinned against evidence_support.numpy_bp) against the dense answer W μ, W Σ Wᵀ on the models of the GPU tests, and the restatement's own error against that
solve — which sets the tolerance of tests/test_gpu_linear_moments.py."""
import numpy as np
import pytest

from tests import evidence_support as E
from tests import functional_support as F
from tests import learning_support as LS

CASES = F.cases(long=True)
_errors = {}


def _measure(name):
    if name not in _errors:
        _model, gm, _load = CASES[name][0]()
        fs, _names = F.standard_functionals(gm)
        ref = F.dense_moments(gm, fs)
        got = F.adjoint_moments(gm, F.forest_bp(gm), fs)
        _errors[name] = F.rel_errors(*got, *ref)
    return _errors[name]


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_matches_the_dense_answer(name):
    em, ec = _measure(name)
    print(f"{name}: mean error {em:.3e}, covariance error {ec:.3e}")
    assert em <= F.REL_TOL / 10 and ec <= F.REL_TOL / 10, (name, em, ec)


def test_restatement_error_sets_the_tolerance():
    """REL_TOL is 10 x the largest error of the restatement over all the models (rounded up, within a factor 2)"""
    worst = max(max(_measure(name)) for name in CASES)
    print(f"largest restatement error {worst:.3e}; REL_TOL {F.REL_TOL:.1e}")
    assert 10 * worst <= F.REL_TOL <= 20 * max(worst, 1e-13)


@pytest.mark.parametrize("name", ["ssm_chain 130", "lgssm_comb 15 d=3", "tree_model 60", "kary tree d=2"])
def test_two_pass_messages_are_the_flooding_fixed_point(name):
    _model, gm, _load = CASES[name][0]()
    a, b = F.forest_bp(gm), E.numpy_bp(gm)
    for k, g in gm.groups.items():
        fr = ~gm.obs[g["vars"]]
        for x, y in zip(a[k], b[k]):
            assert not np.isnan(x[fr]).any() and np.allclose(x[fr], y[fr], rtol=1e-10, atol=1e-12), (name, k)


def test_library_exports_the_entry(hip_lib):
    from cortex.jl_amd import _lib as L
    assert L.ABI_VERSION == 9 and hip_lib.cx_version() == 9 and hasattr(hip_lib, "cx_linear_moments")


def test_dense_moments_of_a_two_state_chain():
    """the yardstick against a hand computation: x1 - x2 of a two-state chain"""
    import cortex.jl_amd as cx
    gm = E.gmodel(cx.synth.ssm_chain(2, seed=3))
    mean, Sig, fpos = LS.dense_posterior(gm)
    free = gm.var_ids[~gm.obs]
    m, c = F.dense_moments(gm, [([free[0], free[1]], [[1.0], [-1.0]])])
    a, b = fpos[np.searchsorted(gm.var_ids, free[:2])]
    assert np.isclose(c[0, 0], Sig[a, a] + Sig[b, b] - 2 * Sig[a, b], rtol=1e-14)
    assert np.isclose(m[0], mean[np.searchsorted(gm.var_ids, free[0]), 0] - mean[np.searchsorted(gm.var_ids, free[1]), 0], rtol=1e-14)
