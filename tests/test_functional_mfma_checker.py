"""CPU: the references of tests/test_gpu_linear_moments_mfma.py on the models those tests run (tests/sample_mfma_support.models()).  The
yardstick is the dense posterior (functional_support.dense_moments); against it, at the fixed point of functional_support.forest_bp,
both the centred restatement of §4i (adjoint_moments) and the UNCENTRED recursion of §4r / §4s that the device implements
(functional_mfma_support.uncentred_moments) stay within 1e-12 by rel_errors: three orders inside the GPU tests' TOL = 1e-9, so the
formula is checked before any GPU run and the references' own error is no part of the GPU tolerance."""
import numpy as np
import pytest

from tests import evidence_support as E
from tests import functional_mfma_support as FM
from tests import functional_support as FS
from tests import learning_support as LS
from tests import sample_mfma_support as SM

MODELS = SM.models()
BOUND = 1e-12


@pytest.fixture(scope="module")
def cache():
    return {}


def _case(cache, name):
    """(gm, fixed-point messages, functionals, dense moments) of a model, made once for both tests"""
    if name not in cache:
        model, opaque, _how = MODELS[name]()
        gm = E.gmodel(model, opaque=opaque) if opaque is not None else E.gmodel(model)
        fs, _names = FS.standard_functionals(gm)
        cache[name] = (gm, FS.forest_bp(gm), fs, FS.dense_moments(gm, fs, dense=LS.dense_posterior(gm)))
    return cache[name]


@pytest.mark.parametrize("name", list(MODELS))
def test_centred_restatement_matches_dense(cache, name):
    gm, f2v, fs, (rm, rc) = _case(cache, name)
    mean, cov = FS.adjoint_moments(gm, f2v, fs)
    em, ec = FS.rel_errors(mean, cov, rm, rc)
    print(name, "K", len(fs), "centred", em, ec)
    assert em <= BOUND and ec <= BOUND, (name, em, ec)


@pytest.mark.parametrize("name", list(MODELS))
def test_uncentred_recursion_matches_dense(cache, name):
    gm, f2v, fs, (rm, rc) = _case(cache, name)
    mean, cov = FM.uncentred_moments(gm, f2v, fs)
    assert np.isfinite(mean).all() and np.isfinite(cov).all()
    em, ec = FS.rel_errors(mean, cov, rm, rc)
    print(name, "K", len(fs), "uncentred", em, ec)
    assert em <= BOUND and ec <= BOUND, (name, em, ec)
