"""CPU: the references of tests/test_gpu_sample_posterior_mfma.py on the models those tests run.  tree_sampler (the forest sampler from the
dense posterior) whitens the dense posterior on every model: B Bᵀ = Σ at rounding level (measured: at most 5e-15 relative, every Σ
conditioned under 5e2), so 1e-9 on the device leaves four orders and more above the references' own error.  normals (the device generator
restated) has the layout the header states at odd dims: the second normal of the last pair is dropped, nothing else moves."""
import numpy as np
import pytest

from tests import evidence_support as E
from tests import sample_mfma_support as SM
from tests import sampling_support as SS

MODELS = SM.models()


@pytest.mark.parametrize("name", list(MODELS))
def test_tree_sampler_whitens_the_dense_posterior(name):
    model, opaque, _how = MODELS[name]()
    gm = E.gmodel(model, opaque=opaque) if opaque is not None else E.gmodel(model)
    mean, B, Sig = SS.tree_sampler(gm)
    assert np.isfinite(mean).all() and mean.shape == (len(gm.var_ids), gm.d)
    err = np.max(np.abs(B @ B.T - Sig)) / np.max(np.abs(Sig))
    cond = np.linalg.cond(Sig)
    print(name, err, cond)
    assert err <= 1e-13 and cond <= 1e3, (name, err, cond)
    assert np.array_equal(mean[gm.obs], gm.y[gm.obs])


def test_the_tiled_chains_have_the_levels_the_gpu_test_says():
    assert [SM.tile_levels(T, SM.TILE) for T, _d, _l in SM.TILED] == [lv for _T, _d, lv in SM.TILED]
    assert all(SM.tile_levels(T, 64) <= 1 for T, _d, _l in SM.TILED)


@pytest.mark.parametrize("d", [5, 17])
def test_normals_at_an_odd_dim_drop_the_second_normal_of_the_last_pair(d):
    samples, nv = np.array([0, 3, 2 ** 32 + 1]), 4
    odd, even = SS.normals(7, samples, nv, d), SS.normals(7, samples, nv, d + 1)
    assert odd.shape == (3, nv, d) and np.array_equal(odd, even[:, :, :d])
    # component k of variable v in sample s comes from counter (k // 2, v, s): a pair is one call
    one = SS.normals(7, samples[1:2], nv, 2)
    assert np.array_equal(one[0], odd[1, :, :2])
    assert not np.array_equal(SS.normals(8, samples, nv, d), odd)
