"""CPU: the numpy statements of tests/sampling_support.py that the posterior-sampling GPU tests lean on — the restated Philox4x32-10
against known answers, its normals, and the forest sampler's whitening identity B Bᵀ = Σ on the dense posterior."""
import numpy as np
import pytest

import cortex.jl_amd as cx
from tests import evidence_support as E
from tests import sampling_support as SS

# (counter, key) -> the four output words; the first three are Random123's known answers, all four agree with rocRAND's
# philox4x32_10_engine::ten_rounds (rocrand/rocrand_philox4x32_10.h)
KATS = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
        ((0xFFFFFFFF,) * 4, (0xFFFFFFFF, 0xFFFFFFFF), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
        ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
        ((1, 2, 3, 4), (7, 0), (0x0F4D221A, 0xA2566CE1, 0xF498801B, 0xB076574D))]


def test_philox_known_answers():
    ctr = np.array([k[0] for k in KATS], np.uint64)
    key = np.array([k[1] for k in KATS], np.uint64)
    got = SS.philox4x32_10(ctr, key)
    assert got.tolist() == [list(k[2]) for k in KATS]


def test_normals_layout_and_moments():
    z = SS.normals(3, np.arange(4000), 25, 3)
    assert z.shape == (4000, 25, 3)
    # sample s, variable v of one call equals the same draw of a call over other samples / variables
    assert np.array_equal(SS.normals(3, [17, 2], 25, 3), z[[17, 2]])
    assert np.array_equal(SS.normals(3, [5], 10, 3)[0], z[5, :10])
    # d = 3 takes components 0, 1 of pair 0 and component 0 of pair 1: d = 4 extends it
    assert np.array_equal(SS.normals(3, [5], 25, 4)[0, :, :3], z[5])
    assert not np.array_equal(SS.normals(4, [5], 25, 3), z[[5]])
    x = z.ravel()
    n = len(x)
    assert abs(x.mean()) < 6 / np.sqrt(n) and abs(x.var() - 1) < 6 * np.sqrt(2 / n)


MODELS = [("ssm_chain", lambda: cx.synth.ssm_chain(30, seed=11)),
          ("ssm_chain_linear", lambda: cx.synth.ssm_chain_linear(30, seed=12)),
          ("lgssm_chain d=3", lambda: cx.synth.lgssm_chain(12, d=3, seed=13)),
          ("lgssm_comb d=2", lambda: cx.synth.lgssm_comb(6, d=2, teeth=1, seed=14)),
          ("kary_model", lambda: cx.synth.kary_model(8, seed=15, tree=True)),
          ("tree_model", lambda: cx.synth.tree_model(30, seed=16, observe=0.25, components=3))]


@pytest.mark.parametrize("name,make", MODELS, ids=[m[0] for m in MODELS])
def test_tree_sampler_whitens_the_dense_posterior(name, make):
    gm = E.gmodel(make())
    mean, B, Sig = SS.tree_sampler(gm)
    assert np.max(np.abs(B @ B.T - Sig)) <= 1e-10 * np.max(np.abs(Sig))
    # identity noise through the sampler's own affine map reproduces B column by column
    eps = SS.identity_noise(gm)
    free = np.flatnonzero(~gm.obs)
    z = eps[:, free, :].reshape(len(eps), -1) @ B.T
    x = np.repeat(mean[None], len(eps), axis=0)
    x[:, free, :] += z.reshape(len(eps), len(free), gm.d)
    assert np.allclose(SS.samples_to_b(x, mean, gm), B, atol=1e-12 * np.max(np.abs(B)))


def test_tree_sampler_refuses_a_cycle():
    gm = E.gmodel(cx.synth.gaussian_grid(3, 3, seed=1))
    with pytest.raises(ValueError):
        SS.tree_sampler(gm)
