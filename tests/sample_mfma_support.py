"""Shared by the cx_sample_posterior_mfma tests (tests/test_gpu_sample_posterior_mfma.py, pinned on the CPU by
tests/test_sample_mfma_checker.py): the forests of the GPU tests by name.  The references are those of the dim 1 - 4 sampler
(tests/sampling_support.py: tree_sampler, identity_noise, samples_to_b, normals; tests/learning_support.py: dense_posterior), which work
at any dim.  The device's whitening matrix B is another square root of the posterior covariance (another root, another elimination
order), so the tests compare B Bᵀ with Σ, never B with the reference's B.

  models()   name -> builder of (model, opaque or None, how to load it): "sweep" synth.load_into_device and one sweep, "flat" through
             missing_data.load (the flat message on the one edge of every latent leaf), "opaque" with evidence_mfma_support.set_opaque
  TILED      the chains long enough for two and three tile levels at CX_SAMPLE_MFMA_TILE = 4 (4, 16, 64 items)
"""
from __future__ import annotations

from tests import anisotropic as AN
from tests import causal_mfma_support as CM
from tests import evidence_mfma_support as S
from tests import predictive_mfma_support as PM

TOL = 1e-9          # against exact references: the project's tolerance for this arithmetic class (tests/test_gpu_posterior_samples.py)
SAME = 1e-12        # between tile sizes, and between the Philox path and its restatement
TWO_PARENT_DIMS = (16, 20, 64)
TILE = 4
TILED = ((70, 5, 3), (70, 16, 3), (70, 17, 3), (22, 40, 2), (20, 64, 2))      # (states, dim, tile levels at TILE items per tile)


def tile_levels(n, tile):
    """tile levels above the positions of a path of n items (cx_sample_core.h: until every path has at most `tile` items)"""
    levels = 0
    while n > tile:
        n = -(-n // tile)
        levels += 1
    return levels


def models():
    out = {}
    for d in PM.SCHEDULE_DIMS:
        out[f"chain d={d}"] = lambda d=d: (PM.chain(d), None, "sweep")
        out[f"comb d={d}"] = lambda d=d: (PM.comb(d), None, "sweep")
    for d in TWO_PARENT_DIMS:
        out[f"two parents d={d}"] = lambda d=d: (CM.two_parents(d), None, "sweep")
    out["branching d=16"] = lambda: (CM.branching(16), None, "sweep")
    for T, d, _levels in TILED:
        out[f"long chain T={T} d={d}"] = lambda T=T, d=d: (AN.chain(T, d), None, "sweep")
    for d in PM.GEN_DIMS:
        out[f"gen alt tail d={d}"] = lambda d=d: (PM.gen(d), None, "flat")
        out[f"leading gap d={d}"] = lambda d=d: (PM.leading_gap(d), None, "flat")
    for d in PM.PRIOR_DIMS:
        out[f"prior d={d}"] = lambda d=d: S.prior_chain(d) + ("opaque",)
    for d in PM.CLAMPED_DIMS:
        out[f"clamped middle d={d}"] = lambda d=d: (S.clamped_middle(d), None, "sweep")
    return out
