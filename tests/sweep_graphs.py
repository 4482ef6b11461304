"""Graphs and read-backs shared by tests/test_gpu_sweep_last_marginals.py, test_gpu_partner_runs.py and test_partner_runs_host.py:
plain cx.synth.Model values, seeded."""
import numpy as np

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L


def with_star(model, hub, n_leaves=12, seed=5):
    """`model` plus `n_leaves` new variables, each with a unary prior and one pairwise factor to variable `hub`: the hub's degree
    grows by n_leaves (beyond 8 it moves to the CSR tail and the wave-per-variable kernels)"""
    rng = np.random.default_rng(seed)
    top = int(max(model.edge_var.max(), model.factor_ids.max()))
    leaf = top + 1 + np.arange(n_leaves, dtype=np.int64)
    prior = leaf + n_leaves
    pair = prior + n_leaves
    return cx.synth.Model(
        edge_var=np.concatenate([model.edge_var, leaf, leaf, np.full(n_leaves, hub, np.int64)]),
        edge_fac=np.concatenate([model.edge_fac, prior, pair, pair]),
        factor_ids=np.concatenate([model.factor_ids, prior, pair]),
        factor_kind=np.concatenate([model.factor_kind, np.full(n_leaves, L.FACTOR_OPAQUE, np.int32), np.full(n_leaves, L.FACTOR_GAUSS_ADDITIVE, np.int32)]),
        factor_var=np.concatenate([model.factor_var, np.ones(n_leaves), rng.uniform(0.5, 2.0, n_leaves)]),
        x_ids=np.concatenate([model.x_ids, leaf]),
        prior_var=np.concatenate([model.prior_var, leaf]), prior_fac=np.concatenate([model.prior_fac, prior]),
        prior_mean=np.concatenate([model.prior_mean, rng.standard_normal(n_leaves)]),
        prior_variance=np.concatenate([model.prior_variance, rng.uniform(0.5, 2.0, n_leaves)]))


def grid_with_star():
    """the 20 x 37 grid with a star of 12 pairwise factors on variable (10, 18): a big-degree lane in the middle of a slice"""
    return with_star(cx.synth.gaussian_grid(20, 37, seed=7), hub=1 + 10 * 37 + 18)


def random_sparse(n_var=600, n_pair=900, seed=42):
    """variables with a unary prior each and random pairwise factors: no two neighbouring lanes share a partner difference"""
    rng = np.random.default_rng(seed)
    pairs = set()
    while len(pairs) < n_pair:
        a, b = rng.integers(1, n_var + 1, 2)
        if a != b:
            pairs.add((int(min(a, b)), int(max(a, b))))
    pairs = np.array(sorted(pairs), dtype=np.int64)
    x = np.arange(1, n_var + 1, dtype=np.int64)
    prior = x + n_var
    pf = 2 * n_var + 1 + np.arange(n_pair, dtype=np.int64)
    return cx.synth.Model(edge_var=np.concatenate([x, pairs[:, 0], pairs[:, 1]]), edge_fac=np.concatenate([prior, pf, pf]),
                          factor_ids=np.concatenate([prior, pf]),
                          factor_kind=np.concatenate([np.full(n_var, L.FACTOR_OPAQUE, np.int32), np.full(n_pair, L.FACTOR_GAUSS_ADDITIVE, np.int32)]),
                          factor_var=np.concatenate([np.ones(n_var), rng.uniform(0.5, 2.0, n_pair)]), x_ids=x,
                          prior_var=x, prior_fac=prior, prior_mean=rng.standard_normal(n_var), prior_variance=rng.uniform(0.5, 2.0, n_var))


def far_pair(n_var=40_000, seed=3):
    """variables 1 and n_var joined by one pairwise factor, every variable with a unary prior: the two ends' slots lie more than
    32,767 apart, so the partners do not fit 16-bit differences and the packed sweep is not taken"""
    rng = np.random.default_rng(seed)
    x = np.arange(1, n_var + 1, dtype=np.int64)
    prior = x + n_var
    pf = np.array([2 * n_var + 1], dtype=np.int64)
    return cx.synth.Model(edge_var=np.concatenate([x, [1, n_var]]), edge_fac=np.concatenate([prior, pf, pf]), factor_ids=np.concatenate([prior, pf]),
                          factor_kind=np.concatenate([np.full(n_var, L.FACTOR_OPAQUE, np.int32), [L.FACTOR_GAUSS_ADDITIVE]]).astype(np.int32),
                          factor_var=np.concatenate([np.ones(n_var), [0.7]]), x_ids=x,
                          prior_var=x, prior_fac=prior, prior_mean=rng.standard_normal(n_var), prior_variance=rng.uniform(0.5, 2.0, n_var))


# name -> (builder, seed variance for the messages nobody set)
PARTNER_RUN_GRAPHS = {
    "grid20x37": (lambda: cx.synth.gaussian_grid(20, 37, seed=7), 1e6),          # 3 slices, row ends inside waves, neighbours in other slices
    "grid2x2": (lambda: cx.synth.gaussian_grid(2, 2, seed=7), 1e6),
    "grid1x300": (lambda: cx.synth.gaussian_grid(1, 300, seed=7), 1e6),          # nv no multiple of 256: idle tail lanes
    "grid5x256": (lambda: cx.synth.gaussian_grid(5, 256, seed=7), 1e6),          # rows = slices: no split, uniform up / down difference
    "ssm_chain700": (lambda: cx.synth.ssm_chain(700, seed=3, random_variances=True), None),      # observed variables; undefined messages stay NaN
    "grid20x37_star": (grid_with_star, 1e6),                                     # a big-degree lane inside a slice
    "random600": (random_sparse, 50.0),                                          # every wave falls back
    "far_pair": (far_pair, 50.0),                                                # no 16-bit differences: the unpacked kernel
}


def read_back(dev, model):
    """every factor→variable message (scalars: natural form, as stored) and every marginal, float64"""
    form = L.FORM_NATURAL if model.dim == 1 else L.FORM_MOMENT
    return (dev.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE, form), dev.get_marginals(model.x_ids))
