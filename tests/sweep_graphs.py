"""Graphs and read-backs shared by tests/test_gpu_sweep_last_marginals.py, test_gpu_partner_runs.py, test_partner_runs_host.py,
test_gpu_sweep_pairs.py, test_gpu_grid_between_calls.py and test_lattice_plan.py: plain cx.synth.Model values, seeded."""
import dataclasses

import numpy as np
import pytest

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


class GridIds:
    """the ids of cx.synth.gaussian_grid(H, W) by grid position: variable (r, c), its unary factor, the pairwise factor towards each neighbour"""

    def __init__(self, H, W):
        self.H, self.W, self.V = H, W, H * W

    def var(self, r, c):
        return 1 + r * self.W + c

    def unary(self, r, c):
        return self.var(r, c) + self.V

    def factor(self, r, c, direction):
        """the factor between (r, c) and its neighbour to the "left", "right", "up" or "down" """
        H, W, V = self.H, self.W, self.V
        if direction in ("left", "right"):
            cc = c - 1 if direction == "left" else c
            assert 0 <= cc < W - 1
            return 2 * V + 1 + r * (W - 1) + cc
        rr = r - 1 if direction == "up" else r
        assert 0 <= rr < H - 1
        return 2 * V + H * (W - 1) + 1 + rr * W + c

    def pairwise_edges(self, r, c):
        """(variable ids, factor ids) of the pairwise edges of (r, c), in the order left, right, up, down with absent directions skipped"""
        have = [d for d, ok in (("left", c > 0), ("right", c < self.W - 1), ("up", r > 0), ("down", r < self.H - 1)) if ok]
        return (np.full(len(have), self.var(r, c), dtype=np.int64), np.array([self.factor(r, c, d) for d in have], dtype=np.int64))


# ---- a grid whose paired sweep meets an undefined variable→factor message in the middle of a call -------------------------------------
# factor_rule<kRuleAdditive> divides by 1 + q w.  The factor right of (1, 1) has q = 0.5 exactly; (1, 1) has the unary message (0, -2) in natural
# form and zeros from its four neighbours, so in sweep 1 its message into that factor is (0, -2), 1 + q w = 0 exactly and the factor sends
# (nan, -inf) to (1, 2).  In sweep 2 the messages out of (1, 2) have precision -inf and the rule turns them into nan; sweep 3 reads those.
UNDEFINED_MIDCALL_SHAPE = (4, 5)
UNDEFINED_MIDCALL_SENDER = (1, 1)


def undefined_midcall_grid():
    """(model, set_vars, set_facs, natural payload [n, 2]): the 4 x 5 grid with the variance of one factor set to 0.5, and the messages to
    store (CX_TO_VARIABLE, CX_FORM_NATURAL) after the usual load with a seed"""
    H, W = UNDEFINED_MIDCALL_SHAPE
    r, c = UNDEFINED_MIDCALL_SENDER
    ids = GridIds(H, W)
    m = cx.synth.gaussian_grid(H, W, seed=7)
    fv = m.factor_var.copy()
    fv[m.factor_ids == ids.factor(r, c, "right")] = 0.5
    model = dataclasses.replace(m, factor_var=fv)
    pv, pf = ids.pairwise_edges(r, c)
    set_vars = np.concatenate([[ids.var(r, c)], pv]).astype(np.int64)
    set_facs = np.concatenate([[ids.unary(r, c)], pf]).astype(np.int64)
    payload = np.zeros((len(set_vars), 2))
    payload[0] = (0.0, -2.0)
    return model, set_vars, set_facs, payload


def natural_form_sweeps(model, seed_variance, set_vars, set_facs, payload, n):
    """n plain Jacobi sweeps of a model of unary and two-variable additive factors in float64 numpy, natural form (xi, w), as the device
    defines them: a variable→factor message is the sum of the variable's OTHER messages in ascending factor id; the factor sends
    (xi, w) / (1 + q w); the result of an undefined (nan precision) variable→factor message is not stored.  Returns per sweep
    (messages with precision -inf, messages with nan precision, undefined variable→factor messages read), counted after / in the sweep."""
    order = np.lexsort((model.edge_fac, model.edge_var))
    ev, ef = model.edge_var[order], model.edge_fac[order]
    q = dict(zip(model.factor_ids.tolist(), np.asarray(model.factor_var, dtype=np.float64).tolist()))
    edge = {(int(v), int(f)): i for i, (v, f) in enumerate(zip(ev, ef))}
    by_fac, by_var = {}, {}
    for i, (v, f) in enumerate(zip(ev.tolist(), ef.tolist())):
        by_fac.setdefault(f, []).append(i)
        by_var.setdefault(v, []).append(i)
    msg = np.full((len(ev), 2), np.nan)
    for v, f, mean, var in zip(model.prior_var, model.prior_fac, model.prior_mean, model.prior_variance):
        msg[edge[(int(v), int(f))]] = (mean / var, 1.0 / var)
    pairwise = np.array([len(by_fac[f]) == 2 for f in ef.tolist()])
    msg[pairwise & np.isnan(msg[:, 1])] = (0.0, 1.0 / seed_variance)
    for v, f, p in zip(set_vars, set_facs, payload):
        msg[edge[(int(v), int(f))]] = p
    out = []
    with np.errstate(all="ignore"):
        for _ in range(n):
            new, undefined_read = msg.copy(), 0
            for f, es in by_fac.items():
                if len(es) != 2:
                    continue
                for src, dst in (es, es[::-1]):
                    acc = np.zeros(2)
                    for k in by_var[int(ev[src])]:
                        if k != src:
                            acc = acc + msg[k]
                    if np.isnan(acc[1]):
                        undefined_read += 1
                        continue
                    new[dst] = acc * (1.0 / (1.0 + q[f] * acc[1]))
            msg = new
            out.append((int(np.sum(msg[:, 1] == -np.inf)), int(np.sum(np.isnan(msg[:, 1]))), undefined_read))
    return out


# ---- what the grid-sweep tests (test_gpu_sweep_deep*.py, test_gpu_sweep_pairs.py, test_gpu_grid_between_calls.py) do to a handle ---------
_grids = {}


def model_of(shape, seed=7):
    """cx.synth.gaussian_grid(*shape, seed), made once"""
    if (shape, seed) not in _grids:
        _grids[(shape, seed)] = cx.synth.gaussian_grid(*shape, seed=seed)
    return _grids[(shape, seed)]


def fused_device(model, seed_variance=1e6):
    dev = cx.DeviceGraph(schedule=L.SCHED_FUSED)
    cx.synth.load_into_device(model, dev, seed_variance)
    return dev


def everything(dev, model):
    """factor→variable messages, marginals, and the variable→factor messages (formed on demand from the last sweep's input)"""
    f2v, marg = read_back(dev, model)
    return f2v, marg, dev.get_messages(model.edge_var, model.edge_fac, L.TO_FACTOR, L.FORM_NATURAL)


def assert_same(a, b, what):
    """two read_back or everything tuples, bit for bit"""
    for x, y, name in zip(a, b, ("messages to variables", "marginals", "messages to factors")):
        assert np.array_equal(x, y, equal_nan=True), f"{what}: {name} differ"


def paired_launches(dev):
    return dev.sweep_stats()["paired_launches"]


def launches(dev):
    """(launches of two sweeps, of three, of four)"""
    d = dev.sweep_deep_stats()
    return dev.sweep_stats()["paired_launches"], d["depth3_launches"], d["depth4_launches"]


def rows_cases(K):
    return (1, 3, 4 * (K - 1))


def load_undefined_midcall():
    model, sv, sf, payload = undefined_midcall_grid()
    dev = fused_device(model)
    dev.set_messages(sv, sf, L.TO_VARIABLE, L.FORM_NATURAL, payload)
    return model, dev


@pytest.fixture
def clean_env(monkeypatch):
    """(a fixture: a test file imports it by name)"""
    for name in ("CX_SWEEP_PAIRS", "CX_SWEEP_DEPTH", "CX_PAIR_ROWS", "CX_DEEP_ROWS", "CX_MARG_EVERY_SWEEP"):
        monkeypatch.delenv(name, raising=False)
    return monkeypatch
