"""-m gpu: one change to a handle that has already run, then the run again — every marginal against the exact posterior of the CHANGED model.

A handle caches what it derives from its inputs (chains, tree plan, rule masks, work lists, constant messages, side sums, request lists);
csrc/cx_derived.h says which of them a change voids.  A flag forgotten there shows here as the posterior of the OLD model, or of a mixture.
Each test builds a handle, runs it to its answer (asserted: the caches are then warm and right), applies ONE change, runs again and compares
with tests/anisotropic.py: joint_solve (a dense solve of the joint Gaussian, no second handle) on the changed model.

Graphs, the smallest on which each cache exists: a chain of T = 12 latent states, each with one observation factor and a unary prior factor on
its first state; a tree of 7 states (root, two children, four grandchildren) with observations on the leaves and a prior on the root; the chain
with one factor of three variables (a state and two observed variables) for the k-ary tables.  Matrices are tests/anisotropic.py's general
(A, Q, R, H).  Chain scan, tree and reference order run ONE sweep; the fused schedule runs twice as many sweeps as there are states, after
which every message on a tree is exact whatever it was seeded with.  Under the reference order a run is "every input set again, one cx_sweep"
(see run()).

Tolerances are those of the exact-schedule tests of each family against the same kind of oracle: dim 1 1e-9 (test_gpu_chain_scan.py,
test_gpu_tree.py, test_gpu_reference_schedule.py; scaled by the median), dim 2..4 and 64 1e-9 (test_gpu_mv_chain.py,
test_gpu_mv64_chain.py; scaled by the maximum), reference order at dim > 1 1e-8 (test_gpu_reference_mv.py).
"""
import dataclasses

import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from tests import anisotropic as AN
from tests.helpers import assert_close

pytestmark = pytest.mark.gpu

T = 12
CHAIN, TREE, REF, FUSED = L.SCHED_CHAIN_SCAN, L.SCHED_TREE, L.SCHED_REFERENCE, L.SCHED_FUSED
NAMES = {CHAIN: "chain-scan", TREE: "tree", REF: "reference", FUSED: "fused"}


@dataclasses.dataclass
class Spec:
    """a model as the test changes it: the device graph and the oracle's model are both derived from this"""
    d: int
    states: list                 # latent state ids
    pair: list                   # (factor id, OUT variable, IN variable, parameter set)
    psets: dict                  # set -> (A, Q)
    data: dict                   # observed variable -> datum [d]
    prior: tuple                 # (variable, unary factor id, mean [d], covariance [d, d])
    kary: dict = None            # {"fid", "out", "ins": [state, observed variable], "sets": [set, set], "qset"}: out = A_s0 x + A_s1 w + N(0, Q_qset)


def _sets(d):
    if d == 1:
        return {0: (np.array([[0.85]]), np.array([[0.4]])), 1: (np.array([[1.3]]), np.array([[0.7]])), 2: (np.array([[-0.6]]), np.array([[0.9]]))}
    A, Q, R, H = AN.general_sets(d, AN.seed_of(d))
    A2, Q2, _, _ = AN.general_sets(d, AN.seed_of(d) + 50)
    return {0: (A, Q), 1: (H, R), 2: (0.8 * A2, Q2)}


def _finish(d, states, trans, obs_of, prior_var, kary_at=None):
    """ids: states as given, one observed variable and one likelihood factor per entry of obs_of, then the transitions, the prior, the k-ary part"""
    rng = np.random.default_rng([d, len(states), 5])
    nxt = max(states) + 1
    pair, data = [], {}
    for x in obs_of:
        y, f = nxt, nxt + 1
        nxt += 2
        pair.append((f, y, x, 1))
        data[y] = 1.5 * rng.standard_normal(d)
    for child, parent in trans:
        pair.append((nxt, child, parent, 0))
        nxt += 1
    B = rng.standard_normal((d, d))
    prior = (prior_var, nxt, rng.standard_normal(d), B @ B.T / d + 0.8 * np.eye(d))
    nxt += 1
    kary = None
    if kary_at is not None:
        u, w, f = nxt, nxt + 1, nxt + 2
        data[u], data[w] = rng.standard_normal(d), rng.standard_normal(d)
        kary = {"fid": f, "out": u, "ins": [kary_at, w], "sets": [0, 2], "qset": 0}
    return Spec(d, list(states), pair, _sets(d), data, prior, kary)


def chain_spec(d, kary=False):
    x = list(range(1, T + 1))
    return _finish(d, x, [(x[t + 1], x[t]) for t in range(T - 1)], x, x[0], kary_at=x[2] if kary else None)


def tree_spec(d):
    return _finish(d, list(range(1, 8)), [(2, 1), (3, 1), (4, 2), (5, 2), (6, 3), (7, 3)], [4, 5, 6, 7], 1)


def edges_of(spec, var):
    return [f for f, o, i, _ in spec.pair if var in (o, i)] + ([spec.prior[1]] if spec.prior[0] == var else []) + \
           ([spec.kary["fid"]] if spec.kary and var in [spec.kary["out"]] + spec.kary["ins"] else [])


def _moment(m, V):
    return np.concatenate([m, np.asarray(V).ravel()])[None, :]


def load(spec, schedule):
    d = spec.d
    dev = cx.DeviceGraph(dim=d, schedule=schedule)
    rows = []                                             # (factor id, kind, params, [(variable, role)])
    for f, o, i, s in spec.pair:
        A, Q = spec.psets[s]
        rows.append((f, L.FACTOR_GAUSS_LINEAR, [Q[0, 0], A[0, 0], 0.0] if d == 1 else [s, 0, 0], [(o, L.ROLE_OUT), (i, L.ROLE_IN)]))
    rows.append((spec.prior[1], L.FACTOR_OPAQUE, [0, 0, 0], [(spec.prior[0], L.ROLE_OUT)]))
    k = spec.kary
    if k:
        q = spec.psets[k["qset"]][1]
        rows.append((k["fid"], L.FACTOR_GAUSS_LINEAR_N, [q[0, 0], 0.0, 0.0] if d == 1 else [k["qset"], 0, 0],
                     [(k["out"], L.ROLE_OUT)] + [(v, L.ROLE_IN) for v in k["ins"]]))
    rows.sort()
    if d > 1:
        for s, (A, Q) in spec.psets.items():
            dev.set_factor_matrices(s, A, Q)
    dev.graph_create([v for r in rows for v, _ in r[3]], [r[0] for r in rows for _ in r[3]], [r[0] for r in rows], [r[1] for r in rows],
                     np.array([r[2] for r in rows], dtype=float), edge_role=[role for r in rows for _, role in r[3]])
    if k:
        set_kary(dev, spec)
    set_data(dev, spec)
    if schedule == FUSED:
        dev.seed_messages(L.TO_VARIABLE, 0.0, 50.0)       # (any proper start: on a tree the sweeps below overwrite all of it)
    set_prior(dev, spec)
    return dev


def set_data(dev, spec):
    dv = [(v, f) for v in spec.data for f in edges_of(spec, v)]
    dev.set_messages([v for v, _ in dv], [f for _, f in dv], L.TO_FACTOR, L.FORM_POINT, np.stack([spec.data[v] for v, _ in dv]))


def set_prior(dev, spec):
    v, f, m, V = spec.prior
    dev.set_messages([v], [f], L.TO_VARIABLE, L.FORM_MOMENT, _moment(m, V))


def set_kary(dev, spec):
    k = spec.kary
    if spec.d == 1:
        dev.set_factor_coefficients(k["ins"], [k["fid"]] * 2, [spec.psets[s][0][0, 0] for s in k["sets"]])
    else:
        dev.set_factor_edge_sets(k["ins"], [k["fid"]] * 2, k["sets"])


def run(dev, spec):
    """the handle to its answer.  Under the reference order ONE cx_sweep is one update_marginals! of the reference: it recomputes what the
    caller's set_value! calls made pending and reads everything else as it stands, so a caller of that schedule sets its inputs again before
    every call (tools/bench_c1_plugin.py, test_gpu_reference_mv.py: test_new_rule_matrices_under_a_standing_reference_plan) — as here"""
    if dev.schedule == REF:
        set_data(dev, spec)
        set_prior(dev, spec)
    dev.sweep(2 * len(spec.states) + 2 if dev.schedule == FUSED else 1)


def oracle_model(spec):
    """the pairwise model joint_solve reads: the prior as a factor to an observed pseudo-variable (datum = its mean, Q = its covariance); the factor
    of three variables, whose other two variables are observed, as a factor between its state and a pseudo-variable with datum y_u - A_1 y_w"""
    d = spec.d
    pair, data, psets = [], dict(spec.data), {}
    nxt = 10_000

    def add(out, inn, A, Q):
        s = len(psets)
        psets[s] = (np.asarray(A), np.asarray(Q))
        pair.append((nxt + s, out, inn, s))

    for _, o, i, s in spec.pair:
        add(o, i, *spec.psets[s])
    v, _, m, V = spec.prior
    data[20_000] = m
    add(20_000, v, np.eye(d), V)
    k = spec.kary
    if k:
        x, w = k["ins"]
        data[20_001] = data.pop(k["out"]) - spec.psets[k["sets"][1]][0] @ data.pop(w)
        add(20_001, x, spec.psets[k["sets"][0]][0], spec.psets[k["qset"]][1])
    dvar = sorted(data)
    latent = [x for x in spec.states if x not in data]
    return cx.synth.Model(edge_var=np.array([v for _, o, i, _ in pair for v in (o, i)]), edge_fac=np.array([f for f, *_ in pair for _ in range(2)]),
                          factor_ids=np.array([f for f, *_ in pair]), factor_kind=np.full(len(pair), L.FACTOR_GAUSS_LINEAR, np.int32),
                          factor_var=np.array([s for *_, s in pair]), x_ids=np.array(latent), data_var=np.array(dvar), data_fac=np.zeros(len(dvar), np.int64),
                          data_y=np.stack([data[v] for v in dvar]), dim=d, edge_role=np.array([L.ROLE_OUT, L.ROLE_IN] * len(pair), np.int32), psets=psets)


def tolerance(d, schedule):
    if d == 1:
        return 1e-9, "median"
    return (1e-8 if schedule == REF else 1e-9), "max"


def check(dev, spec, what):
    d = spec.d
    m = oracle_model(spec)
    mean, cov = AN.dense_posterior(m)
    marg = dev.get_marginals(m.x_ids)
    tol, scale = tolerance(d, dev.schedule)
    what = f"d={d} {NAMES[dev.schedule]} {what}"
    worst = max(assert_close(marg[:, :d], mean, tol, f"{what}: marginal means", scale_by=scale),
                assert_close(marg[:, d:].reshape(len(m.x_ids), d, d), cov, tol, f"{what}: marginal covariances", scale_by=scale))
    print(f"{what}: worst relative error {worst:.2e} (bound {tol:.0e})")


def warm(spec, schedule):
    dev = load(spec, schedule)
    run(dev, spec)
    check(dev, spec, "before the change")
    return dev


# ---- the changes: each applies itself to the handle and returns the changed model ------------------------------------------------------
def new_datum(dev, spec):
    y = sorted(o for _, o, _, s in spec.pair if s == 1)[1]      # the observation of the second observed state
    val = spec.data[y] + np.linspace(0.7, -1.1, spec.d)
    dev.set_messages([y], edges_of(spec, y), L.TO_FACTOR, L.FORM_POINT, val[None, :])
    return dataclasses.replace(spec, data={**spec.data, y: val})


def observe_state(dev, spec):
    x = spec.states[len(spec.states) // 2]                # mid-chain: the chain splits in two; tree: a grandchild, its parent keeps one child
    fs = edges_of(spec, x)
    val = np.linspace(0.4, -0.9, spec.d)
    dev.set_messages([x] * len(fs), fs, L.TO_FACTOR, L.FORM_POINT, np.tile(val, (len(fs), 1)))
    return dataclasses.replace(spec, data={**spec.data, x: val})


def new_prior(dev, spec):
    v, f, m, V = spec.prior
    m2, V2 = m + 1.0, 0.3 * V + 0.1 * np.eye(spec.d)
    dev.set_messages([v], [f], L.TO_VARIABLE, L.FORM_MOMENT, _moment(m2, V2))
    return dataclasses.replace(spec, prior=(v, f, m2, V2))


def new_transition_matrices(dev, spec):
    A, Q = spec.psets[2]
    A2, Q2 = 1.1 * A, 0.5 * (Q + spec.psets[0][1])
    dev.set_factor_matrices(0, A2, Q2)
    return dataclasses.replace(spec, psets={**spec.psets, 0: (A2, Q2)})


def new_kary_parameters(dev, spec):
    """dim 1: a new coefficient (cx_set_factor_coefficients); dim 2: another parameter set for the state's edge (cx_set_factor_edge_sets)"""
    k = dict(spec.kary)
    if spec.d == 1:
        spec = dataclasses.replace(spec, psets={**spec.psets, 3: (np.array([[1.7]]), spec.psets[0][1])})
        k["sets"] = [3, k["sets"][1]]
        spec = dataclasses.replace(spec, kary=k)
        dev.set_factor_coefficients([k["ins"][0]], [k["fid"]], [1.7])
    else:
        k["sets"] = [2, k["sets"][1]]
        spec = dataclasses.replace(spec, kary=k)
        dev.set_factor_edge_sets([k["ins"][0]], [k["fid"]], [2])
    return spec


CHAINS = [(1, CHAIN), (1, REF), (1, FUSED), (2, CHAIN), (2, REF), (2, FUSED), (4, CHAIN), (4, FUSED), (64, CHAIN), (64, FUSED)]
TREES = [(1, TREE), (2, TREE)]
KEYED_ON_OBSERVED = [(1, CHAIN), (1, REF), (2, CHAIN), (2, REF), (64, CHAIN)]


def _spec(d, schedule, kary=False):
    return tree_spec(d) if schedule == TREE and not kary else chain_spec(d, kary)


def _ids(cases):
    return [f"d{d}-{NAMES[s]}" for d, s in cases]


@pytest.mark.parametrize("d,schedule", CHAINS + TREES, ids=_ids(CHAINS + TREES))
def test_new_datum_on_an_observed_variable(hip_lib, d, schedule):
    spec = _spec(d, schedule)
    dev = warm(spec, schedule)
    spec = new_datum(dev, spec)
    run(dev, spec)
    check(dev, spec, "after a new datum")


@pytest.mark.parametrize("d,schedule", KEYED_ON_OBSERVED + TREES, ids=_ids(KEYED_ON_OBSERVED + TREES))
def test_a_free_state_becomes_observed(hip_lib, d, schedule):
    """CX_FORM_POINT on every edge of a state that was free: it leaves the chains / the forest / the cached request of the reference order.

    dim 1 chain scan also reads two variables OFF the chains, whose marginals are the products of the STORED messages into them: the newly
    observed state (the messages into it are those of the run before — none of them depends on its own datum — so its marginal is its
    posterior in the model before the change) and an observed variable into which the test stored a message (that message).  The dim > 1
    kernels never form the marginal of an observed variable (cx_mv.hip: the variable phase skips them): those reads are dim 1's.
    Under the reference order the newly observed state must also leave the request of a plain cx_sweep (read back from the call's trace)."""
    spec = _spec(d, schedule)
    offchain = d == 1 and schedule == CHAIN
    dev = load(spec, schedule)
    if offchain:
        y = min(spec.data)
        dev.set_messages([y], edges_of(spec, y), L.TO_VARIABLE, L.FORM_MOMENT, np.array([[0.25, 1.75]]))
    run(dev, spec)
    check(dev, spec, "before the change")
    before = oracle_model(spec)
    changed = observe_state(dev, spec)
    run(dev, changed)
    check(dev, changed, "after a state became observed")
    if schedule == REF:
        # a plain cx_sweep of the reference order asks for every variable that is neither observed nor a stand-in (cx_api_ref.hip: ref_sweep_all)
        asked = sorted(v for kind, v, *_ in dev.ref_trace() if kind == L.ITEM_INDIVIDUAL_MARGINAL)
        assert asked == sorted(x for x in changed.states if x not in changed.data), "the marginals the call after the change computed"
    if offchain:
        x = spec.states[len(spec.states) // 2]
        mean, cov = AN.dense_posterior(before)
        i = int(np.flatnonzero(before.x_ids == x)[0])
        assert_close(dev.get_marginals([x]), np.array([[mean[i, 0], cov[i, 0, 0]]]), 1e-9, "the newly observed state: product of the stored messages into it")
        assert_close(dev.get_marginals([y]), np.array([[0.25, 1.75]]), 1e-12, "an observed variable off the chains: the stored message into it")


@pytest.mark.parametrize("d,schedule", CHAINS + TREES, ids=_ids(CHAINS + TREES))
def test_new_prior_on_an_end_variable(hip_lib, d, schedule):
    spec = _spec(d, schedule)
    dev = warm(spec, schedule)
    spec = new_prior(dev, spec)
    run(dev, spec)
    check(dev, spec, "after a new prior")


MATRICES = [c for c in CHAINS + TREES if c[0] > 1]


@pytest.mark.parametrize("d,schedule", MATRICES, ids=_ids(MATRICES))
def test_new_transition_matrices(hip_lib, d, schedule):
    spec = _spec(d, schedule)
    dev = warm(spec, schedule)
    spec = new_transition_matrices(dev, spec)
    run(dev, spec)
    check(dev, spec, "after new (A, Q) of the transition set")


KARY = [(1, FUSED), (1, TREE), (1, REF), (2, FUSED), (2, TREE), (2, REF)]


@pytest.mark.parametrize("d,schedule", KARY, ids=_ids(KARY))
def test_new_parameters_of_a_factor_of_three_variables(hip_lib, d, schedule):
    spec = _spec(d, schedule, kary=True)
    dev = warm(spec, schedule)
    spec = new_kary_parameters(dev, spec)
    run(dev, spec)
    check(dev, spec, "after new k-ary parameters")


IMPORTS = KEYED_ON_OBSERVED + TREES + [(1, FUSED), (2, FUSED), (64, FUSED)]


@pytest.mark.parametrize("d,schedule", IMPORTS, ids=_ids(IMPORTS))
def test_state_of_the_changed_model_imported_into_a_handle_that_ran_on_the_old_one(hip_lib, d, schedule):
    """the change: a state becomes observed where a cache is keyed on the observed set, a new datum elsewhere"""
    spec = _spec(d, schedule)
    donor, other = warm(spec, schedule), warm(spec, schedule)
    changed = (observe_state if schedule != FUSED else new_datum)(donor, spec)
    run(donor, changed)
    other.import_state(donor.export_state())
    check(other, changed, "right after the import")
    run(other, changed)
    check(other, changed, "a run after the import")
