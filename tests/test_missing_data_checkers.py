"""CPU: the references and the host logic on chains with UNOBSERVED states and with a forecast tail (tests/missing_data.py).

Every other model of the suite gives every latent variable a side message of its own.  Here: (a) on every model of the GPU table the
dense references (evidence_support.gmodel and what is built on it) agree with a covariance-form Kalman filter and smoother that skips
the update at a missing step and shares nothing with them; (b) a tail changes neither the evidence nor the first T marginals, and its
own marginals are the forecast recursion; (c) the host logic (cx_flatten.h, cx_chains.h, the tree plans) takes these graphs: a
thinned chain is one path of T positions, a tailed one of T + h - 1 — the degree-1 end is off the chain; (d) the lazy numpy BP on a tail
whose end message is unset: the forward messages are defined, no marginal is; (e) the gap — two plausible wrong passes agree with the
right one on a fully observed chain and fail on every thinned model; (f) the table is not vacuous: every model has a state without a side
message, every `run` model a whole scan unit without data."""
import functools

import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from tests import anisotropic as AN
from tests import evidence_support as E
from tests import functional_support as F
from tests import learning_support as LS
from tests import missing_data as MD
from tests import predictive_support as P
from tests.hostlogic import FlatGraph

TOL = 1e-10          # dense versus Kalman, as tests/test_evidence_checker.py and tests/test_predictive_checker.py
MODELS = MD.gpu_models()
CHAINS = [c[0] for c in MD.gpu_cases()]
COMBS = [n for n in MODELS if "comb" in n]
THINNED = [n for n, f, T, d, p, h in MD.gpu_cases() if p]


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(float(np.max(np.abs(b))), 1e-300))


@functools.lru_cache(maxsize=4)
def _dense(name):
    model = MODELS[name]()
    gm = E.gmodel(model)
    mean, S, fpos = LS.dense_posterior(gm)
    d = model.dim
    xi = np.searchsorted(gm.var_ids, model.x_ids)
    cov = np.stack([S[a * d:(a + 1) * d, a * d:(a + 1) * d] for a in fpos[xi]])
    return model, gm, mean[xi], cov, (mean, S, fpos)


def _cancellation(model):
    """what dense_log_z loses to rounding: it adds -1/2 sum y' R^-1 y and +1/2 h' J^-1 h, each of that size, and keeps their difference.
    ssm_chain's data grow like 2 t: at T = 3300 the two are 2.4e10 and log Z is -7e3, so the sum is good to eps * 2.4e10 = 5e-6 at best
    (measured against the filter, whose terms are all small: 1.2e-5 there, 5e-5 with every second datum).  64 ulp of that size are
    allowed on top of the 1e-10; on every other model of the table they come to 5e-10 at most.  The GPU file reads evidences at T = 40 only."""
    s = MD.chain_spec(model)
    y, keep = s["y"][s["keep"]], s["keep"]
    size = 0.5 * float(np.einsum("ni,nij,nj->", y, np.linalg.inv(s["R"][keep]), y))
    return 64 * np.finfo(float).eps * size


# ---- (a) the references agree ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CHAINS)
def test_dense_references_equal_the_kalman_smoother_that_skips_missing_steps(name):
    model, gm, mean, cov, dense = _dense(name)
    k = MD.kalman_missing(model)
    assert _rel(mean, k["mean"]) <= TOL and _rel(cov, k["cov"]) <= TOL
    log_z = E.dense_log_z(gm)
    assert abs(log_z - k["log_evidence"]) <= TOL * abs(log_z) + _cancellation(model), (log_z, k["log_evidence"])
    if not MD.is_reader_size(model):
        return
    d = model.dim
    # factor beliefs: the smoothed moments and the lag-one covariances, transitions inside a gap and inside a tail too
    means, covs = LS.dense_factor_beliefs(gm)
    where = {int(f): r for r, f in enumerate(gm.groups[2]["fid"])}
    tr, _ = MD._transitions(model)
    rows = [where[int(f)] for f in tr]
    later_first = not MD.chain_spec(model)["reverse"]           # entry 0 is the out end: x_{t+1}, but x_t on ssm_chain (additive: the lower id)
    a, b = (slice(0, d), slice(d, 2 * d)) if later_first else (slice(d, 2 * d), slice(0, d))
    assert _rel(means[rows][:, a], k["mean"][1:]) <= TOL and _rel(means[rows][:, b], k["mean"][:-1]) <= TOL
    assert _rel(covs[rows][:, a, a], k["cov"][1:]) <= TOL and _rel(covs[rows][:, b, b], k["cov"][:-1]) <= TOL
    assert _rel(covs[rows][:, a, b], k["lag_one"]) <= TOL
    # predictive rows: causal from exact messages = the innovations of the observed steps; leave-one-out from messages = the dense one
    f2v = F.forest_bp(gm)
    cau = P.predictive_from_messages(gm, f2v, mode=P.CAUSAL)
    want = {"factor_ids": k["factor_ids"], "mean": k["yhat"], "cov": k["S"], "log_density": k["log_density"], "mahalanobis": k["mahalanobis"]}
    # (the formula inverts the precision of a forward message; behind a gap of 26 steps it is 1.02e-10 from the filter, elsewhere
    # below 1e-10: held to the 1e-9 the GPU file asks of the device)
    P.assert_rows_close(cau, want, 1e-9, name + " causal")
    assert cau["counts"]["improper"] == 1 and cau["counts"]["rows"] == len(model.data_fac) < len(model.x_ids)
    assert abs(cau["total"] + k["log_first"] - log_z) <= TOL * abs(log_z)
    # leave-one-out: the dense solve against the formula, row by row.  A row is good to 1e-10 unless leaving its datum out leaves a state
    # known only across a gap, through A^-k: with the general A (singular values down to 0.4) of tests/anisotropic.py that problem is
    # nearly improper, and the two f64 computations differ by up to 4e-6 (d = 4, sparse).  Such rows exist only next to a gap on a
    # general model; the GPU file holds them to 10 times this measured difference and every other row to 1e-9.
    err = MD.loo_reference_error(gm, P.dense_loo_all(gm))
    s = MD.chain_spec(model)
    next_to_gap = np.array([t == 0 or t == s["T"] - 1 or not s["keep"][t - 1] or not s["keep"][t + 1] for t in k["steps"]])
    assert np.all(err[~next_to_gap] <= TOL) and np.all(err <= 1e-5), (name, err)
    if model.meta.get("general") is None:
        assert np.all(err <= TOL), (name, err)


@pytest.mark.parametrize("name", COMBS)
def test_dense_references_on_thinned_combs(name):
    """no chain: the joint solve of tests/anisotropic.py, assembled straight from roles, parameter sets and data, stands in for the filter"""
    model, gm, mean, cov, _ = _dense(name)
    jm, jc = AN.dense_posterior(model)
    assert _rel(mean, jm) <= TOL and _rel(cov, jc) <= TOL
    log_z = E.dense_log_z(gm)
    assert abs(log_z - AN.joint_solve(model)[3]) <= TOL * abs(log_z)
    leaves, _ = MD.flat_end_edges(model)
    assert len(leaves) >= 5, "unobserved teeth are latent leaves of degree 1"


@pytest.mark.parametrize("name", ["ssm T=40 d=1 sparse", "lin T=40 d=1 run(5,30)", "iso T=40 d=4 alt", "gen T=40 d=3 run(5,30)", "gen T=40 d=16 sparse"])
def test_the_f64_references_are_good_to_1e_12(name):
    """the Kalman reference in long double arithmetic is not available for missing steps; the two f64 references, which share no code and
    no algorithm (a joint solve, a filter), differ by less than 1e-12 on these well-conditioned problems (joint condition number <= 1e3)"""
    model, gm, mean, cov, _ = _dense(name)
    k = MD.kalman_missing(model)
    assert _rel(mean, k["mean"]) <= 1e-12 and _rel(cov, k["cov"]) <= 1e-12


# ---- (b) tail invariance in the references --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,d,pat,h", [("ssm", 1, None, 5), ("lin", 1, "alt", 5), ("lin", 1, None, 1), ("iso", 3, None, 5), ("gen", 4, "alt", 5), ("gen", 16, None, 1)])
def test_a_tail_changes_nothing_before_it(family, d, pat, h):
    T = 24 if d > 4 else 40
    plain, tailed = MD.make(family, T, d, pat), MD.make(family, T, d, pat, h)
    ga, gb = E.gmodel(plain), E.gmodel(tailed)
    za, zb = E.dense_log_z(ga), E.dense_log_z(gb)
    assert abs(za - zb) <= 1e-10 * abs(za)
    (ma, Sa, pa), (mb, Sb, pb) = LS.dense_posterior(ga), LS.dense_posterior(gb)
    xa, xb = np.searchsorted(ga.var_ids, plain.x_ids), np.searchsorted(gb.var_ids, tailed.x_ids)
    blocks = lambda S, pos: np.stack([S[a * d:(a + 1) * d, a * d:(a + 1) * d] for a in pos])
    assert _rel(mb[xb[:T]], ma[xa]) <= 1e-12 and _rel(blocks(Sb, pb[xb[:T]]), blocks(Sa, pa[xa])) <= 1e-12
    fm, fP = MD.kalman_missing(tailed)["forecast"]
    assert _rel(mb[xb[T:]], fm) <= TOL and _rel(blocks(Sb, pb[xb[T:]]), fP) <= TOL
    assert np.all(np.diff([np.trace(P_) for P_ in fP]) > 0) or family == "lin", "the forecast covariance grows along the tail"


# ---- (c) the host logic ---------------------------------------------------------------------------------------------------------------
def _flat(model, schedule):
    g = FlatGraph(model.edge_var, model.edge_fac, model.factor_ids, model.factor_kind, model.factor_var, edge_role=model.edge_role, dim=model.dim, schedule=schedule)
    assert g.status == L.OK, g.error
    g.clamp(model.data_var)
    return g


@pytest.mark.parametrize("family,d", [("ssm", 1), ("lin", 1), ("gen", 2), ("iso", 4), ("gen", 16)])
@pytest.mark.parametrize("pat,h", [("alt", 0), ("sparse", 0), ("run(5,30)", 0), (None, 1), (None, 5), ("alt", 5)])
def test_chain_decomposition_and_tree_plans(family, d, pat, h):
    T = 40
    model = MD.make(family, T, d, pat, h)
    g = _flat(model, L.SCHED_CHAIN_SCAN)
    rc, err = g.chains()
    assert rc == L.OK, err
    n_pos = T + h - 1 if h else T                           # the degree-1 end of a tail is off the chain
    pos = g.arr("var_ids")[g.arr("pos_var")]
    assert np.array_equal(pos, model.x_ids[:n_pos]) or np.array_equal(pos[::-1], model.x_ids[:n_pos])
    assert len(g.arr("from")) == n_pos - 1 and np.array_equal(g.arr("link_pos"), np.arange(n_pos - 1))
    hf, hb = g.arr("head_fwd"), g.arr("head_bwd")
    assert hf[0] == 1 and hf.sum() == 1 and hb[-1] == 1 and hb.sum() == 1
    if d > 1:
        assert g.scalar("npos_linked") == n_pos
    t = _flat(model, L.SCHED_TREE)
    for plan in (t.tree, t.tree_hp):
        rc, err = plan()
        assert rc == L.OK, err
    assert t.scalar("tree_components") == 1


@pytest.mark.parametrize("name", COMBS)
def test_tree_plans_take_a_thinned_comb(name):
    t = _flat(MODELS[name](), L.SCHED_TREE)
    for plan in (t.tree, t.tree_hp):
        rc, err = plan()
        assert rc == L.OK, err


# ---- (d) the lazy BP with the end message unset ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,d", [("ssm", 1), ("lin", 1), ("gen", 2)])
def test_lazy_bp_on_a_tail_whose_end_message_is_unset(family, d):
    """the reference of the GPU file's unset-end case: an undefined (NaN) message on the degree-1 end.  Every forward message — towards
    the tail — is defined at the fixed point, every backward message along the whole chain is not, and no marginal is"""
    T, h = 12, 3
    model = MD.make(family, T, d, None, h)
    v, f = MD.flat_end_edges(model)
    assert list(v) == [int(model.x_ids[-1])]
    gm = E.gmodel(model, opaque=(v, f, np.full((1, d), np.nan), np.full((1, d, d), np.nan)))
    e, l = E.numpy_bp(gm, max_iter=T + h + 4)[2]
    g = gm.groups[2]
    undefined = np.isnan(e).any(axis=2) | np.isnan(l).any(axis=(2, 3))
    ids = gm.var_ids[g["vars"]]
    tr = set(MD._transitions(model)[0].tolist())
    n_fwd = n_bwd = 0
    for fi, (fid, (va, vb), (ua, ub)) in enumerate(zip(g["fid"], ids, undefined)):
        if int(fid) not in tr:
            x = int(np.flatnonzero(~gm.obs[g["vars"][fi]])[0])
            assert not (ua, ub)[x], "a likelihood's message into its state"
            continue
        later = int(np.argmax([va, vb]))                     # ids grow along the chain and into the tail
        assert not (ua, ub)[later] and (ua, ub)[1 - later]
        n_fwd += 1; n_bwd += 1
    assert n_fwd == T + h - 1
    # with the flat message instead, everything is defined
    full = E.numpy_bp(E.gmodel(model), max_iter=T + h + 4)[2]
    assert not np.isnan(full[0][~gm.obs[g["vars"]]]).any()


# ---- (e) the gap ------------------------------------------------------------------------------------------------------------------------
def _causal_rows(model, carry_gap):
    s = MD.chain_spec(model)
    assert s["h"] == 0
    o = slice(None, None, -1) if s["reverse"] else slice(None)          # (ssm_chain: the device's causal order runs backwards; A = 1 there)
    keep = s["keep"][o]
    f = MD.kalman_filter(s["A"][o], s["b"][o], s["Q"][o], s["H"], s["R"][o], s["y"][o], keep, carry_gap=carry_gap)
    return f["yhat"][keep][1:], f["S"][keep][1:]


def test_two_wrong_passes_agree_with_the_right_one_on_a_fully_observed_chain():
    for family, d in (("lin", 1), ("gen", 3)):
        model = MD.make(family, 40, d)
        right, wrong = MD.chain_pass(model), MD.chain_pass(model, empty_side_is_undefined=True)
        assert _rel(wrong[0], right[0]) <= 1e-13 and _rel(wrong[1], right[1]) <= 1e-13
        em, ec = AN.dense_posterior(model) if d > 1 else _dense_scalar(model)
        assert _rel(right[0], em) <= TOL and _rel(right[1], ec) <= TOL
        a, b = _causal_rows(model, True), _causal_rows(model, False)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _dense_scalar(model):
    gm = E.gmodel(model)
    mean, S, fpos = LS.dense_posterior(gm)
    xi = np.searchsorted(gm.var_ids, model.x_ids)
    return mean[xi], np.diag(S)[fpos[xi]].reshape(-1, 1, 1)


@pytest.mark.parametrize("name", THINNED)
def test_the_wrong_passes_fail_on_every_thinned_model(name):
    """(1) a pass that takes a state WITHOUT a side message for one whose side message is not there yet leaves the chain undefined;
    (2) a causal prediction from the last filtered state with one transition drops the A P A' + Q accumulated over the gap: its
    predictive covariance after a gap is wrong."""
    family, T, d, pat, h = next(c[1:] for c in MD.gpu_cases() if c[0] == name)
    model = MD.make(family, T, d, pat)                       # (the passes take no tail)
    right, wrong = MD.chain_pass(model), MD.chain_pass(model, empty_side_is_undefined=True)
    k = MD.kalman_missing(model)
    assert _rel(right[0], k["mean"]) <= TOL and _rel(right[1], k["cov"]) <= TOL
    assert np.isnan(wrong[1]).any() or _rel(wrong[1], right[1]) > 1e-3
    a, b = _causal_rows(model, True), _causal_rows(model, False)
    assert _rel(b[1], a[1]) > 1e-3, "the predictive covariance after a gap"


# ---- (f) the table is not vacuous -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODELS))
def test_every_model_has_a_latent_state_without_a_side_message(name):
    model = MODELS[name]()
    ev = np.asarray(model.edge_var)
    deg = {int(v): int(c) for v, c in zip(*np.unique(ev, return_counts=True))}
    lik = set(np.asarray(model.data_fac).tolist())
    sided = set(ev[np.isin(model.edge_fac, list(lik))].tolist())
    bare = [int(x) for x in model.x_ids if int(x) not in sided]
    assert bare and all(deg[x] in ((1, 2, 3) if "comb" in name else (1, 2)) for x in bare)      # (a spine state: two neighbours and its tooth)
    assert not len(model.prior_var), "no unary prior stands in for the likelihood"
    if "tail" in model.meta:
        assert deg[int(model.x_ids[-1])] == 1
    elif "comb" not in name:
        assert MD.chain_spec(model)["keep"][[0, -1]].all()


def _bare_units(keep, unit):
    """aligned units of `unit` links (link l joins states l and l + 1) none of whose states has a datum"""
    n = len(keep)
    return [u for u in range((n - 1) // unit) if not keep[u * unit:(u + 1) * unit + 1].any()]


def test_every_run_leaves_a_whole_scan_unit_without_data():
    """the units: a 1024-link tile of cx_chain.hip; a 256 K tile of cx_mvchain.hip at K = 1 and, at K = 5 — whose tile of 1280 links
    is longer than the chain —, a thread's K links; a level-0 block of K0 links of cx_chain64_plan.h at the K the GPU test sets"""
    ks = MD.run(MD.SCALAR_T, *MD.SCALAR_RUN)
    assert _bare_units(ks, MD.SCALAR_TILE) == [1] and ks[MD.SCALAR_RUN[0] - 1] and MD.SCALAR_RUN[0] % MD.SCALAR_TILE and (MD.SCALAR_RUN[1] + 1) % MD.SCALAR_TILE
    km = MD.run(MD.MV_T, *MD.MV_RUN)
    assert MD.MV_K == (1, 5)
    assert _bare_units(km, MD.MV_LANES * 1) == [1]
    assert len(_bare_units(km, 5)) >= 100 and MD.MV_LANES * 5 > MD.MV_T
    kc = MD.run(MD.CORE_T, *MD.CORE_RUN)
    assert len(_bare_units(kc, MD.CORE_K)) >= 2 * MD.CORE_FAN, "whole groups of fan level-0 blocks"
    # a tail of 1500 scalar links crosses a tile boundary, and the tile it ends in holds nothing but transitions behind the last datum
    assert (MD.SCALAR_T - 1) // MD.SCALAR_TILE < (MD.SCALAR_T + 1500 - 2) // MD.SCALAR_TILE
    names = set(MODELS)
    for fam in ("ssm", "lin"):
        assert MD.case_name(fam, MD.SCALAR_T, 1, f"run({MD.SCALAR_RUN[0]},{MD.SCALAR_RUN[1]})", 0) in names
    for d in (2, 3, 4):
        assert MD.case_name("gen", MD.MV_T, d, f"run({MD.MV_RUN[0]},{MD.MV_RUN[1]})", 0) in names
    for d in MD.CORE_DIMS:
        assert MD.case_name("gen", MD.CORE_T, d, f"run({MD.CORE_RUN[0]},{MD.CORE_RUN[1]})", 0) in names


def test_thin_and_tail_keep_the_ids():
    base = cx.synth.lgssm_chain(9, d=2, seed=1)
    keep = MD.alt(9)
    m = MD.thin(base, keep)
    gone = base.data_fac[~keep]
    assert not np.isin(gone, m.edge_fac).any() and not np.isin(gone, m.factor_ids).any() and not np.isin(base.data_var[~keep], m.edge_var).any()
    assert len(m.edge_var) == len(base.edge_var) - 2 * len(gone) == len(m.edge_role) and len(m.factor_ids) == len(m.factor_kind) == len(m.factor_var)
    assert np.array_equal(m.x_ids, base.x_ids) and np.array_equal(m.data_var, base.data_var[keep]) and np.array_equal(m.data_y, base.data_y[keep])
    assert set(m.factor_ids.tolist()) < set(base.factor_ids.tolist())
    t = MD.tail(m, 3)
    assert np.array_equal(t.x_ids[:9], base.x_ids) and t.x_ids[9:].min() > max(base.edge_var.max(), base.edge_fac.max())
    assert len(set(t.factor_ids.tolist())) == len(t.factor_ids) and not set(t.factor_ids.tolist()) & set(t.edge_var.tolist())
    v, f = MD.flat_end_edges(t)
    assert list(v) == [int(t.x_ids[-1])] and list(f) == [int(t.factor_ids[-1])]
    for pat in (MD.alt(9), MD.sparse(9), MD.run(9, 2, 6), MD.random_keep(50, 0.3, 1)):
        assert pat[0] and pat[-1] and not pat.all()
    assert MD.sparse(9).sum() == 3
