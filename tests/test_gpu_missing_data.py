"""-m gpu: chains and combs with UNOBSERVED states and chains with a forecast tail (tests/missing_data.py), at every dim and under every
exact schedule, the fused sweep and the readers.

Everywhere else in the suite every latent variable has a side message of its own.  Here a state may have none — its side sum is exactly
zero, its link map a pure transition, a whole scan unit (a 1024-link tile of cx_chain.hip, a 256 K tile or a thread's K links of
cx_mvchain.hip, a level-0 block of cx_mv64chain.hip) may hold no data — and a tail ends in a latent variable of degree 1 whose
variable→factor message is the caller's flat (0, 0).  tests/test_missing_data_checkers.py pins the references on the same table of
models and shows that two plausible wrong passes agree with the right one on observed chains and fail on these.

Tolerances are those of each kernel family's own file (scale_by="max"): 1e-9 for the scalar chain scan, d <= 4 and d = 5 .. 64 at small
T; for the tree and reference-order schedules 1e-9 (scalar, d <= 4) and 1e-8 (matrix cores); the readers at their own files' 1e-9 and
functional_support.REL_TOL.  The f64 dense reference is good to <= 1e-12 on these models (the checker file measures it)."""
import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from cortex.jl_amd import learn
from tests import evidence_support as E
from tests import functional_support as F
from tests import learning_support as LS
from tests import missing_data as MD
from tests import predictive_support as P
from tests import sampling_support as SS
from tests.helpers import assert_close_by_max as assert_close
from tests.learning_support import assert_rel_close as _close

pytestmark = pytest.mark.gpu

CASES = {c[0]: c for c in MD.gpu_cases()}
MODELS = MD.gpu_models()


def names(pred):
    return [n for n, f, T, d, p, h in MD.gpu_cases() if pred(f, T, d, p, h)]


def tol_exact(d, schedule):
    if schedule == L.SCHED_CHAIN_SCAN or d <= 4:
        return 1e-9
    return 1e-8


_cache = {}


def ref(name):
    """per model of the table: the model, its GModel and the dense posterior of its states — computed once, left unchanged"""
    if name not in _cache:
        model = MODELS[name]()
        gm = E.gmodel(model)
        mean, S, fpos = LS.dense_posterior(gm)
        d = model.dim
        xi = np.searchsorted(gm.var_ids, model.x_ids)
        cov = np.stack([S[a * d:(a + 1) * d, a * d:(a + 1) * d] for a in fpos[xi]])
        _cache[name] = dict(model=model, gm=gm, mean=mean[xi], cov=cov, dense=(mean, S, fpos))
    return _cache[name]


def make_dev(model, schedule, flat_ends=True, **kw):
    dev = cx.DeviceGraph(dim=model.dim, schedule=schedule, **kw)
    return MD.load(model, dev, flat_ends=flat_ends)


def split(marg, d):
    """(means [n, d], covariances [n, d, d]) of get_marginals' rows"""
    n = len(marg)
    return marg[:, :d], marg[:, d:].reshape(n, d, d)


def check_marginals(dev, model, mean, cov, tol, what):
    d = model.dim
    marg = dev.get_marginals(model.x_ids)
    assert not np.any(np.isnan(marg)), f"{what}: undefined marginals"
    gm_, gc_ = split(marg, d)
    print(f"{what}: mean err {np.max(np.abs(gm_ - mean)) / np.max(np.abs(mean)):.2e} cov err {np.max(np.abs(gc_ - cov)) / np.max(np.abs(cov)):.2e}")
    assert_close(gm_, mean, tol, f"{what}: marginal means")
    assert_close(gc_, cov, tol, f"{what}: marginal covariances")
    return marg


def check_healthy(dev, what):
    """(dim > 1: a flat message that a rule sends — behind a tail's end, deep inside a gap — is rounding of either sign, measured at
    5e-17 .. 4e-15 of the rule's largest precision entry; cx_message_health counts a diagonal entry as negative below -1e-12 of it)"""
    h = dev.message_health()
    assert h["undefined"] == 0 and h["negative_precision"] == 0 and h["non_finite"] == 0 and h["defined"] > 0, (what, h)


def one_exact_sweep(name, schedule, what):
    """(a): one sweep, no seeding; every marginal; healthy messages; a second sweep leaves the marginals where they are"""
    r = ref(name)
    model = r["model"]
    dev = make_dev(model, schedule)
    dev.sweep(1)
    marg = check_marginals(dev, model, r["mean"], r["cov"], tol_exact(model.dim, schedule), what)
    check_healthy(dev, what)
    dev.sweep(1)
    assert_close(dev.get_marginals(model.x_ids), marg, 1e-12, f"{what}: second sweep")
    return dev


# ---- (a) exact schedules ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("onepass", ["default", "0"])
@pytest.mark.parametrize("name", names(lambda f, T, d, p, h: d == 1 and T == MD.SCALAR_T))
def test_scalar_chain_scan(hip_lib, monkeypatch, name, onepass):
    """run(600,2900): links 1024 .. 2047 are a whole tile of pure transitions (B = 0, D = a^2, rescaled to D = 1), and the gap starts and
    ends inside a tile; tail=1500 crosses a tile with nothing but transitions behind the last datum"""
    if onepass == "0":
        monkeypatch.setenv("CX_CHAIN_ONEPASS", "0")
    one_exact_sweep(name, L.SCHED_CHAIN_SCAN, f"{name} onepass {onepass}").close()


@pytest.mark.parametrize("K", MD.MV_K)
@pytest.mark.parametrize("name", names(lambda f, T, d, p, h: 2 <= d <= 4 and T == MD.MV_T))
def test_mv_chain_scan(hip_lib, monkeypatch, name, K):
    """P~ = P + U with U = 0: run(100,650) leaves the 256-link tile 256 .. 511 without data at K = 1 and whole threads at K = 5"""
    monkeypatch.setenv("CX_MVC_K", str(K))
    one_exact_sweep(name, L.SCHED_CHAIN_SCAN, f"{name} K={K}").close()


CORE_SCAN = [(n, "small") for n in names(lambda f, T, d, p, h: d >= 5 and h == 0)] + [(n, "default") for n in names(lambda f, T, d, p, h: d == 64 and h == 0)]


@pytest.mark.parametrize("name,plan", CORE_SCAN, ids=[f"{n}-{p}" for n, p in CORE_SCAN])
def test_matrix_core_chain_scan(hip_lib, monkeypatch, name, plan):
    """level-0 blocks of K0 = 3 links and groups of fan = 2 potentials composed of transitions only (native 16 and 32 tiles and 64)"""
    if plan == "small":
        monkeypatch.setenv("CX_MVC64_K", str(MD.CORE_K))
        monkeypatch.setenv("CX_MVC64_FAN", str(MD.CORE_FAN))
    dev = one_exact_sweep(name, L.SCHED_CHAIN_SCAN, f"{name} plan {plan}")
    if plan == "small":
        assert dev.chain_plan_stats()["levels"] >= 2
    dev.close()


TREE = names(lambda f, T, d, p, h: (d == 1 and T == MD.SCALAR_T and (h in (1, 1500) or (p or "").startswith("run")))
             or T == MD.READER_T and d <= 4
             or (T == MD.MV_T and f == "gen" and p != "sparse")
             or (d in (7, 16, 64) and p != "sparse" and h != 1)) + [n for n in MODELS if "comb" in n]


@pytest.mark.parametrize("heavy_paths", ["0", "1"])
@pytest.mark.parametrize("name", TREE)
def test_tree_schedule(hip_lib, monkeypatch, name, heavy_paths):
    """heavy paths through states with nothing hanging on them; a degree-1 latent leaf (a tail's end, an unobserved tooth of a comb)
    whose stored flat message goes through the rule"""
    monkeypatch.setenv("CX_TREE_HP", heavy_paths)
    one_exact_sweep(name, L.SCHED_TREE, f"{name} heavy paths {heavy_paths}").close()


REFERENCE = names(lambda f, T, d, p, h: T == MD.READER_T and (d <= 4 or (d in (16, 64) and (h == 5 or (p or "").startswith("run")))))


@pytest.mark.parametrize("name", REFERENCE)
def test_reference_order(hip_lib, name):
    one_exact_sweep(name, L.SCHED_REFERENCE, f"{name} reference order").close()


# ---- (b) fused sweeps ------------------------------------------------------------------------------------------------------------------
READER = names(lambda f, T, d, p, h: T == MD.READER_T and d <= 4)


def bp_counts(gm, f2v):
    """(defined, undefined) of the messages into non-observed variables"""
    free = ~gm.obs
    n_def = n_all = 0
    for k, g in gm.groups.items():
        e, l = f2v[k]
        into = free[g["vars"]]
        ok = ~(np.isnan(e).any(axis=2) | np.isnan(l).any(axis=(2, 3)))
        n_def += int((ok & into).sum())
        n_all += int(into.sum())
    return n_def, n_all - n_def


@pytest.mark.parametrize("name", READER)
def test_fused_sweeps(hip_lib, name):
    """no seeding: a message is defined once its inputs are.  After k < T sweeps as many messages are defined as after k rounds of the
    lazy numpy BP (the flat end message counts as defined from the start, an empty side sum is (0, 0), not undefined); after n + 8 sweeps
    the marginals are the dense ones"""
    r = ref(name)
    model, gm = r["model"], r["gm"]
    n, k = len(model.x_ids), 7
    dev = make_dev(model, L.SCHED_FUSED)
    dev.sweep(k)
    h = dev.message_health()
    want = bp_counts(gm, E.numpy_bp(gm, max_iter=k))
    assert want[1] > 0 and (h["defined"], h["undefined"]) == want and h["negative_precision"] == 0 and h["non_finite"] == 0, (name, h, want)
    dev.sweep(n + 8 - k)
    check_marginals(dev, model, r["mean"], r["cov"], 1e-9, f"{name} fused")
    check_healthy(dev, name)
    dev.close()


# ---- (c) readers ---------------------------------------------------------------------------------------------------------------------
def gaps(model):
    """maximal runs of states without a datum (a tail is the last one), as (first, last) indices into x_ids"""
    s = MD.chain_spec(model)
    out, start = [], None
    for t, k in enumerate(s["keep"].tolist() + [True]):
        if not k and start is None:
            start = t
        if k and start is not None:
            out.append((start, t - 1)); start = None
    return out


def functionals(model):
    """unit functionals at an observed state, inside the longest gap and at the last state; contrasts x_a - x_b with both ends inside one
    gap (where one is long enough), straddling a gap's edge, spanning the whole chain and from an observed state to the last state (of the
    tail, where there is one)"""
    d, x = model.dim, model.x_ids
    n = len(x)
    g = max(gaps(model), key=lambda ab: ab[1] - ab[0])
    eye = np.eye(d)
    w = np.linspace(0.5, 1.5, d)[None, :]
    fs = [([x[t]], eye[i:i + 1]) for t in (0, g[0], n - 1) for i in range(d)]
    pairs = [(g[0] - 1, g[0]), (0, n - 1), (n // 2, n - 1), (g[0] - 1, g[1] + 1 if g[1] + 1 < n else g[1])]
    if g[1] > g[0]:
        pairs.append((g[0], g[1]))
    return fs + [([x[a], x[b]], np.concatenate([w, -w])) for a, b in pairs]


def reader_ref(name):
    r = ref(name)
    if "log_z" not in r:
        model, gm = r["model"], r["gm"]
        d = model.dim
        k = MD.kalman_missing(model)
        nr = len(k["steps"])
        causal = {"factor_ids": k["factor_ids"], "mean": k["yhat"], "cov": k["S"], "log_density": k["log_density"], "mahalanobis": k["mahalanobis"]}
        if d > 1:
            fids, groups = LS.pset_groups(model)
        else:
            # dim 1 has per-factor parameters and a group shares its A: the likelihoods are one group; the additive transitions of
            # ssm_chain another, the linear ones of ssm_chain_linear (their own a and b each) a group each
            fids = np.asarray(model.factor_ids, np.int64)
            lik = np.isin(fids, np.asarray(model.data_fac))
            groups = np.where(lik, 0, 1 + (np.cumsum(~lik) - 1) * (model.meta["kind"] == "ssm_chain_linear")).astype(np.int64)
        n_groups = int(groups.max()) + 1
        fs = functionals(model)
        loo = P.dense_loo_all(gm)
        loo_err = MD.loo_reference_error(gm, loo)
        r.update(log_z=E.dense_log_z(gm), kalman=k, causal=causal, n_rows=nr, loo=loo, loo_err=loo_err, beliefs=LS.dense_factor_beliefs(gm),
                 fids=fids, groups=groups, n_groups=n_groups, stats=LS.grouped_statistics(gm, fids, groups, n_groups), functionals=fs, moments=F.dense_moments(gm, fs))
    return r


def rows_subset(res, sel):
    return {k: np.asarray(res[k])[sel] for k in ("factor_ids", "mean", "cov", "log_density", "mahalanobis")}


def check_loo_rows(got, want, ref_err, what):
    """test_gpu_predictive.py's 1e-9 on every row whose dense reference is itself good to 1e-10.  The others — with general matrices,
    leaving out a datum next to a long gap leaves a state known only through A^-k, a nearly improper problem: the dense solve and the
    message formula, both f64 on the CPU, differ by up to 4e-6 there (tests/test_missing_data_checkers.py measures it) — are held to
    10 times that difference, row by row"""
    assert np.array_equal(got["factor_ids"], want["factor_ids"]), what
    good = ref_err <= 1e-10
    P.assert_rows_close(rows_subset(got, good), rows_subset(want, good), 1e-9, what)
    for i in np.flatnonzero(~good):
        P.assert_rows_close(rows_subset(got, [i]), rows_subset(want, [i]), 10 * ref_err[i], f"{what} row {i} (reference error {ref_err[i]:.1e})")


READER_RUNS = [(n, s) for n in READER for s in ("chain-scan", "tree") if s == "tree" or CASES[n][3] == 1 or CASES[n][5] == 0]


@pytest.mark.parametrize("name,sched", READER_RUNS, ids=[f"{n}-{s}" for n, s in READER_RUNS])
def test_readers(hip_lib, name, sched):
    """variable terms of degree 2 with no opaque part, fewer predictive rows than states, a causal prediction that carries the Q
    accumulated over a gap, factor beliefs with a zero block on a tail, sampler and moment paths that start or end in a tail"""
    r = reader_ref(name)
    model, gm, k = r["model"], r["gm"], r["kalman"]
    d = model.dim
    dev = make_dev(model, L.SCHED_CHAIN_SCAN if sched == "chain-scan" else L.SCHED_TREE)
    dev.sweep(1)
    what = f"{name} {sched}"
    # evidence: the dense value and the Kalman filter's sum (test_gpu_evidence.py: 1e-9 relative)
    got, cnt = dev.log_evidence()
    assert cnt["undefined"] == 0 and cnt["not_positive_definite"] == 0, (what, cnt)
    assert abs(got - r["log_z"]) <= 1e-9 * abs(r["log_z"]), (what, got, r["log_z"])
    assert abs(got - k["log_evidence"]) <= 1e-9 * abs(k["log_evidence"]), (what, got, k["log_evidence"])
    # predictive: exactly the observed steps; causal = the innovations (test_gpu_predictive.py: 1e-9), the step after a gap included
    cau, loo = dev.predictive("causal"), dev.predictive("loo")
    assert np.array_equal(cau["factor_ids"], np.sort(model.data_fac)) and np.array_equal(loo["factor_ids"], cau["factor_ids"]), what
    P.assert_rows_close(cau, r["causal"], 1e-9, what + " causal")
    assert cau["counts"] == {"rows": r["n_rows"], "scored": r["n_rows"] - 1, "undefined": 0, "improper": 1}, (what, cau["counts"])
    assert abs(cau["total"] + k["log_first"] - r["log_z"]) <= 1e-9 * abs(r["log_z"]), (what, cau["total"], r["log_z"])
    check_loo_rows(loo, r["loo"], r["loo_err"], what + " loo")
    assert loo["counts"]["undefined"] == 0 and loo["counts"]["improper"] == r["loo"]["counts"]["improper"], (what, loo["counts"])
    # factor beliefs and statistics, transitions inside a gap and inside a tail too (test_gpu_factor_statistics.py: 1e-9)
    fids = gm.groups[2]["fid"]
    bm, bc = dev.factor_beliefs(fids)
    wm, wc = r["beliefs"]
    _close(bm, wm, 1e-9, what + " belief means")
    _close(bc, wc, 1e-9 * max(1.0, float(np.max(np.abs(wc)))), what + " belief covariances")
    st, scnt = dev.factor_statistics(n_groups=2) if d > 1 else dev.factor_statistics(r["fids"], r["groups"])
    for key in LS.KEYS:
        scale = max(1.0, float(np.max(np.abs(r["stats"][key])))) if key in ("S_xx", "sum_x") else 1.0
        _close(st[key], r["stats"][key], 1e-9 * scale, f"{what} {key}")
    assert scnt == {"factors": len(r["fids"]), "groups": r["n_groups"], "undefined": 0, "not_positive_definite": 0}, (what, scnt)
    # linear functionals (functional_support.REL_TOL)
    fm, fc, fcnt = dev.linear_moments(r["functionals"])
    em, ec = F.rel_errors(fm, fc, *r["moments"])
    assert fcnt["failed"] == 0 and em <= F.REL_TOL and ec <= F.REL_TOL, (what, em, ec, fcnt)
    # samples: the map from the normals is exact (test_gpu_posterior_samples.py: 1e-9)
    mean, Sig, _ = r["dense"]
    nv = len(gm.var_ids)
    x0, xcnt = dev.sample_posterior(1, noise=np.zeros((1, nv, d)))
    _close(x0[0], mean, 1e-9, what + " sample mean")
    assert xcnt["free"] == int((~gm.obs).sum()) and xcnt["undefined"] == 0 and xcnt["not_positive_definite"] == 0, (what, xcnt)
    eps = SS.identity_noise(gm)
    x, _ = dev.sample_posterior(len(eps), noise=eps)
    B = SS.samples_to_b(x, mean, gm)
    assert np.max(np.abs(B @ B.T - Sig)) <= 1e-9 * np.max(np.abs(Sig)), what + " B B'"
    dev.close()


def test_em_with_missing_observations(hip_lib):
    """learn.em on a chain observed at every second step: an exact E-step, so the trace does not decrease; the parameters are those of
    Shumway–Stoffer EM fed with the moments of the Kalman smoother that skips the missing steps (test_gpu_factor_statistics.py: 1e-7)"""
    d, T = 2, MD.MV_T
    model = MD.make("iso", T, d, "alt")
    rng = np.random.default_rng(d)
    A0 = model.meta["A"] + 0.05 * rng.standard_normal((d, d))
    Q0, C0, R0 = 2.0 * model.meta["Q"], np.eye(d) + 0.05 * rng.standard_normal((d, d)), 0.5 * model.meta["R"]
    want_trace, want = MD.ss_em_missing(model, A0, Q0, C0, R0, 5)
    dev = make_dev(model, L.SCHED_CHAIN_SCAN)
    trace, params = learn.em(dev, {0: (A0, Q0), 1: (C0, R0)}, n_iter=5)
    assert np.all(np.diff(trace) >= -1e-9 * abs(trace[-1])), np.diff(trace)
    _close(trace, want_trace, 1e-7, "trace")
    for got, w, what in ((params[0][0], want[0], "A"), (params[0][1], want[1], "Q"), (params[1][0], want[2], "C"), (params[1][1], want[3], "R")):
        assert np.max(np.abs(got - w)) <= 1e-7 * max(1.0, float(np.max(np.abs(w)))), (what, got, w)
    dev.close()


# ---- (d) tail invariance on the device ---------------------------------------------------------------------------------------------------
TAILS = [("ssm", 1, MD.READER_T, 1), ("ssm", 1, MD.READER_T, 5), ("lin", 1, MD.READER_T, 5), ("ssm", 1, MD.SCALAR_T, 1500), ("lin", 1, MD.SCALAR_T, 1500),
         ("gen", 2, MD.READER_T, 1), ("gen", 2, MD.READER_T, 5), ("iso", 4, MD.READER_T, 5), ("gen", 16, MD.CORE_T, 1), ("gen", 16, MD.CORE_T, 5),
         ("gen", 64, MD.CORE_T, 5)]


@pytest.mark.parametrize("family,d,T,h", TAILS)
def test_a_tail_leaves_the_rest_of_the_model_untouched(hip_lib, family, d, T, h):
    """a handle with the tail and one without, same data, same schedule (the scalar chain scan; the tree schedule for dim > 1, whose chain
    scan refuses a degree-1 end)"""
    schedule = L.SCHED_CHAIN_SCAN if d == 1 else L.SCHED_TREE
    name = MD.case_name(family, T, d, None, h)
    tailed = ref(name)["model"]
    plain = MD.make(family, T, d)
    a, b = make_dev(tailed, schedule), make_dev(plain, schedule)
    a.sweep(1); b.sweep(1)
    ma, mb = a.get_marginals(tailed.x_ids), b.get_marginals(plain.x_ids)
    assert not np.any(np.isnan(ma)) and not np.any(np.isnan(mb))
    tol = tol_exact(d, schedule)
    assert_close(ma[:T], mb, tol, f"{name}: the first T marginals")
    fm, fP = MD.kalman_missing(tailed)["forecast"]
    gm_, gc_ = split(ma[T:], d)
    assert_close(gm_, fm, tol, f"{name}: tail means vs the forecast recursion")
    assert_close(gc_, fP, tol, f"{name}: tail covariances vs the forecast recursion")
    # the backward messages along the tail are the flat message, natural-form zeros — not NaN, the marker of an undefined message
    xs, n = tailed.x_ids, len(tailed.x_ids)
    fs = tailed.factor_ids[-h:]
    back = a.get_messages(xs[T - 1:n - 1], fs, L.TO_VARIABLE, L.FORM_NATURAL)
    assert not np.any(np.isnan(back)), f"{name}: backward messages along the tail read as undefined"
    scale = float(np.max(np.abs(a.get_messages(xs[T:], fs, L.TO_VARIABLE, L.FORM_NATURAL))))
    assert np.max(np.abs(back)) <= 1e-9 * scale, (name, np.max(np.abs(back)), scale)
    if d <= 4:
        (za, ca), (zb, cb) = a.log_evidence(), b.log_evidence()
        assert ca["undefined"] == 0 and ca["not_positive_definite"] == 0, ca
        assert abs(za - zb) <= 1e-9 * abs(zb), (name, za, zb)
        for mode in ("causal", "loo"):
            pa, pb = a.predictive(mode, rows=False), b.predictive(mode, rows=False)
            assert pa["counts"] == pb["counts"], (name, mode, pa["counts"], pb["counts"])
            assert abs(pa["total"] - pb["total"]) <= 1e-9 * abs(pb["total"]), (name, mode, pa["total"], pb["total"])
    a.close(); b.close()


# ---- (e) the contract of the dim > 1 chain scan ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 16])
def test_dim_gt_1_chain_scan_refuses_a_tail_and_the_other_schedules_take_it(hip_lib, d):
    """the degree-1 end is off the chains: it would read a message the scan does not produce (cx_api_mv.hip)"""
    name = MD.case_name("gen", MD.READER_T if d <= 4 else MD.CORE_T, d, None, 5)
    r = ref(name)
    model = r["model"]
    dev = make_dev(model, L.SCHED_CHAIN_SCAN)
    with pytest.raises(cx.CortexHipError) as err:
        dev.sweep(1)
    assert err.value.code == L.ERR_UNSUPPORTED and "degree 1" in err.value.message
    dev.close()
    n = len(model.x_ids)
    for schedule, sweeps in ((L.SCHED_TREE, 1), (L.SCHED_REFERENCE, 1), (L.SCHED_FUSED, n + 8)):
        dev = make_dev(model, schedule)
        dev.sweep(sweeps)
        check_marginals(dev, model, r["mean"], r["cov"], 1e-9 if d <= 4 else 1e-8, f"{name} schedule {schedule}")
        dev.close()
    sname = MD.case_name("lin", MD.READER_T, 1, None, 5)
    one_exact_sweep(sname, L.SCHED_CHAIN_SCAN, sname + " scalar chain scan").close()


# ---- (f) the end message left unset ------------------------------------------------------------------------------------------------------
def unset_end_pattern(model):
    """the lazy numpy BP on the model with its degree-1 ends' messages UNDEFINED (a NaN opaque message on each): which messages into
    latent variables and which marginals are defined at the fixed point"""
    d = model.dim
    v, f = MD.flat_end_edges(model)
    gm = E.gmodel(model, opaque=(v, f, np.full((len(v), d), np.nan), np.full((len(v), d, d), np.nan)))
    f2v = E.numpy_bp(gm, max_iter=len(model.x_ids) + 4)
    nv = len(gm.var_ids)
    bad = np.zeros(nv, bool)                 # (the end's own marginal is the product of the messages INTO it: the forward message alone)
    g = gm.groups[2]
    e, l = f2v[2]
    undefined = np.isnan(e).any(axis=2) | np.isnan(l).any(axis=(2, 3))             # [n, 2]
    np.logical_or.at(bad, g["vars"].reshape(-1), undefined.reshape(-1))
    into_free = ~gm.obs[g["vars"]]
    return gm, bad, g["fid"], g["vars"], undefined, into_free


@pytest.mark.parametrize("family,d,schedule", [("ssm", 1, L.SCHED_CHAIN_SCAN), ("lin", 1, L.SCHED_CHAIN_SCAN), ("lin", 1, L.SCHED_TREE), ("gen", 2, L.SCHED_TREE)],
                         ids=["ssm-scan", "lin-scan", "lin-tree", "gen2-tree"])
def test_an_unset_end_message_leaves_the_component_undefined(hip_lib, family, d, schedule):
    """flat and undefined are different things: with the tail's end message left unset the forward messages are computed, the backward
    ones stay undefined and with them every marginal of the component but the end's own (the product of the messages INTO the end:
    the forward message alone), the evidence is NaN — and the calls return CX_OK"""
    model = MD.make(family, 12, d, None, 3)
    gm, bad, fid, vars_, undefined, into_free = unset_end_pattern(model)
    xi = np.searchsorted(gm.var_ids, model.x_ids)
    assert bad[xi][:-1].all() and not bad[xi][-1] and (~undefined & into_free).sum() >= len(model.x_ids) - 1, "the reference: the forward messages, no marginal but the end's own"
    dev = make_dev(model, schedule, flat_ends=False)
    dev.sweep(1)
    marg = dev.get_marginals(model.x_ids)
    assert np.array_equal(np.isnan(marg).any(axis=1), bad[xi]), marg
    sel = into_free.reshape(-1)
    msgs = dev.get_messages(gm.var_ids[vars_.reshape(-1)][sel], np.repeat(fid, 2)[sel], L.TO_VARIABLE, L.FORM_NATURAL)
    assert np.array_equal(np.isnan(msgs).any(axis=1), undefined.reshape(-1)[sel]), "which factor→variable messages are undefined"
    value, cnt = dev.log_evidence()
    assert np.isnan(value) and cnt["undefined"] > 0, (value, cnt)
    dev.close()


# ---- (g) new data between sweeps -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,d,T", [("ssm", 1, MD.SCALAR_T), ("lin", 1, MD.READER_T), ("gen", 4, MD.MV_T), ("gen", 16, MD.CORE_T)])
def test_new_data_between_sweeps(hip_lib, monkeypatch, family, d, T):
    """the cached side sums must not depend on a side message being there: sweep, move the data, sweep, and compare with the reference of
    the new data"""
    if d > 4:
        monkeypatch.setenv("CX_MVC64_K", str(MD.CORE_K))
        monkeypatch.setenv("CX_MVC64_FAN", str(MD.CORE_FAN))
    name = MD.case_name(family, T, d, "alt", 0)
    r = ref(name)
    model = r["model"]
    dev = make_dev(model, L.SCHED_CHAIN_SCAN)
    dev.sweep(1)
    check_marginals(dev, model, r["mean"], r["cov"], 1e-9, name)
    y2 = np.asarray(model.data_y) * 0.5 + np.random.default_rng(7).standard_normal(np.shape(model.data_y))
    dev.set_messages(model.data_var, model.data_fac, L.TO_FACTOR, L.FORM_POINT, y2)
    dev.sweep(1)
    k = MD.kalman_missing(MD.with_data(model, y2))
    check_marginals(dev, model, k["mean"], k["cov"], 1e-9, name + " after new data")
    check_healthy(dev, name)
    dev.close()


def test_the_readme_example(hip_lib):
    """README, Use: a random walk with a datum at every third step and twenty steps ahead, built from plain arrays"""
    T, h = 600, 20
    n = T + h
    x = np.arange(1, n + 1)
    seen = x[:T:3]
    y, lik, tr = seen + n, seen + 2 * n, 3 * n + x[:-1]
    data = np.cumsum(np.random.default_rng(3).standard_normal(T) * 0.3)[::3]
    model = cx.synth.Model(edge_var=np.r_[y, seen, x[:-1], x[1:]], edge_fac=np.r_[lik, lik, tr, tr], factor_ids=np.r_[lik, tr],
                           factor_kind=np.full(len(lik) + n - 1, L.FACTOR_GAUSS_ADDITIVE, np.int32),
                           factor_var=np.r_[np.full(len(lik), 0.5), np.full(n - 1, 0.1)], x_ids=x, data_var=y, data_fac=lik, data_y=data)
    dev = cx.DeviceGraph(schedule=L.SCHED_CHAIN_SCAN)
    dev.graph_create(model.edge_var, model.edge_fac, model.factor_ids, model.factor_kind, model.factor_var)
    dev.set_messages(y, lik, L.TO_FACTOR, L.FORM_POINT, data)
    dev.set_messages([x[-1]], [tr[-1]], L.TO_FACTOR, L.FORM_NATURAL, [0.0, 0.0])
    dev.sweep(1)
    gm = E.gmodel(model)
    mean, S, fpos = LS.dense_posterior(gm)
    xi = np.searchsorted(gm.var_ids, x)
    marg = dev.get_marginals(x)
    assert_close(marg[:, 0], mean[xi, 0], 1e-9, "means")
    assert_close(marg[:, 1], np.diag(S)[fpos[xi]], 1e-9, "variances")
    last = int(np.flatnonzero(np.isin(x, seen))[-1])
    ahead = dev.get_marginals(x[T:])
    assert_close(np.diff(marg[last:, 1]), np.full(n - 1 - last, 0.1), 1e-9, "the variance grows by q a step behind the last datum")
    assert_close(ahead[:, 0], np.full(h, marg[last, 0]), 1e-9, "a random walk's forecast is its last smoothed mean")
    dev.close()
