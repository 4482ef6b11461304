"""-m gpu: cx_linear_moments_mfma — exact mean and covariance of linear functionals at the matrix-core dims (cx_create dim 5 .. 64;
DESIGN.md §4s) — against the dense posterior (functional_support.dense_moments: W μ and W Σ Wᵀ), against cx_sample_posterior_mfma on the
same handle through identity noise, and against itself across tile sizes, chunks, panels and handles.  The models are those of
tests/sample_mfma_support.py and the functionals functional_support.standard_functionals (units, contrasts, a window mean, dense random
weights, a repeated id, one functional with and without a weight on an observed variable: K between 33 and 1289, many panels);
tests/test_functional_mfma_checker.py pins the references and the uncentred recursion on them on the CPU (1e-12).

Tolerances, measured by functional_support.rel_errors (covariances relative to sqrt(cov_kk cov_ll), means to the posterior spread):
TOL = 1e-9 against the exact references, SAME = 1e-12 between tile sizes or paths that compute the same thing in another order
(tests/sample_mfma_support.py).  Every test prints its largest observed error."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from tests import anisotropic as AN
from tests import evidence_mfma_support as S
from tests import evidence_support as E
from tests import functional_support as FS
from tests import learning_support as LS
from tests import missing_data as MD
from tests import predictive_mfma_support as PM
from tests import sample_mfma_support as SM
from tests import sampling_support as SS
from tests.gpu_support import assert_reader_refusals, code_of, demo_chain_model, run_demo, under_capture
from tests.gpu_support import loaded_device as _load

pytestmark = pytest.mark.gpu
TOL, SAME = SM.TOL, SM.SAME
WHO = "cx_linear_moments_mfma"
MODELS = SM.models()
_REFS = {}


def _reference(model, opaque=None, key=None):
    """(gm, functionals, names, dense mean [K], dense cov [K, K], dense posterior); made once per key"""
    if key is not None and key in _REFS:
        return _REFS[key]
    gm = E.gmodel(model, opaque=opaque) if opaque is not None else E.gmodel(model)
    dense = LS.dense_posterior(gm)
    fs, names = FS.standard_functionals(gm)
    rm, rc = FS.dense_moments(gm, fs, dense=dense)
    ref = (gm, fs, names, rm, rc, dense)
    if key is not None:
        _REFS[key] = ref
    return ref


def _named(name):
    model, opaque, how = MODELS[name]()
    return model, opaque, how, _reference(model, opaque, key=name)


def _within(mean, cov, ref_mean, ref_cov, tol, what):
    em, ec = FS.rel_errors(mean, cov, ref_mean, ref_cov)
    print(what, "mean", em, "cov", ec)
    assert np.isfinite(mean).all() and (cov is None or np.isfinite(cov).all()), what
    assert em <= tol and ec <= tol, (what, em, ec)


def _exact(dev, ref, what, components=1):
    """mean and cov of the standard functionals against dense within TOL; the counts; returns (mean, cov)"""
    gm, fs, _names, rm, rc, _dense = ref
    mean, cov, cnt = dev.linear_moments_mfma(fs)
    assert mean.shape == (len(fs),) and cov.shape == (len(fs), len(fs))
    assert cnt == {"components": components, "failed": 0, "nan_functionals": 0, "free": int((~gm.obs).sum())}, (what, cnt)
    _within(mean, cov, rm, rc, TOL, what)
    return mean, cov


# ---- 1. exact after every schedule -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["chain", "comb"])
@pytest.mark.parametrize("d", PM.SCHEDULE_DIMS)
def test_exact_after_every_schedule(hip_lib, d, shape):
    """comb: a second light depth, the pulls of the teeth injected into the spine"""
    model, _o, _h, ref = _named(f"{shape} d={d}")
    for s in [L.SCHED_TREE, L.SCHED_REFERENCE] + ([L.SCHED_CHAIN_SCAN] if shape == "chain" else []):
        dev = _load(model, schedule=s)
        _exact(dev, ref, f"d {d} {shape} schedule {s}")
        dev.close()


# ---- 2. both link directions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [f"two parents d={d}" for d in SM.TWO_PARENT_DIMS] + ["branching d=16"])
def test_both_link_directions(hip_lib, name):
    model, _o, _h, ref = _named(name)
    dev = _load(model)
    _exact(dev, ref, name)
    dev.close()


# ---- 3. tile levels and injection into tiled paths ---------------------------------------------------------------------------------------
def _tiled_and_flat(model, ref, tile, what, monkeypatch):
    monkeypatch.setenv("CX_SAMPLE_MFMA_TILE", str(tile))      # read when the plan is built: before the handle's first call
    dev = _load(model)
    tm, tc = _exact(dev, ref, f"{what} tiles of {tile}")
    dev.close()
    monkeypatch.delenv("CX_SAMPLE_MFMA_TILE")
    dev = _load(model)
    fm, fc = _exact(dev, ref, f"{what} the default tile")
    dev.close()
    _within(tm, tc, fm, fc, SAME, f"{what} tiles of {tile} against the default tile")


@pytest.mark.parametrize("T,d,levels", SM.TILED)
def test_tile_levels(hip_lib, T, d, levels, monkeypatch):
    """tiles of 4 items: three levels (4, 16, 64) on 70 states, two on 22 and 20 — every compose and walk kernel of the adjoint scan"""
    assert SM.tile_levels(T, SM.TILE) == levels
    model, _o, _h, ref = _named(f"long chain T={T} d={d}")
    _tiled_and_flat(model, ref, SM.TILE, f"T {T} d {d}", monkeypatch)


@pytest.mark.parametrize("d", [16, 17])
def test_injection_into_a_tiled_path(hip_lib, d, monkeypatch):
    """tiles of 2 items: the teeth of the comb hang on a spine that is itself tiled"""
    model, _o, _h, ref = _named(f"comb d={d}")
    _tiled_and_flat(model, ref, 2, f"comb d {d}", monkeypatch)


# ---- 4. gaps, a forecast tail, a leading gap, an opaque prior, a clamped state -----------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in MODELS if n.split(" d=")[0] in ("gen alt tail", "leading gap", "prior", "clamped middle")])
def test_gaps_tails_priors_and_a_clamped_state(hip_lib, name):
    model, opaque, how, ref = _named(name)
    dev = _load(model, opaque, how)
    clamped = name.startswith("clamped")
    _exact(dev, ref, name, components=2 if clamped else 1)
    if clamped:      # two components: nothing joins a state before the clamp and one after it
        gm = ref[0]
        free = gm.var_ids[~gm.obs]
        one = np.ones((1, gm.d))
        _m, cov, cnt = dev.linear_moments_mfma([([free[0]], one), ([free[-1]], one)])
        assert cnt["components"] == 2 and cov[0, 1] == 0.0 and cov[1, 0] == 0.0 and cov[0, 0] > 0.0 and cov[1, 1] > 0.0, cov
    dev.close()


# ---- 5. embedded dims ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [5, 17])
def test_embedded_dims_at_any_tile_size(hip_lib, d, monkeypatch):
    model, _o, _h, ref = _named(f"comb d={d}")
    dev = _load(model)
    nm, nc = _exact(dev, ref, f"d {d} native")
    dev.close()
    monkeypatch.setenv("CX_MFMA_DIM", "64")
    dev = _load(model)
    monkeypatch.delenv("CX_MFMA_DIM")
    fm, fc = _exact(dev, ref, f"d {d} in 4 x 4 tiles")      # (every output finite: the padding never shows)
    _within(fm, fc, nm, nc, SAME, f"d {d}: 4 x 4 tiles against the native tile")
    dev.close()


# ---- 6. invariances, bit for bit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain d=16", "comb d=17"])
def test_invariances(hip_lib, name, monkeypatch):
    model, _o, _h, ref = _named(name)
    gm, fs, names, rm, rc, _dense = ref
    assert len(fs) > 40
    dev = _load(model)
    mean, cov, cnt = dev.linear_moments_mfma(fs)
    m2, c2, _ = dev.linear_moments_mfma(fs)
    assert mean.tobytes() == m2.tobytes() and cov.tobytes() == c2.tobytes()                     # two calls: the same bits
    assert np.array_equal(cov, cov.T)                                                            # exactly symmetric
    for k in (0, 15, 16, 33, names.index("window mean"), names.index("dense"), len(fs) - 1):    # alone against among the others
        m1, c1, _ = dev.linear_moments_mfma([fs[k]])
        assert m1[0] == mean[k] and c1[0, 0] == cov[k, k], (k, names[k])
    for K in (1, 16, 17, 33, 40):                                                                # prefixes: whole and partial panels
        mk, ck, _ = dev.linear_moments_mfma(fs[:K])
        assert np.array_equal(mk, mean[:K]) and np.array_equal(ck, cov[:K, :K]), K
    monkeypatch.setenv("CX_FN_MFMA_CHUNK", "16")                                                 # read per call: several chunks
    m3, c3, _ = dev.linear_moments_mfma(fs)
    monkeypatch.delenv("CX_FN_MFMA_CHUNK")
    assert np.array_equal(m3, mean) and np.array_equal(c3, cov)
    m4, c4, cnt4 = dev.linear_moments_mfma(fs, cov=False)
    assert c4 is None and np.array_equal(m4, mean) and cnt4 == cnt
    # a repeated id is the summed weight
    ids, w = fs[names.index("repeat")]
    assert ids[0] == ids[2]
    ms, cs, _ = dev.linear_moments_mfma([(ids, w), ([ids[0], ids[1]], np.stack([w[0] + w[2], w[1]]))])
    _within(ms[:1], cs[:1, :1], ms[1:], cs[1:, 1:], SAME, name + " a repeated id against the summed weight")
    # with and without a weight on an observed variable: the same covariances, the means differ by w'·datum
    a, b = names.index("without observed"), names.index("with observed")
    assert np.array_equal(cov[a], cov[b]) and np.array_equal(cov[:, a], cov[:, b])
    o, wo = fs[b][0][-1], fs[b][1][-1]
    shift = float(wo @ gm.y[np.searchsorted(gm.var_ids, o)])
    assert abs((mean[b] - mean[a]) - shift) <= SAME * max(abs(shift), np.sqrt(rc[a, a])), (mean[b] - mean[a], shift)
    m0, c0, cnt0 = dev.linear_moments_mfma([])                                                   # K = 0: the counts alone
    assert m0.shape == (0,) and c0.shape == (0, 0) and cnt0 == cnt
    dev.close()


# ---- 7. against the sampler on the same handle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain d=16", "comb d=17", "two parents d=20"])
def test_against_the_sampler_on_the_same_handle(hip_lib, name):
    model, _o, _h, ref = _named(name)
    gm, fs, _names, rm, rc, _dense = ref
    nv, d = len(gm.var_ids), gm.d
    dev = _load(model)
    eps = SS.identity_noise(gm)
    x0, _ = dev.sample_posterior_mfma(1, noise=np.zeros((1, nv, d)))
    x, _ = dev.sample_posterior_mfma(len(eps), noise=eps)
    mean, cov, _ = dev.linear_moments_mfma(fs)
    W = FS.weight_matrix(gm, fs)
    WB = W[:, ~gm.obs, :].reshape(len(W), -1) @ SS.samples_to_b(x, x0[0], gm)
    _within(mean, cov, np.einsum("kvi,vi->k", W, x0[0]), WB @ WB.T, SAME, name + " W x0 and (W B)(W B)' of the sampler")
    # the unit functionals of one state: the marginal covariance block
    v = gm.var_ids[~gm.obs][len(gm.var_ids[~gm.obs]) // 2]
    blk = dev.posterior_covariance_mfma(v, v)
    marg = dev.get_marginals([v])[0]
    want = marg[d:d + d * d].reshape(d, d)
    sd = np.sqrt(np.diag(want))
    err = float(np.max(np.abs(blk - want) / np.outer(sd, sd)))
    print(name, "marginal block", err)
    assert err <= TOL, err
    cv = dev.contrast_variance_mfma(v, gm.var_ids[~gm.obs][0])
    assert np.isfinite(cv) and cv > 0.0
    dev.close()


# ---- 8. failed components ---------------------------------------------------------------------------------------------------------------------
def _two_components(dev, first, ids, free2, d, what, failed_counts):
    """functionals on the first component match its own dense posterior, those touching the second are NaN with their rows and columns"""
    gm, fs1, _names, rm, rc, _dense = _reference(first, key=what + " first")
    one = np.ones((1, d))
    bad = [([v], one) for v in ids[free2][:2]] + [([fs1[0][0][0], ids[free2][0]], np.concatenate([one, -one]))]
    fs = fs1 + bad
    mean, cov, cnt = dev.linear_moments_mfma(fs)
    K1 = len(fs1)
    assert cnt == {"components": 2, "failed": 1, "nan_functionals": len(bad), "free": failed_counts}, cnt
    assert np.isnan(mean[K1:]).all() and np.isnan(cov[K1:]).all() and np.isnan(cov[:, K1:]).all()
    _within(mean[:K1], cov[:K1, :K1], rm, rc, TOL, what)
    m1, _c, cnt1 = dev.linear_moments_mfma(fs, cov=False)
    assert np.array_equal(m1, mean, equal_nan=True) and cnt1 == cnt


def test_a_component_without_information_is_nan(hip_lib):
    first = AN.chain(5, 16)
    model = cx.synth.concat_models([first, MD.thin(AN.chain(4, 16), np.zeros(4, bool))])
    ids = np.unique(model.edge_var)
    n1 = len(np.unique(first.edge_var))
    assert len(ids) == 14 and np.array_equal(ids[:n1], np.unique(first.edge_var))
    dev = cx.DeviceGraph(dim=16, schedule=L.SCHED_TREE)
    MD.load(model, dev)
    dev.sweep(1)
    _two_components(dev, first, ids, np.arange(len(ids)) >= n1, 16, "beside a component without information", 9)
    dev.close()


def test_a_component_with_an_undefined_input_is_nan(hip_lib):
    first = AN.chain(5, 16)
    model = cx.synth.concat_models([first, MD.tail(AN.chain(4, 16), 2)])
    ids = np.unique(model.edge_var)
    n1 = len(np.unique(first.edge_var))
    dev = cx.DeviceGraph(dim=16, schedule=L.SCHED_TREE)
    MD.load(model, dev, flat_ends=False)      # the last state of the tail never sends: every message behind it is undefined
    dev.sweep(1)
    free2 = (np.arange(len(ids)) >= n1) & np.isin(ids, model.x_ids)
    _two_components(dev, first, ids, free2, 16, "beside an undefined component", 5 + int(free2.sum()))
    dev.close()


# ---- 9. new parameters ----------------------------------------------------------------------------------------------------------------------
def test_new_parameters_are_read_by_the_next_call(hip_lib):
    model, _o, _h, ref = _named("chain d=16")
    dev = _load(model)
    _exact(dev, ref, "old (A, Q)")
    psets = dict(model.psets)
    psets[0] = (psets[0][0], 2.0 * np.asarray(psets[0][1]))
    dev.set_factor_matrices(0, *psets[0])
    dev.sweep(1)
    new = _reference(dataclasses.replace(model, psets=psets, meta={**model.meta, "Q": psets[0][1]}))
    assert np.max(np.abs(new[4] - ref[4])) > 1e-3
    _exact(dev, new, "new (A, 2 Q)")      # the links are per call
    dev.close()


# ---- 10. moves nothing ----------------------------------------------------------------------------------------------------------------------
def test_moves_nothing(hip_lib):
    model, _o, _h, ref = _named("chain d=16")
    fs = ref[1]
    for s in (L.SCHED_CHAIN_SCAN, L.SCHED_REFERENCE, L.SCHED_TREE):
        dev = _load(model, schedule=s)
        if s == L.SCHED_CHAIN_SCAN:      # (another reader first: every reader of the messages brings them to their slots)
            dev.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE)
        blob, marg, health = dev.export_state(), dev.get_marginals(model.x_ids), np.asarray(dev.message_health())
        msgs = dev.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE)
        dev.linear_moments_mfma(fs[:20])      # the FIRST call: it builds the plan and allocates the links
        dev.linear_moments_mfma(fs, cov=False)
        assert np.array_equal(blob, dev.export_state()) and np.array_equal(marg, dev.get_marginals(model.x_ids))
        assert np.array_equal(msgs, dev.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE), equal_nan=True)
        assert np.array_equal(health, np.asarray(dev.message_health()))
        dev.close()


# ---- 11. one handle -------------------------------------------------------------------------------------------------------------------------
def test_one_handle_with_the_sampler_follows_the_observed_flags(hip_lib):
    """a handle that called both entries before a state is observed (one plan, one link workspace, reused and rebuilt) against a twin with
    the same history that never called either: byte for byte"""
    model = AN.chain(9, 16)
    d, i = 16, 4
    x = model.x_ids[i]
    facs = np.asarray(model.edge_fac)[np.asarray(model.edge_var) == x]
    value = np.random.default_rng(84).standard_normal(d)
    a, b = _load(model), _load(model)
    nv = a.stats()["n_variables"]
    eps = SS.normals(11, np.arange(18), nv, d)
    a.sample_posterior_mfma(18, noise=eps)
    _exact(a, _reference(model, key="AN.chain(9, 16)"), "before the clamp")
    for dev in (a, b):
        dev.set_messages(np.full(len(facs), x), facs, L.TO_FACTOR, L.FORM_POINT, np.tile(value, (len(facs), 1)))
        dev.sweep(1)
    clamped = dataclasses.replace(model, data_var=np.concatenate([model.data_var, np.full(len(facs), x)]), data_fac=np.concatenate([model.data_fac, facs]),
                                  data_y=np.vstack([model.data_y, np.tile(value, (len(facs), 1))]))
    ref = _reference(clamped, key="AN.chain(9, 16) clamped")
    ma, ca = _exact(a, ref, "after the clamp", components=2)
    xa, cnta = a.sample_posterior_mfma(18, noise=eps)
    mb, cb, _ = b.linear_moments_mfma(ref[1])
    xb, cntb = b.sample_posterior_mfma(18, noise=eps)
    assert ma.tobytes() == mb.tobytes() and ca.tobytes() == cb.tobytes()
    assert xa.tobytes() == xb.tobytes() and cnta == cntb and cnta["components"] == 2 and cnta["free"] == 8
    a.close(); b.close()


# ---- 12. refusals -----------------------------------------------------------------------------------------------------------------------------
def _one(dev):
    """the cheapest functional: the sum of the entries of variable 1, at the handle's dim"""
    return [([1], np.ones((1, dev.dim)))]


def _raw_one(dev):
    """_one(dev) through the C ABI; the status"""
    off, ids, w = FS.as_csr(_one(dev), dev.dim)
    p64, pd = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    mean, cov = np.zeros(1), np.zeros((1, 1))
    return dev.lib.cx_linear_moments_mfma(dev.h, 1, off.ctypes.data_as(p64), ids.ctypes.data_as(p64), w.ctypes.data_as(pd),
                                          mean.ctypes.data_as(pd), cov.ctypes.data_as(pd), (C.c_int64 * 4)())


def test_refusals(hip_lib):
    assert_reader_refusals(WHO, "cx_linear_moments", lambda dev: dev.linear_moments_mfma(_one(dev)), lambda dev: dev.linear_moments(_one(dev)), _raw_one)
    m16 = cx.synth.lgssm_chain(4, d=16, seed=92)
    one16 = [([int(m16.x_ids[0])], np.ones((1, 16)))]
    dev = cx.DeviceGraph(dim=16, schedule=L.SCHED_FUSED)      # a cycle among the non-observed variables
    ring = S.ring(16)
    cx.synth.load_into_device(ring, dev, seed_variance=1e6)
    dev.sweep(3)
    code, msg = code_of(dev.linear_moments_mfma, [([int(ring.x_ids[0])], np.ones((1, 16)))])
    assert code == L.ERR_UNSUPPORTED and msg.startswith(WHO) and "cycle" in msg and "variable" in msg, msg
    dev.close()
    dev = _load(m16)
    code, msg = code_of(dev.linear_moments, one16)
    assert code == L.ERR_UNSUPPORTED and "cx_linear_moments" in msg and WHO not in msg      # the old call keeps refusing these dims
    # the argument errors of cx_linear_moments, through the C ABI: a refused call writes nothing
    off, ids, w = FS.as_csr(one16, 16)
    mean, cov, cnt = np.full(1, 7.0), np.full((1, 1), 7.0), (C.c_int64 * 4)(7, 7, 7, 7)
    po, pi, pw = (a.ctypes.data_as(C.POINTER(t)) for a, t in ((off, C.c_int64), (ids, C.c_int64), (w, C.c_double)))
    pm, pc = mean.ctypes.data_as(C.POINTER(C.c_double)), cov.ctypes.data_as(C.POINTER(C.c_double))
    dec, start1 = np.array([0, 1, 0], np.int64), np.array([1, 1], np.int64)
    pdec, pst = dec.ctypes.data_as(C.POINTER(C.c_int64)), start1.ctypes.data_as(C.POINTER(C.c_int64))
    call = dev.lib.cx_linear_moments_mfma
    for args in ((-1, po, pi, pw, pm, pc, cnt), (32769, po, pi, pw, pm, pc, cnt), (1, None, pi, pw, pm, pc, cnt), (1, po, pi, pw, None, pc, cnt),
                 (1, po, pi, pw, pm, pc, None), (1, po, None, pw, pm, pc, cnt), (1, po, pi, None, pm, pc, cnt), (2, pdec, pi, pw, pm, pc, cnt),
                 (1, pst, pi, pw, pm, pc, cnt)):
        if args[0] == 32769:
            big = np.zeros(32770, np.int64)
            args = (32769, big.ctypes.data_as(C.POINTER(C.c_int64))) + args[2:]
        assert call(dev.h, *args) == L.ERR_INVALID_ARGUMENT, args
        assert dev.lib.cx_last_error(dev.h).decode().startswith(WHO)
    assert mean[0] == 7.0 and cov[0, 0] == 7.0 and list(cnt) == [7, 7, 7, 7]
    code, msg = code_of(dev.linear_moments_mfma, [([int(m16.x_ids[0]), 10 ** 9], np.ones((2, 16)))])
    assert code == L.ERR_NOT_FOUND and msg.startswith(WHO) and str(10 ** 9) in msg
    want = dev.linear_moments_mfma(one16)      # and the handle works on
    assert call(dev.h, 1, po, pi, pw, pm, None, cnt) == L.OK and list(cnt) == [1, 0, 0, 4] and mean[0] == want[0][0] and cov[0, 0] == 7.0
    mean[:] = 7.0
    rc, msg = under_capture(dev, lambda: call(dev.h, 1, po, pi, pw, pm, pc, cnt))
    assert rc == L.ERR_STATE and msg.startswith(WHO) and "captured" in msg, (rc, msg)
    assert mean[0] == 7.0 and cov[0, 0] == 7.0      # a refused call writes nothing
    again = dev.linear_moments_mfma(one16)
    assert np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1])
    dev.close()


# ---- 13. the C++ host class -------------------------------------------------------------------------------------------------------------------
def test_cpp_host_class_linear_moments_mfma(hip_lib, tmp_path):
    rows = {line.split()[0]: [float(v) for v in line.split()[1:]] for line in run_demo("linear_moments_mfma_demo", tmp_path)}
    T, d = 12, 16
    model = demo_chain_model(T, d)
    e0 = np.eye(d)[:1]
    fs = [(np.arange(3, 9), np.full((6, d), 1.0 / (6 * d))), ([2], e0), ([11], e0),
          ([1, 12, T + 5], np.concatenate([np.ones((1, d)), -np.ones((1, d)), 2.0 * np.ones((1, d))]))]
    gm = E.gmodel(model)
    rm, rc = FS.dense_moments(gm, fs)
    assert rows["counts"] == [1, 0, 0, T] and rows["sizes"] == [4, 16, 4, 0]
    cm, cc = np.asarray(rows["mean"]), np.asarray(rows["cov"]).reshape(4, 4)
    assert rows["means_only"] == rows["mean"]
    _within(cm, cc, rm, rc, TOL, "C++ against dense")
    dev = _load(model, schedule=L.SCHED_CHAIN_SCAN)
    pm, pc, _ = dev.linear_moments_mfma(fs)
    _within(cm, cc, pm, pc, SAME, "C++ against Python")
    dev.close()
