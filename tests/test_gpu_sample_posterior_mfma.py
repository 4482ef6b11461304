"""-m gpu: cx_sample_posterior_mfma — joint posterior samples at the matrix-core dims (cx_create dim 5 .. 64) — against the
dense posterior (its mean under ε = 0, and B Bᵀ = Σ through identity noise), the numpy restatement of the device generator
(tests/sampling_support.py) and itself across tile sizes, chunks, panels and handles.  The models are those of
tests/sample_mfma_support.py; tests/test_sample_mfma_checker.py pins the references on them on the CPU (B Bᵀ = Σ to 1e-13).

Tolerances: TOL = 1e-9 against the exact references, scaled as tests/test_gpu_posterior_samples.py scales (by max(|want|, 1) per entry;
max|B Bᵀ - Σ| <= 1e-9 max|Σ|); SAME = 1e-12 between tile sizes and between the Philox path and its restatement.  A call is the affine
map x = mean + B ε (tests 1 - 5) and the device's ε are the restated Philox normals (test 6), whose moments tests/test_sampling_checker.py
pins on the CPU: there is no Monte-Carlo test."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from tests import anisotropic as AN
from tests import evidence_mfma_support as S
from tests import evidence_support as E
from tests import learning_support as LS
from tests import missing_data as MD
from tests import predictive_mfma_support as PM
from tests import sample_mfma_support as SM
from tests import sampling_support as SS
from tests.gpu_support import assert_reader_refusals, code_of, demo_chain_model, run_demo, under_capture
from tests.gpu_support import loaded_device as _load

pytestmark = pytest.mark.gpu
TOL, SAME = SM.TOL, SM.SAME
WHO = "cx_sample_posterior_mfma"
MODELS = SM.models()


def _close(got, want, rtol, what=""):
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = np.maximum(np.abs(want), 1.0)
    err = float(np.max(np.abs(got - want) / scale)) if got.size else 0.0
    print(what, err)
    assert err <= rtol, (what, err)


def _reference(model, opaque=None):
    gm = E.gmodel(model, opaque=opaque) if opaque is not None else E.gmodel(model)
    mean, Sig, _ = LS.dense_posterior(gm)
    return gm, mean, Sig, SS.identity_noise(gm)


def _exact(dev, ref, what, components=1):
    """ε = 0 gives the dense mean, identity noise B Bᵀ = Σ, the observed rows are the data bit for bit, the counts are right; returns the
    identity-noise samples"""
    gm, mean, Sig, eps = ref
    nv, d = len(gm.var_ids), gm.d
    x0, cnt = dev.sample_posterior_mfma(1, noise=np.zeros((1, nv, d)))
    assert x0.shape == (1, nv, d)
    assert cnt == {"free": int((~gm.obs).sum()), "components": components, "undefined": 0, "not_positive_definite": 0}, (what, cnt)
    _close(x0[0], mean, TOL, what + " mean")
    x, _ = dev.sample_posterior_mfma(len(eps), noise=eps)
    B = SS.samples_to_b(x, mean, gm)
    err = np.max(np.abs(B @ B.T - Sig)) / np.max(np.abs(Sig))
    print(what, "B B'", err)
    assert err <= TOL, (what + " B B'", err)
    assert np.array_equal(x[:, gm.obs], np.broadcast_to(gm.y[gm.obs], x[:, gm.obs].shape)), what + " data"
    return x


# ---- 1. exact mean and covariance after every schedule ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["chain", "comb"])
@pytest.mark.parametrize("d", PM.SCHEDULE_DIMS)
def test_exact_mean_and_covariance(hip_lib, d, shape):
    """comb: a second light depth, a path that starts from a parent written by the depth before"""
    model = PM.chain(d) if shape == "chain" else PM.comb(d)
    ref = _reference(model)
    for s in [L.SCHED_TREE, L.SCHED_REFERENCE] + ([L.SCHED_CHAIN_SCAN] if shape == "chain" else []):
        dev = _load(model, schedule=s)
        _exact(dev, ref, f"d {d} {shape} schedule {s}")
        dev.close()


# ---- 2. both link directions and more than three sources -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [f"two parents d={d}" for d in SM.TWO_PARENT_DIMS] + ["branching d=16"])
def test_both_link_directions_and_four_sources(hip_lib, name):
    """two parents: on the path through the state with two parents one link has its child at the OUT end and the next at the IN end,
    whichever end is the root; the inner states of both models sum four records.  The posterior is proper: the dense solve is the reference"""
    model, _o, _h = MODELS[name]()
    dev = _load(model)
    _exact(dev, _reference(model), name)
    dev.close()


# ---- 3. tile levels --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,d,levels", SM.TILED)
def test_tile_levels(hip_lib, T, d, levels, monkeypatch):
    """tiles of 4 items: three levels (4, 16, 64) on 70 states, two on 22 and 20 — every compose and walk kernel of the blocked scan"""
    assert SM.tile_levels(T, SM.TILE) == levels
    model = AN.chain(T, d)
    ref = _reference(model)
    monkeypatch.setenv("CX_SAMPLE_MFMA_TILE", str(SM.TILE))      # read when the plan is built: before the handle's first call
    dev = _load(model)
    tiled = _exact(dev, ref, f"T {T} d {d} tiles of {SM.TILE}")
    dev.close()
    monkeypatch.delenv("CX_SAMPLE_MFMA_TILE")
    dev = _load(model)
    flat = _exact(dev, ref, f"T {T} d {d} the default tile")
    dev.close()
    _close(tiled, flat, SAME, f"T {T} d {d} tiles of {SM.TILE} against the default tile, one ε")


# ---- 4. gaps, a forecast tail, a leading gap, an opaque prior, a clamped state -----------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in MODELS if n.split(" d=")[0] in ("gen alt tail", "leading gap", "prior", "clamped middle")])
def test_gaps_tails_priors_and_a_clamped_state(hip_lib, name):
    model, opaque, how = MODELS[name]()
    dev = _load(model, opaque, how)
    _exact(dev, _reference(model, opaque), name, components=2 if name.startswith("clamped") else 1)
    dev.close()


# ---- 5. embedded dims ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [5, 17])
def test_embedded_dims_at_any_tile_size(hip_lib, d, monkeypatch):
    model = PM.comb(d)
    nv = len(np.unique(model.edge_var))
    eps = SS.normals(3, np.arange(4), nv, d)
    dev = _load(model)
    native, seeded = dev.sample_posterior_mfma(4, noise=eps)[0], dev.sample_posterior_mfma(20, seed=5)[0]
    dev.close()
    monkeypatch.setenv("CX_MFMA_DIM", "64")
    dev = _load(model)
    monkeypatch.delenv("CX_MFMA_DIM")
    forced, cnt = dev.sample_posterior_mfma(4, noise=eps)
    assert forced.shape == (4, nv, d) and cnt["undefined"] == 0 and cnt["not_positive_definite"] == 0      # the padding never shows
    _close(forced, native, SAME, f"d {d}: 4 x 4 tiles against the native tile, one ε")
    _close(dev.sample_posterior_mfma(20, seed=5)[0], seeded, SAME, f"d {d}: 4 x 4 tiles against the native tile, one seed")
    dev.close()


# ---- 6. the generator and the invariances ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain d=16", "comb d=17"])
def test_generator_and_invariances(hip_lib, name, monkeypatch):
    model, _o, _h = MODELS[name]()
    dev = _load(model)
    nv, d = dev.stats()["n_variables"], model.dim
    x, _ = dev.sample_posterior_mfma(5, seed=7)
    y, _ = dev.sample_posterior_mfma(5, noise=SS.normals(7, np.arange(5), nv, d))
    _close(x, y, SAME, name + " Philox restated")
    assert np.array_equal(x, dev.sample_posterior_mfma(5, seed=7)[0])                      # two calls: bit-identical
    x40, _ = dev.sample_posterior_mfma(40, seed=7)
    assert np.array_equal(x40[:5], x)                                                      # across a panel boundary
    for n in (1, 17, 33):                                                                  # the partial panel
        assert np.array_equal(dev.sample_posterior_mfma(n, seed=7)[0], x40[:n]), n
    eps40 = SS.normals(7, np.arange(40), nv, d)
    y40, _ = dev.sample_posterior_mfma(40, noise=eps40)
    _close(x40, y40, SAME, name + " Philox restated, 40 samples")
    monkeypatch.setenv("CX_SAMPLE_MFMA_CHUNK", "16")                                       # read per call: across chunk boundaries
    assert np.array_equal(dev.sample_posterior_mfma(40, seed=7)[0], x40)
    assert np.array_equal(dev.sample_posterior_mfma(40, noise=eps40)[0], y40)
    assert np.array_equal(dev.sample_posterior_mfma(5, seed=7)[0], x)
    monkeypatch.delenv("CX_SAMPLE_MFMA_CHUNK")
    ids = np.unique(model.edge_var)
    sub = ids[::3][::-1]
    got, _ = dev.sample_posterior_mfma(5, seed=7, variable_ids=sub)
    assert np.array_equal(got, x[:, np.searchsorted(ids, sub)])                            # a reversed subset: the same rows
    other, _ = dev.sample_posterior_mfma(5, seed=8)
    assert not np.allclose(other, x)
    dev.close()


# ---- 7. failed components; new parameters ------------------------------------------------------------------------------------------------
def _first_component(first, x0, what):
    gm, mean, _Sig, _eps = _reference(first)
    ids = np.unique(first.edge_var)      # the first part of a concatenation keeps its ids, the lowest
    _close(x0[: len(ids)], mean[np.searchsorted(gm.var_ids, ids)], TOL, what)


def test_a_component_without_information_is_nan(hip_lib):
    first = AN.chain(5, 16)
    model = cx.synth.concat_models([first, MD.thin(AN.chain(4, 16), np.zeros(4, bool))])
    ids = np.unique(model.edge_var)
    assert len(ids) == 14
    n1 = len(np.unique(first.edge_var))
    assert np.array_equal(ids[:n1], np.unique(first.edge_var))
    dev = cx.DeviceGraph(dim=16, schedule=L.SCHED_TREE)
    MD.load(model, dev)
    dev.sweep(1)
    x0, cnt = dev.sample_posterior_mfma(1, noise=np.zeros((1, 14, 16)))
    assert cnt == {"free": 9, "components": 2, "undefined": 0, "not_positive_definite": 1}, cnt
    assert np.isnan(x0[0, n1:]).all()
    _first_component(first, x0[0], "the component beside one without information")
    x, cnt = dev.sample_posterior_mfma(3, seed=2)
    assert cnt["not_positive_definite"] == 1 and np.isnan(x[:, n1:]).all() and np.isfinite(x[:, :n1]).all()
    dev.close()


def test_a_component_with_an_undefined_input_is_nan(hip_lib):
    first = AN.chain(5, 16)
    tailed = MD.tail(AN.chain(4, 16), 2)
    model = cx.synth.concat_models([first, tailed])
    n1 = len(np.unique(first.edge_var))
    nv = len(np.unique(model.edge_var))
    dev = cx.DeviceGraph(dim=16, schedule=L.SCHED_TREE)
    MD.load(model, dev, flat_ends=False)      # the last state of the tail never sends: every message behind it is undefined
    dev.sweep(1)
    x0, cnt = dev.sample_posterior_mfma(1, noise=np.zeros((1, nv, 16)))
    assert cnt["components"] == 2 and cnt["undefined"] == 1 and cnt["not_positive_definite"] == 0, cnt
    free2 = np.isin(np.unique(model.edge_var)[n1:], model.x_ids)
    assert np.isnan(x0[0, n1:][free2]).all() and np.isfinite(x0[0, n1:][~free2]).all()      # its states NaN, its data the data
    _first_component(first, x0[0], "the component beside an undefined one")
    dev.close()


def test_new_parameters_are_read_by_the_next_call(hip_lib):
    model = PM.chain(16)
    dev = _load(model)
    _exact(dev, _reference(model), "old (A, Q)")
    psets = dict(model.psets)
    psets[0] = (psets[0][0], 2.0 * np.asarray(psets[0][1]))
    dev.set_factor_matrices(0, *psets[0])
    dev.sweep(1)
    new = dataclasses.replace(model, psets=psets, meta={**model.meta, "Q": psets[0][1]})
    ref = _reference(new)
    assert np.max(np.abs(ref[2] - _reference(model)[2])) > 1e-3
    _exact(dev, ref, "new (A, 2 Q)")      # the links are per call
    dev.close()


# ---- 8. moves nothing; one handle --------------------------------------------------------------------------------------------------------
def test_moves_nothing(hip_lib):
    model = PM.chain(16)
    for s in (L.SCHED_CHAIN_SCAN, L.SCHED_REFERENCE, L.SCHED_TREE):
        dev = _load(model, schedule=s)
        if s == L.SCHED_CHAIN_SCAN:      # (another reader first: every reader of the messages brings them to their slots)
            dev.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE)
        blob, marg, health = dev.export_state(), dev.get_marginals(model.x_ids), np.asarray(dev.message_health())
        msgs = dev.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE)
        dev.sample_posterior_mfma(3, seed=1)      # the FIRST call: it builds the plan and allocates the links
        dev.sample_posterior_mfma(20, seed=2, variable_ids=model.x_ids)
        assert np.array_equal(blob, dev.export_state()) and np.array_equal(marg, dev.get_marginals(model.x_ids))
        assert np.array_equal(msgs, dev.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE), equal_nan=True)
        assert np.array_equal(health, np.asarray(dev.message_health()))
        dev.close()


def test_one_handle_follows_the_observed_flags(hip_lib):
    """a handle that sampled before a state is observed (its plan and link workspace are reused and rebuilt) against a twin with the
    same history that never called it: byte for byte under one ε"""
    model = AN.chain(9, 16)
    d, i = 16, 4
    x = model.x_ids[i]
    facs = np.asarray(model.edge_fac)[np.asarray(model.edge_var) == x]
    value = np.random.default_rng(84).standard_normal(d)
    a, b = _load(model), _load(model)
    nv = a.stats()["n_variables"]
    eps = SS.normals(11, np.arange(18), nv, d)
    before, cnt = a.sample_posterior_mfma(18, noise=eps)
    assert cnt["components"] == 1 and cnt["free"] == 9
    for dev in (a, b):
        dev.set_messages(np.full(len(facs), x), facs, L.TO_FACTOR, L.FORM_POINT, np.tile(value, (len(facs), 1)))
        dev.sweep(1)
    xa, ca = a.sample_posterior_mfma(18, noise=eps)
    xb, cb = b.sample_posterior_mfma(18, noise=eps)
    assert ca == cb and ca["components"] == 2 and ca["free"] == 8 and ca["undefined"] == 0 and ca["not_positive_definite"] == 0, (ca, cb)
    assert xa.tobytes() == xb.tobytes()
    ids = np.unique(model.edge_var)
    assert np.array_equal(xa[:, np.searchsorted(ids, x)], np.broadcast_to(value, (18, d)))      # its datum now
    assert np.abs(xa[:, np.searchsorted(ids, model.x_ids[i - 1])] - before[:, np.searchsorted(ids, model.x_ids[i - 1])]).max() > 1e-3
    clamped = dataclasses.replace(model, data_var=np.concatenate([model.data_var, np.full(len(facs), x)]), data_fac=np.concatenate([model.data_fac, facs]),
                                  data_y=np.vstack([model.data_y, np.tile(value, (len(facs), 1))]))
    _exact(a, _reference(clamped), "after the clamp", components=2)
    a.close(); b.close()


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------------------
def _raw_one(dev):
    """one sample of every variable of a dim 16 handle of 8 variables through the C ABI; the status"""
    out = np.zeros((1, 8, 16))
    return dev.lib.cx_sample_posterior_mfma(dev.h, 1, C.c_uint64(0), None, 0, None, out.ctypes.data_as(C.POINTER(C.c_double)), (C.c_int64 * 4)())


def test_refusals(hip_lib):
    assert_reader_refusals(WHO, "cx_sample_posterior", lambda dev: dev.sample_posterior_mfma(1), lambda dev: dev.sample_posterior(1), _raw_one)
    m16 = cx.synth.lgssm_chain(4, d=16, seed=92)
    dev = cx.DeviceGraph(dim=16, schedule=L.SCHED_FUSED)      # a cycle among the non-observed variables
    cx.synth.load_into_device(S.ring(16), dev, seed_variance=1e6)
    dev.sweep(3)
    code, msg = code_of(dev.sample_posterior_mfma, 1)
    assert code == L.ERR_UNSUPPORTED and msg.startswith(WHO) and "cycle" in msg and "variable" in msg, msg
    dev.close()
    dev = _load(m16)
    code, msg = code_of(dev.sample_posterior, 1)
    assert code == L.ERR_UNSUPPORTED and "cx_sample_posterior" in msg and WHO not in msg      # the old call keeps refusing these dims
    n = 8
    out, c4 = np.zeros((2, n, 16)), (C.c_int64 * 4)()
    po = out.ctypes.data_as(C.POINTER(C.c_double))
    ids = (C.c_int64 * 1)(int(m16.x_ids[0]))
    call = dev.lib.cx_sample_posterior_mfma
    assert call(dev.h, 2, C.c_uint64(0), None, 0, None, po, c4) == L.OK and list(c4) == [4, 1, 0, 0]
    for args in ((0, C.c_uint64(0), None, 0, None, po, c4), (1, C.c_uint64(0), None, 0, None, None, c4), (1, C.c_uint64(0), None, 0, None, po, None),
                 (1, C.c_uint64(0), None, -1, ids, po, c4)):
        assert call(dev.h, *args) == L.ERR_INVALID_ARGUMENT, args
        assert dev.lib.cx_last_error(dev.h).decode().startswith(WHO)
    code, msg = code_of(dev.sample_posterior_mfma, 1, variable_ids=[int(m16.x_ids[0]), 10 ** 9])
    assert code == L.ERR_NOT_FOUND and msg.startswith(WHO) and str(10 ** 9) in msg
    want = dev.sample_posterior_mfma(3, seed=4)[0]      # and the handle works on
    out3 = np.zeros((3, n, 16))
    rc, msg = under_capture(dev, lambda: call(dev.h, 3, C.c_uint64(4), None, 0, None, out3.ctypes.data_as(C.POINTER(C.c_double)), c4))
    assert rc == L.ERR_STATE and msg.startswith(WHO) and "captured" in msg, (rc, msg)
    assert not out3.any()                                # a refused call writes nothing
    assert np.array_equal(dev.sample_posterior_mfma(3, seed=4)[0], want)
    dev.close()
    # (a factor of another kind: cx_graph_create admits none at these dims — tests/test_gpu_causal_marginals_mfma.py shows it — so the
    # refusal of mfr::checked_pairs under this call's name is a guard that no graph reaches through the API)


# ---- 10. the C++ host class --------------------------------------------------------------------------------------------------------------
def test_cpp_host_class_sample_posterior_mfma(hip_lib, tmp_path):
    rows = {line.split()[0]: [float(v) for v in line.split()[1:]] for line in run_demo("sample_mfma_demo", tmp_path)}
    T, d = 12, 16
    model = demo_chain_model(T, d)
    y = model.data_y
    gm, mean, _Sig, _eps = _reference(model)
    xs = np.searchsorted(gm.var_ids, model.x_ids)
    assert rows["counts"] == [T, 1, 0, 0] and rows["sizes"] == [T * d, 3 * T * d, 2 * T * d]
    _close(np.asarray(rows["mean"]).reshape(T, d), mean[xs], TOL, "C++ mean vs dense")
    dev = _load(model, schedule=L.SCHED_CHAIN_SCAN)
    draws, _ = dev.sample_posterior_mfma(3, seed=7, variable_ids=model.x_ids)
    _close(np.asarray(rows["draws"]).reshape(3, T, d), draws, SAME, "C++ draws vs Python")
    every, _ = dev.sample_posterior_mfma(1, seed=7)
    _close(np.asarray(rows["all"]).reshape(1, 2 * T, d), every, SAME, "C++ every variable vs Python")
    assert np.array_equal(np.asarray(rows["all"]).reshape(2 * T, d)[gm.obs], y)
    dev.close()
