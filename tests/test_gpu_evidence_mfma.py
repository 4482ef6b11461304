"""-m gpu: cx_log_evidence_mfma — log p(data) at the matrix-core dims (cx_create dim 5 .. 64) — against the dense
joint, the Kalman filter and the numpy restatement of the formula on the device's own messages (tests/evidence_support.py; the inputs of
the loop and forecast cases are pinned on the CPU by tests/test_evidence_mfma_checker.py)."""
import ctypes as C
import math

import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from tests import evidence_mfma_support as S
from tests import evidence_support as E
from tests import missing_data as MD
from tests.gpu_support import assert_reader_refusals, code_of, demo_chain, run_demo, swept_device

pytestmark = pytest.mark.gpu
DIMS = (5, 8, 16, 17, 32, 33, 64)      # 5: the least; 17, 33: the first of the next tile size; 16, 32, 64: native


def _exact(dev, want, rtol=1e-9, what=""):
    got, cnt = dev.log_evidence_mfma()
    print(what, "got", repr(got), "want", repr(want), "rel", abs(got - want) / abs(want), cnt)
    assert cnt["undefined"] == 0 and cnt["not_positive_definite"] == 0, (what, cnt)
    assert abs(got - want) <= rtol * abs(want), (what, got, want)
    return got, cnt


def _n_rule_factors(gm):
    return sum(len(g["fid"]) for g in gm.groups.values())


# ---- 1. exact after every schedule ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["chain", "comb"])
@pytest.mark.parametrize("d", DIMS)
def test_exact_after_every_schedule(hip_lib, d, shape):
    model = cx.synth.lgssm_chain(6, d=d, seed=30 + d) if shape == "chain" else cx.synth.lgssm_comb(4, d=d, teeth=1, seed=40 + d)
    gm = E.gmodel(model)
    want = E.dense_log_z(gm)
    for s in [L.SCHED_TREE, L.SCHED_REFERENCE, L.SCHED_FUSED] + ([L.SCHED_CHAIN_SCAN] if shape == "chain" else []):
        dev = swept_device(model, s)      # (fused: seed variance 1e6 and 60 sweeps, the diameter is under 20)
        _, cnt = _exact(dev, want, what=f"d {d} {shape} schedule {s}")
        assert cnt["factor_terms"] == _n_rule_factors(gm)
        assert cnt["variable_terms"] == len(model.x_ids)      # every state has two or three factors
        dev.close()


# ---- 2. the formula on the device's own messages, a loop included -------------------------------------------------------------------
@pytest.mark.parametrize("d", S.RING_DIMS)
def test_loop_matches_the_restatement_on_the_device_messages(hip_lib, d):
    model = S.ring(d)
    gm = E.gmodel(model)
    dev = swept_device(model, L.SCHED_FUSED, S.RING_SWEEPS)
    got, cnt = dev.log_evidence_mfma()
    again, _ = dev.log_evidence_mfma()
    assert np.float64(got).tobytes() == np.float64(again).tobytes()         # two calls on one state: bit-identical
    assert cnt["undefined"] == 0 and cnt["not_positive_definite"] == 0, cnt
    assert cnt["factor_terms"] == 2 * S.RING_T and cnt["variable_terms"] == S.RING_T
    f2v, opq = E.device_messages(gm, dev)
    want = E.bethe_log_z(gm, f2v, opq)
    exact = E.dense_log_z(gm)
    print("ring d", d, "got", repr(got), "bethe", repr(want), "rel", abs(got - want) / abs(want), "exact", repr(exact))
    assert abs(got - want) <= 1e-10 * abs(want), (got, want)
    assert abs(got - exact) > 1e-6 * abs(exact), (got, exact)             # the Bethe estimate, not the exact value
    dev.close()


# ---- 3. flat leaves, missing data, a forecast tail ----------------------------------------------------------------------------------
@pytest.mark.parametrize("d", S.FORECAST_DIMS)
def test_missing_data_and_a_forecast_tail(hip_lib, d):
    model, thin = S.forecast_chain(d)
    want = E.dense_log_z(E.gmodel(model))
    dev = cx.DeviceGraph(dim=d, schedule=L.SCHED_TREE)
    MD.load(model, dev)                    # the flat message on the last state's one edge
    dev.sweep(1)
    got, cnt = _exact(dev, want, what=f"forecast tail d {d}")
    dev.close()
    # the forecast states' own terms come out 0 net: the value of the chain without the tail
    dev = cx.DeviceGraph(dim=d, schedule=L.SCHED_TREE)
    MD.load(thin, dev)
    dev.sweep(1)
    short, _ = _exact(dev, want, what=f"no tail d {d}")
    assert abs(got - short) <= 1e-9 * abs(want), (got, short)
    dev.close()


# ---- 3b. opaque messages: a proper prior (its constant c_o), a flat one (no constant, no failure), a negative one (a belief that fails) --
def _opaque_dev(model, opq, schedule):
    dev = cx.DeviceGraph(dim=model.dim, schedule=schedule)
    cx.synth.load_into_device(model, dev, seed_variance=1e6 if schedule == L.SCHED_FUSED else None)
    S.set_opaque(dev, opq)
    dev.sweep(60 if schedule == L.SCHED_FUSED else 1)
    return dev


@pytest.mark.parametrize("d", S.OPAQUE_DIMS)
def test_opaque_prior_and_flat_opaque_forecast_end(hip_lib, d):
    for name, (model, opq) in (("proper prior on x_1", S.prior_chain(d)), ("flat opaque end behind a forecast tail", S.flat_opaque_tail(d))):
        gm = E.gmodel(model, opaque=opq)
        want = E.dense_log_z(gm)
        for s in (L.SCHED_TREE, L.SCHED_FUSED):
            dev = _opaque_dev(model, opq, s)
            _, cnt = _exact(dev, want, what=f"{name}, d {d}, schedule {s}")      # (not_positive_definite == 0: a flat opaque message is no failure)
            assert cnt["factor_terms"] == _n_rule_factors(gm)
            dev.close()


def test_a_first_factorisation_that_fails_counts_as_not_positive_definite(hip_lib):
    # every stored message defined; then the prior on x_2 — the OUT end of the first transition, whose both ends are free — becomes
    # negative definite WITHOUT a sweep: x_2's variable term, its likelihood's term and the FIRST factorisation of that transition
    # (Λ_{out→a} + Q⁻¹) fail, and nothing is undefined
    d = 16
    base = cx.synth.lgssm_chain(5, d=d, seed=77)
    model, f = S._with_opaque(base, base.x_ids[1:2])
    opq = (base.x_ids[1:2], f, np.zeros((1, d)), np.eye(d)[None])
    dev = _opaque_dev(model, opq, L.SCHED_TREE)
    _exact(dev, E.dense_log_z(E.gmodel(model, opaque=opq)), what="proper prior on x_2")
    S.set_opaque(dev, (opq[0], opq[1], opq[2], -100.0 * opq[3]))
    v, cnt = dev.log_evidence_mfma()
    assert math.isnan(v) and cnt["undefined"] == 0, (v, cnt)
    assert cnt["not_positive_definite"] == 4, cnt      # x_2, its likelihood, the transition out of it (second stage), the one into it (first stage)
    dev.close()


@pytest.mark.parametrize("d", [16, 40])
def test_an_observed_state_in_the_middle(hip_lib, d):
    # a factor with both ends observed, one with its OUT end and one with its IN end observed (the table towards OUT)
    model = S.clamped_middle(d)
    gm = E.gmodel(model)
    want = E.dense_log_z(gm)
    for s in (L.SCHED_TREE, L.SCHED_FUSED):
        dev = swept_device(model, s)
        _, cnt = _exact(dev, want, what=f"clamped middle d {d} schedule {s}")
        assert cnt["factor_terms"] == _n_rule_factors(gm) and cnt["variable_terms"] == len(model.x_ids) - 1      # every free state has two or three factors
        dev.close()


# ---- 4. undefined inputs; new parameters ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [8, 32])
def test_undefined_then_exact_then_new_parameters(hip_lib, d):
    model = cx.synth.lgssm_chain(7, d=d, seed=81 + d)
    dev = cx.DeviceGraph(dim=d, schedule=L.SCHED_TREE)
    cx.synth.load_into_device(model, dev)
    v, cnt = dev.log_evidence_mfma()                     # before any sweep
    assert math.isnan(v) and cnt["undefined"] > 0, (v, cnt)
    dev.sweep(1)
    first, _ = _exact(dev, E.dense_log_z(E.gmodel(model)), what="old (A, Q)")
    A, Q = model.psets[0]
    dev.set_factor_matrices(0, A, 2.0 * np.asarray(Q))
    dev.sweep(1)
    psets = dict(model.psets)
    psets[0] = (A, 2.0 * np.asarray(Q))
    second, _ = _exact(dev, E.dense_log_z(E.gmodel(model, psets=psets)), what="new (A, 2 Q)")      # the log-det table followed
    assert abs(second - first) > 1e-3
    dev.close()


# ---- 5. the embedded-dim rule ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [8, 20])
def test_embedded_dims_give_the_real_models_value_at_any_tile_size(hip_lib, d, monkeypatch):
    model = cx.synth.lgssm_chain(5, d=d, seed=90 + d)
    want = E.dense_log_z(E.gmodel(model))
    dev = swept_device(model, L.SCHED_TREE)
    native, _ = _exact(dev, want, what=f"d {d}, native tile")
    dev.close()
    monkeypatch.setenv("CX_MFMA_DIM", "64")
    dev = swept_device(model, L.SCHED_TREE)
    monkeypatch.delenv("CX_MFMA_DIM")
    forced, _ = _exact(dev, want, what=f"d {d}, 4 x 4 tiles")
    dev.close()
    assert abs(forced - native) <= 1e-12 * abs(native), (forced, native)


# ---- 6. moves nothing ------------------------------------------------------------------------------------------------------------
def test_moves_nothing(hip_lib):
    model = cx.synth.lgssm_chain(8, d=16, seed=72)
    for s in (L.SCHED_CHAIN_SCAN, L.SCHED_REFERENCE, L.SCHED_TREE):
        dev = swept_device(model, s)
        if s == L.SCHED_CHAIN_SCAN:      # (another reader first: every reader of the messages brings them to their slots)
            dev.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE)
        blob, marg = dev.export_state(), dev.get_marginals(model.x_ids)
        dev.log_evidence_mfma()          # the FIRST call: it builds the term lists
        assert np.array_equal(blob, dev.export_state())
        assert np.array_equal(marg, dev.get_marginals(model.x_ids))
        dev.log_evidence_mfma()
        assert np.array_equal(blob, dev.export_state())
        dev.close()
    # fused: the next sweeps are those of a twin handle that never called it, bit for bit
    a, b = swept_device(model, L.SCHED_FUSED, 5), swept_device(model, L.SCHED_FUSED, 5)
    assert a.residual() == b.residual()      # (the first call takes the snapshot the next one measures against)
    a.log_evidence_mfma()
    a.sweep(3); b.sweep(3)
    ra, rb = a.residual(), b.residual()
    assert math.isfinite(ra) and ra == rb, (ra, rb)
    assert np.array_equal(a.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE), b.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE),
                          equal_nan=True)      # (the messages into the observed variables are never computed)
    assert np.array_equal(a.get_marginals(model.x_ids), b.get_marginals(model.x_ids))
    a.close(); b.close()


# ---- 7. more terms than resident waves -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,d", [(2000, 64), (20000, 16)])
def test_long_chains_against_the_kalman_filter(hip_lib, T, d):
    model = cx.synth.lgssm_chain(T, d=d, seed=33)
    dev = swept_device(model, L.SCHED_CHAIN_SCAN)
    _, cnt = _exact(dev, E.kalman_of_chain(model), what=f"d = {d}, T = {T}, chain scan")
    assert cnt["factor_terms"] == 2 * T - 1 and cnt["variable_terms"] == T
    dev.close()


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(hip_lib):
    val, c4 = C.c_double(), (C.c_int64 * 4)()
    assert_reader_refusals("cx_log_evidence_mfma", "cx_log_evidence", lambda dev: dev.log_evidence_mfma(), lambda dev: dev.log_evidence(),
                           lambda dev: dev.lib.cx_log_evidence_mfma(dev.h, C.byref(val), c4))
    m16 = cx.synth.lgssm_chain(4, d=16, seed=92)
    dev = swept_device(m16, L.SCHED_FUSED, 2)
    assert dev.lib.cx_log_evidence_mfma(dev.h, None, None) == L.ERR_INVALID_ARGUMENT
    assert b"null argument" in dev.lib.cx_last_error(dev.h)
    code, msg = code_of(dev.halo_configure, [m16.x_ids[0]], [3 * 4 + 1], [], [])
    assert code == L.ERR_UNSUPPORTED and "dim == 1" in msg      # (no plain halo list exists at these dims)
    dev.close()


# ---- the C++ host class ---------------------------------------------------------------------------------------------------------
def test_cpp_host_class_log_evidence_mfma(hip_lib, tmp_path):
    rows = {line.split()[0]: line.split()[1:] for line in run_demo("evidence_mfma_demo", tmp_path)}
    T, d = 12, 16
    A, Q, R, y = demo_chain(T, d)
    want = E.kalman_log_lik(np.broadcast_to(A, (T - 1, d, d)), np.zeros((T - 1, d)), np.broadcast_to(Q, (T - 1, d, d)),
                            np.broadcast_to(R, (T, d, d)), y)
    assert math.isnan(float(rows["before"][0])) and int(rows["before"][3]) > 0
    got = float(rows["evidence"][0])
    assert abs(got - want) <= 1e-9 * abs(want), (got, want)
    assert rows["evidence"][1:] == [str(2 * T - 1), str(T), "0", "0"]
