"""-m gpu: cx_predictive_mfma — the predictive scores of the data at the matrix-core dims (cx_create dim 5 .. 64) —
against the dense leave-one-out solve, the Kalman innovations and the numpy restatement of cx_predictive's formula on the device's own
messages (tests/predictive_support.py; the models are those of tests/predictive_mfma_support.py, pinned on the CPU by
tests/test_predictive_mfma_checker.py).  Rows are held to predictive_support.assert_rows_close(..., 1e-9), totals to 1e-9 relative."""
import ctypes as C
import math

import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from tests import evidence_mfma_support as S
from tests import evidence_support as E
from tests import predictive_mfma_support as PM
from tests import predictive_support as P
from tests.gpu_support import (HANDLE_CASES, STREAM_CASES, assert_reader_refusals, code_of, demo_chain, missing_data_device, run_demo,
                               swept_device, under_capture, with_sets)

pytestmark = pytest.mark.gpu
TOL = 1e-9


def _close(got, want, what):
    errs = P.assert_rows_close(got, want, TOL, what)
    print(what, errs)
    return errs


def _on_device_messages(gm, dev, mode):
    f2v, opq = E.device_messages(gm, dev)
    return P.predictive_from_messages(gm, f2v, opq, mode=mode)


def _rel(a, b):
    return abs(a - b) / abs(b)


def _counts(n, improper=0, undefined=0):
    return {"rows": n, "scored": n - improper - undefined, "undefined": undefined, "improper": improper}


# ---- 1. rows after every schedule -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["chain", "comb"])
@pytest.mark.parametrize("d", PM.SCHEDULE_DIMS)
def test_rows_after_every_schedule(hip_lib, d, shape):
    model = PM.chain(d) if shape == "chain" else PM.comb(d)
    gm = E.gmodel(model)
    dense = P.dense_loo_all(gm)
    inno = PM.innovations_rows(model) if shape == "chain" else None
    n = len(dense["factor_ids"])
    for s in [L.SCHED_TREE, L.SCHED_REFERENCE, L.SCHED_FUSED] + ([L.SCHED_CHAIN_SCAN] if shape == "chain" else []):
        what = f"d {d} {shape} schedule {s}"
        dev = swept_device(model, s)      # (fused: seed variance 1e6 and 60 sweeps, the diameter is under 20)
        assert np.array_equal(dev.predictive_rows_mfma(), dense["factor_ids"])
        loo, cau = dev.predictive_mfma("loo"), dev.predictive_mfma("causal")
        _close(loo, dense, what + " loo vs dense")
        assert loo["counts"] == _counts(n), (what, loo["counts"])
        _close(cau, _on_device_messages(gm, dev, P.CAUSAL), what + " causal vs the formula on the device's messages")
        assert cau["counts"] == _counts(n, improper=1) and math.isnan(cau["log_density"][0]), (what, cau["counts"])      # the first row: nothing is kept
        if inno is not None:
            _close(cau, inno, what + " causal vs the Kalman innovations")
            z, _ = dev.log_evidence_mfma()      # (H = I at these seeds: the improper first row's share, -log|det H|, is 0)
            print(what, "causal total", repr(cau["total"]), "log evidence", repr(z), "rel", _rel(cau["total"], z))
            assert _rel(cau["total"], z) <= TOL, (what, cau["total"], z)
        dev.close()


# ---- 2. general matrices, gaps and a forecast tail -----------------------------------------------------------------------------------
@pytest.mark.parametrize("d", PM.GEN_DIMS)
def test_general_matrices_gaps_and_a_forecast_tail(hip_lib, d):
    model = PM.gen(d)
    gm = E.gmodel(model)
    want, log_first = PM.kalman_rows(model)
    dev = missing_data_device(model)
    cau, loo = dev.predictive_mfma("causal"), dev.predictive_mfma("loo")
    assert np.array_equal(cau["factor_ids"], np.sort(model.data_fac)) and np.array_equal(loo["factor_ids"], cau["factor_ids"])      # the observed steps
    _close(cau, want, f"gen d {d} causal vs kalman_missing")
    _close(loo, P.dense_loo_all(gm), f"gen d {d} loo vs dense")
    n = len(cau["factor_ids"])
    assert cau["counts"] == _counts(n, improper=1) and loo["counts"] == _counts(n), (cau["counts"], loo["counts"])
    z, _ = dev.log_evidence_mfma()
    print("gen d", d, "causal total + log_first", repr(cau["total"] + log_first), "log evidence", repr(z), "rel", _rel(cau["total"] + log_first, z))
    assert _rel(cau["total"] + log_first, z) <= TOL
    dev.close()


# ---- 3. a leading gap: the flat-pivot rule ----------------------------------------------------------------------------------------------
def _pivots(A):
    """the pivots of an unpivoted symmetric elimination of A, up to and including the first that is not positive"""
    A = np.array(A, float)
    out = []
    for k in range(len(A)):
        p = A[k, k]
        out.append(p)
        if not p > 0.0:
            break
        A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k, k + 1:]) / p
    return np.array(out)


@pytest.mark.parametrize("d", PM.GEN_DIMS)
def test_a_leading_gap_is_improper_by_the_flat_pivot_rule(hip_lib, d):
    model = PM.leading_gap(d)
    gm = E.gmodel(model)
    dev = missing_data_device(model)
    cau, loo = dev.predictive_mfma("causal"), dev.predictive_mfma("loo")
    # the measurement the rule's constant rests on: row 0's causal cavity is the one message of the first transition into x_2, whose
    # information is flat — its pivots against the diagonal of the sum of all messages into x_2, from the device's own messages
    f2v, _ = E.device_messages(gm, dev)
    _fid, k, fi, _o = P.rows_of(gm)[0]
    g = gm.groups[k]
    x = int(g["vars"][fi, 1])
    lam = f2v[k][1]
    into = [(f, j) for f in range(len(g["fid"])) for j in range(k) if int(g["vars"][f, j]) == x]
    kept = [(f, j) for (f, j) in into if j == 0]
    assert len(kept) == 1 and len(into) == 3
    ref = np.diag(sum(lam[f, j] for (f, j) in into))
    piv = _pivots(lam[kept[0]])
    ratio = piv / ref[:len(piv)]
    print(f"leading gap d {d}: pivot / ref of the flat cavity", ratio.tolist(), "largest |.|", float(np.abs(ratio).max()),
          "rule 64 d eps", 64 * d * np.finfo(float).eps)
    assert cau["counts"] == _counts(4, improper=1) and PM.status_of(cau).tolist() == [2, 0, 0, 0], cau["counts"]
    _close(cau, _on_device_messages(gm, dev, P.CAUSAL), f"leading gap d {d} causal vs the formula on the device's messages")
    assert loo["counts"] == _counts(4), loo["counts"]
    _close(loo, P.dense_loo_all(gm), f"leading gap d {d} loo vs dense")
    dev.close()


# ---- 4. a proper opaque prior ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", PM.PRIOR_DIMS)
def test_a_proper_opaque_prior_scores_every_row(hip_lib, d):
    model, opq = S.prior_chain(d)
    gm = E.gmodel(model, opaque=opq)
    z, dense = E.dense_log_z(gm), P.dense_loo_all(gm)
    n = len(dense["factor_ids"])
    for s in (L.SCHED_TREE, L.SCHED_FUSED):
        dev = cx.DeviceGraph(dim=d, schedule=s)
        cx.synth.load_into_device(model, dev, seed_variance=1e6 if s == L.SCHED_FUSED else None)
        S.set_opaque(dev, opq)
        dev.sweep(60 if s == L.SCHED_FUSED else 1)
        cau, loo = dev.predictive_mfma("causal"), dev.predictive_mfma("loo")
        assert cau["counts"] == _counts(n) and loo["counts"] == _counts(n), (cau["counts"], loo["counts"])
        print("prior d", d, "schedule", s, "causal total", repr(cau["total"]), "dense log z", repr(z), "rel", _rel(cau["total"], z))
        assert _rel(cau["total"], z) <= TOL
        _close(loo, dense, f"prior d {d} schedule {s} loo vs dense")
        dev.close()


# ---- 5. a clamped state in the middle --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", PM.CLAMPED_DIMS)
def test_a_clamped_state_in_the_middle(hip_lib, d):
    model = S.clamped_middle(d)
    gm = E.gmodel(model)
    x = model.x_ids[model.meta["clamped_state"]]
    ev, ef, er = np.asarray(model.edge_var), np.asarray(model.edge_fac), np.asarray(model.edge_role)
    into = int(ef[(ev == x) & (er == L.ROLE_OUT)][0])                          # the transition into x: x is its OUT end
    lik = int(np.asarray(model.data_fac)[model.meta["clamped_state"]])         # x's likelihood: both ends observed
    dev = swept_device(model, L.SCHED_TREE)
    rows = dev.predictive_rows_mfma()
    assert len(rows) == 5 and into in rows.tolist() and lik not in rows.tolist()
    with pytest.raises(L.CortexHipError) as e:
        dev.predictive_mfma("loo", factor_ids=[lik])
    assert e.value.code == L.ERR_UNSUPPORTED and f"factor {lik}" in e.value.message and "not a row" in e.value.message
    cau, loo = dev.predictive_mfma("causal"), dev.predictive_mfma("loo")
    _close(loo, P.dense_loo_all(gm), f"clamped middle d {d} loo vs dense")
    assert PM.status_of(cau).tolist() == [2, 0, 0, 0, 0] and cau["counts"] == _counts(5, improper=1), cau["counts"]
    _close(cau, _on_device_messages(gm, dev, P.CAUSAL), f"clamped middle d {d} causal vs the formula on the device's messages")
    dev.close()


# ---- 6. a loop -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", S.RING_DIMS)
def test_a_loop_matches_the_formula_on_the_device_messages(hip_lib, d):
    model = S.ring(d)
    gm = E.gmodel(model)
    dev = swept_device(model, L.SCHED_FUSED, S.RING_SWEEPS)
    for name, mode in (("loo", P.LOO), ("causal", P.CAUSAL)):
        got, again = dev.predictive_mfma(name), dev.predictive_mfma(name)
        _close(got, _on_device_messages(gm, dev, mode), f"ring d {d} {name}")
        assert got["counts"]["undefined"] == 0 and got["counts"]["scored"] > 0
        for key in ("mean", "cov", "log_density", "mahalanobis"):
            assert got[key].tobytes() == again[key].tobytes(), (name, key)      # two calls on one state: bit-identical
        assert np.float64(got["total"]).tobytes() == np.float64(again["total"]).tobytes()
    dev.close()


# ---- 7. embedded dims ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [8, 20])
def test_embedded_dims_give_the_real_models_rows_at_any_tile_size(hip_lib, d, monkeypatch):
    model = cx.synth.lgssm_chain(5, d=d, seed=90 + d)
    dev = swept_device(model, L.SCHED_TREE)
    native = {m: dev.predictive_mfma(m) for m in ("loo", "causal")}
    dev.close()
    monkeypatch.setenv("CX_MFMA_DIM", "64")
    dev = swept_device(model, L.SCHED_TREE)
    monkeypatch.delenv("CX_MFMA_DIM")
    for m in ("loo", "causal"):
        forced = dev.predictive_mfma(m)
        errs = P.assert_rows_close(forced, native[m], 1e-12, f"d {d} {m}: 4 x 4 tiles against the native tile")
        print("embedded d", d, m, errs)
        assert forced["counts"] == native[m]["counts"] and _rel(forced["total"], native[m]["total"]) <= 1e-12
    assert math.isnan(native["causal"]["log_density"][0]) and native["causal"]["counts"]["improper"] == 1
    dev.close()


# ---- 8. undefined inputs; new parameters -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [8, 32])
def test_undefined_then_exact_then_new_parameters(hip_lib, d):
    model = cx.synth.lgssm_chain(7, d=d, seed=81 + d)
    dev = cx.DeviceGraph(dim=d, schedule=L.SCHED_TREE)
    cx.synth.load_into_device(model, dev)
    for m in ("loo", "causal"):                      # before any sweep
        r = dev.predictive_mfma(m)
        assert r["counts"] == _counts(7, undefined=7) and r["total"] == 0.0, (m, r["counts"], r["total"])
        assert all(np.isnan(r[k]).all() for k in ("mean", "cov", "log_density", "mahalanobis"))
    psets = dict(model.psets)
    first = None
    for step in ("old (A, Q)", "new (A, 2 Q)", "new (H, 2 R)"):
        if step == "new (A, 2 Q)":
            psets[0] = (psets[0][0], 2.0 * np.asarray(psets[0][1]))
            dev.set_factor_matrices(0, *psets[0])
        if step == "new (H, 2 R)":
            psets[1] = (psets[1][0], 2.0 * np.asarray(psets[1][1]))
            dev.set_factor_matrices(1, *psets[1])
        dev.sweep(1)
        cau, loo = dev.predictive_mfma("causal"), dev.predictive_mfma("loo")
        _close(cau, PM.innovations_rows(with_sets(model, psets)), f"d {d} {step} causal vs the Kalman innovations")      # the [A' | Q] table followed
        _close(loo, P.dense_loo_all(E.gmodel(model, psets=psets)), f"d {d} {step} loo vs dense")
        if first is None:
            first = cau
        elif step == "new (A, 2 Q)":
            assert np.abs(cau["cov"][1] - first["cov"][1]).max() > 1e-3
        else:      # S_t = H P_t H' + R: doubling R moves the second row's S by R and by what the first state's filtered covariance gained
            assert np.abs(cau["cov"][1] - second["cov"][1]).max() > 1e-3
        second = cau
    dev.close()


# ---- 9. named rows -----------------------------------------------------------------------------------------------------------------------
def test_named_rows_in_the_callers_order(hip_lib):
    model = cx.synth.lgssm_chain(9, d=16, seed=83)
    dev = swept_device(model, L.SCHED_TREE)
    for m in ("loo", "causal"):
        full = dev.predictive_mfma(m)
        ids = full["factor_ids"]
        for pick in ([7, 2, 5, 0], [1, 8]):       # (the second list: another request, the plan is rebuilt)
            sub = dev.predictive_mfma(m, factor_ids=ids[pick])
            assert np.array_equal(sub["factor_ids"], ids[pick]) and sub["counts"]["rows"] == len(pick)
            for key in ("mean", "cov", "log_density", "mahalanobis"):
                assert sub[key].tobytes() == full[key][pick].tobytes(), (m, pick, key)
            lean = dev.predictive_mfma(m, factor_ids=ids[pick], rows=False)
            assert lean["mean"] is None and lean["cov"] is None and lean["log_density"] is None and lean["mahalanobis"] is None
            assert np.float64(lean["total"]).tobytes() == np.float64(sub["total"]).tobytes() and lean["counts"] == sub["counts"]
        lean = dev.predictive_mfma(m, rows=False)
        assert lean["mean"] is None and np.float64(lean["total"]).tobytes() == np.float64(full["total"]).tobytes() and lean["counts"] == full["counts"]
    with pytest.raises(L.CortexHipError) as e:
        dev.predictive_mfma("loo", factor_ids=[10 ** 9])
    assert e.value.code == L.ERR_NOT_FOUND
    dev.close()


# ---- 10. more rows than resident waves and than one payload chunk -------------------------------------------------------------------------
@pytest.mark.parametrize("T,d", [(2500, 64), (20000, 16)])
def test_long_chains_against_the_kalman_innovations(hip_lib, T, d):
    model = cx.synth.lgssm_chain(T, d=d, seed=33)
    assert T * (d + d * d + 2) * 8 > 32 << 20      # more than one chunk of the payload
    dev = swept_device(model, L.SCHED_CHAIN_SCAN)
    cau = dev.predictive_mfma("causal")
    _close(cau, PM.innovations_rows(model), f"d = {d}, T = {T}, chain scan, causal vs the Kalman innovations")
    assert cau["counts"] == _counts(T, improper=1), cau["counts"]
    z, _ = dev.log_evidence_mfma()
    print("long chain d", d, "causal total", repr(cau["total"]), "log evidence", repr(z), "rel", _rel(cau["total"], z))
    assert _rel(cau["total"], z) <= TOL
    lean = dev.predictive_mfma("causal", rows=False)
    assert np.float64(lean["total"]).tobytes() == np.float64(cau["total"]).tobytes() and lean["counts"] == cau["counts"]
    dev.close()


# ---- 11. moves nothing -------------------------------------------------------------------------------------------------------------------
def test_moves_nothing(hip_lib):
    model = cx.synth.lgssm_chain(8, d=16, seed=72)
    for s in (L.SCHED_CHAIN_SCAN, L.SCHED_REFERENCE, L.SCHED_TREE):
        dev = swept_device(model, s)
        if s == L.SCHED_CHAIN_SCAN:      # (another reader first: every reader of the messages brings them to their slots)
            dev.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE)
        blob, marg = dev.export_state(), dev.get_marginals(model.x_ids)
        dev.predictive_mfma("causal")      # the FIRST call: it builds the rows
        assert np.array_equal(blob, dev.export_state())
        assert np.array_equal(marg, dev.get_marginals(model.x_ids))
        dev.predictive_mfma("loo", rows=False)
        assert np.array_equal(blob, dev.export_state())
        dev.close()
    # fused: the next sweeps are those of a twin handle that never called it, bit for bit
    a, b = swept_device(model, L.SCHED_FUSED, 5), swept_device(model, L.SCHED_FUSED, 5)
    assert a.residual() == b.residual()      # (the first call takes the snapshot the next one measures against)
    a.predictive_mfma("causal"); a.predictive_mfma("loo")
    a.sweep(3); b.sweep(3)
    ra, rb = a.residual(), b.residual()
    assert math.isfinite(ra) and ra == rb, (ra, rb)
    assert np.array_equal(a.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE), b.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE),
                          equal_nan=True)      # (the messages into the observed variables are never computed)
    assert np.array_equal(a.get_marginals(model.x_ids), b.get_marginals(model.x_ids))
    a.close(); b.close()


# ---- 12. refusals ------------------------------------------------------------------------------------------------------------------------
WHO = "cx_predictive_mfma"


def _raw_causal(dev, out):
    """every causal row through the C ABI, into out [rows, d + d d + 2]; the status"""
    return dev.lib.cx_predictive_mfma(dev.h, L.PREDICT_CAUSAL, 0, None, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(C.c_double()), (C.c_int64 * 4)())


# what assert_reader_refusals asks of this reader (rows=False: the call itself; with rows the row list, cx_predictive_rows_mfma, is asked
# first; raw: its dim 16 chain has 4 rows)
_COMMON = dict(who=WHO, small="cx_predictive", call=lambda dev: dev.predictive_mfma(rows=False), small_call=lambda dev: dev.predictive(),
               raw=lambda dev: _raw_causal(dev, np.zeros((4, 16 + 256 + 2))))


def test_refusals(hip_lib):
    who = WHO
    assert_reader_refusals(**_COMMON, cases=HANDLE_CASES)
    m4 = cx.synth.lgssm_chain(5, d=4, seed=91)
    m16 = cx.synth.lgssm_chain(4, d=16, seed=92)
    dev = swept_device(m4, L.SCHED_TREE)
    code, msg = code_of(dev.predictive_rows_mfma)
    assert code == L.ERR_UNSUPPORTED and msg.startswith("cx_predictive_rows_mfma")      # the row list refuses under its own name
    dev.close()
    dev = swept_device(m16, L.SCHED_FUSED, 2)
    assert code_of(dev.predictive_rows)[0] == L.ERR_UNSUPPORTED      # the old row list keeps refusing these dims too
    tot, c4 = C.c_double(), (C.c_int64 * 4)()
    ids = (C.c_int64 * 1)(int(m16.data_fac[0]))
    for args, text in (((7, 0, None, None, C.byref(tot), c4), "mode is"), ((L.PREDICT_LOO, 0, None, None, C.byref(tot), None), "counts4 is null"),
                       ((L.PREDICT_LOO, -1, ids, None, C.byref(tot), c4), "negative count")):
        assert dev.lib.cx_predictive_mfma(dev.h, *args) == L.ERR_INVALID_ARGUMENT
        assert dev.lib.cx_last_error(dev.h).decode().startswith(who) and text in dev.lib.cx_last_error(dev.h).decode()
    dev.close()


def test_refusals_of_a_captured_stream_and_of_parameter_sets_never_set(hip_lib):
    assert_reader_refusals(**_COMMON, cases=STREAM_CASES)
    d = 16
    model = cx.synth.lgssm_chain(5, d=d, seed=93)
    dev = swept_device(model, L.SCHED_TREE)
    want = dev.predictive_mfma("causal")
    out = np.zeros((5, d + d * d + 2))
    rc, msg = under_capture(dev, lambda: _raw_causal(dev, out))
    assert rc == L.ERR_STATE and msg.startswith("cx_predictive_mfma") and "captured" in msg, (rc, msg)
    assert not out.any()                                       # nothing was written
    got = dev.predictive_mfma("causal")                        # and the handle works on, bit for bit
    assert all(got[k].tobytes() == want[k].tobytes() for k in ("mean", "cov", "log_density", "mahalanobis")) and got["total"] == want["total"]
    dev.close()


# ---- 13. the C++ host class --------------------------------------------------------------------------------------------------------------
def test_cpp_host_class_predictive_mfma(hip_lib, tmp_path):
    lines = [line.split() for line in run_demo("predictive_mfma_demo", tmp_path)]
    head = {ln[0]: ln[1:] for ln in lines if ln[0] != "row"}
    rows = [ln[1:] for ln in lines if ln[0] == "row"]
    T, d = 12, 16
    A, Q, R, y = demo_chain(T, d)
    yh, Sm, term, maha = P.kalman_innovations(np.broadcast_to(A, (T - 1, d, d)), np.zeros((T - 1, d)), np.broadcast_to(Q, (T - 1, d, d)),
                                              np.broadcast_to(R, (T, d, d)), y)
    assert float(head["before"][0]) == 0.0 and head["before"][1:] == [str(T), "0", str(T), "0"]
    want_total = float(np.sum(term[1:]))
    assert abs(float(head["causal"][0]) - want_total) <= TOL * abs(want_total) and head["causal"][1:] == [str(T), str(T - 1), "0", "1"]
    assert float(head["total_only"][0]) == float(head["causal"][0]) and head["total_only"][1] == "0"
    assert [int(r[0]) for r in rows] == [2 * T + 1 + t for t in range(T)]
    assert all(math.isnan(float(v)) for v in rows[0][1:])
    for t in range(1, T):
        got = [float(v) for v in rows[t][1:]]
        want = [term[t], maha[t], yh[t][0], Sm[t][0, 0], Sm[t][1, 0]]
        assert all(abs(g - w) <= TOL * max(abs(w), 1.0) for g, w in zip(got, want)), (t, got, want)
