"""What the tests/test_gpu_*.py files share: how a refusal is caught, how a handle is loaded and swept, how a tests/cpp demo is built and
run, the numpy form of the demos' model, and the refusals that every matrix-core reader owes to mfr::prepare (csrc/cx_mfma_reader.h).
A plain module: no fixtures, nothing collected.  tests/test_gpu_support_checker.py shows on the CPU that the two asserting helpers
(code_of, assert_reader_refusals) can fail."""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from tests import evidence_mfma_support as S
from tests import missing_data as MD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITER = (L.SCHED_FUSED, L.SCHED_FLOODING)      # the schedules that iterate: seeded messages, many sweeps


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def code_of(fn, *a, **k):
    """(code, message) of the CortexHipError that fn(*a, **k) raises; a call that does not raise fails the test"""
    with pytest.raises(L.CortexHipError) as e:
        fn(*a, **k)
    return e.value.code, e.value.message


def under_capture(dev, call):
    """the status of `call` while the handle's stream is being captured (relaxed mode: the refusal's own runtime queries do not void
    the capture); the handle is back on its own stream afterwards"""
    hip = C.CDLL([ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln][0])
    stream, graph = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    dev.set_stream(stream.value)
    assert hip.hipStreamBeginCapture(stream, 2) == 0
    rc = call()
    assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0
    if graph.value:
        hip.hipGraphDestroy(graph)
    dev.set_stream(None)
    assert hip.hipStreamDestroy(stream) == 0
    return rc, dev.lib.cx_last_error(dev.h).decode()


# ---- loaders ---------------------------------------------------------------------------------------------------------------------------
def swept_device(model, schedule, fused_sweeps=60):
    """the matrix-core readers' handle: seed variance 1e6 and fused_sweeps sweeps under SCHED_FUSED, one sweep otherwise"""
    dev = cx.DeviceGraph(dim=model.dim, schedule=schedule)
    cx.synth.load_into_device(model, dev, seed_variance=1e6 if schedule == L.SCHED_FUSED else None)
    dev.sweep(fused_sweeps if schedule == L.SCHED_FUSED else 1)      # (reference order: cx_sweep requests every variable)
    return dev


def iterative_device(model, schedule, iterative_sweeps=0):
    """the dim 1 .. 4 readers' handle: seed variance 1e6 and iterative_sweeps sweeps under a schedule of ITER, one sweep otherwise"""
    dev = cx.DeviceGraph(dim=model.dim, schedule=schedule)
    cx.synth.load_into_device(model, dev, seed_variance=1e6 if schedule in ITER else None)
    dev.sweep(iterative_sweeps if schedule in ITER else 1)      # (reference order: cx_sweep requests every variable)
    return dev


def missing_data_device(model):
    dev = cx.DeviceGraph(dim=model.dim, schedule=L.SCHED_TREE)
    MD.load(model, dev)                    # the flat message on the one edge of every latent leaf
    dev.sweep(1)
    return dev


def loaded_device(model, opaque=None, how="sweep", schedule=L.SCHED_TREE):
    """one sweep on a model of tests/sample_mfma_support.models(): how = "sweep", "flat" (missing data) or "opaque" (set_opaque(opaque))"""
    dev = cx.DeviceGraph(dim=model.dim, schedule=schedule)
    if how == "flat":
        MD.load(model, dev)                    # the flat message on the one edge of every latent leaf
    else:
        cx.synth.load_into_device(model, dev)
    if how == "opaque":
        S.set_opaque(dev, opaque)
    dev.sweep(1)
    return dev


def with_sets(model, psets):
    """the model with the (A, Q) of set 0 and the R of set 1 in its meta, where the Kalman references read them"""
    A, Q = psets[0]
    _, R = psets[1]
    return dataclasses.replace(model, meta={**model.meta, "A": np.asarray(A), "Q": np.asarray(Q), "R": np.asarray(R)})


# ---- the C++ demos of tests/cpp ----------------------------------------------------------------------------------------------------------
def build_demo(name, tmp_path):
    """tests/cpp/<name>.cpp built against the C ABI alone, warnings as errors; returns the program's path"""
    exe = str(tmp_path / name)
    libdir = os.path.join(ROOT, "cortex.jl_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe,
                           "-L" + libdir, "-lcortex_hip", "-Wl,-rpath," + libdir])
    return exe


def run_demo(name, tmp_path, timeout=120):
    """builds and runs tests/cpp/<name>.cpp; the lines it printed"""
    out = subprocess.run([build_demo(name, tmp_path)], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr
    return out.stdout.splitlines()


def demo_chain(T=12, d=16):
    """(A, Q, R, y) of the model of tests/cpp/demo_chain.hpp: A = 0.9 I plus 0.05 on the cyclic super-diagonal, Q = I / 2, H = R = I,
    y_t[k] = 0.25 t + ((3 t + k) % 7) - 3 for t = 1 .. T"""
    A = np.array([[0.9 if i == j else (0.05 if j == (i + 1) % d else 0.0) for j in range(d)] for i in range(d)])
    y = np.array([[0.25 * t + ((3 * t + k) % 7) - 3.0 for k in range(d)] for t in range(1, T + 1)], dtype=np.float64)
    return A, 0.5 * np.eye(d), np.eye(d), y


def demo_chain_model(T=12, d=16):
    """that model as a synth model: the demo's ids are lgssm_chain's; its connections in the demo's order"""
    A, Q, R, y = demo_chain(T, d)
    base = cx.synth.lgssm_chain(T, d=d, seed=1)
    x, yv, lik, tr = base.x_ids, base.x_ids + T, base.x_ids + 2 * T, np.arange(3 * T + 1, 4 * T)
    ev = np.concatenate([np.stack([yv, x], 1).ravel(), np.stack([x[:-1], x[1:]], 1).ravel()])
    ef = np.concatenate([np.repeat(lik, 2), np.repeat(tr, 2)])
    er = np.concatenate([np.tile([L.ROLE_OUT, L.ROLE_IN], T), np.tile([L.ROLE_IN, L.ROLE_OUT], T - 1)]).astype(np.int32)
    return dataclasses.replace(base, edge_var=ev, edge_fac=ef, edge_role=er, data_y=y, psets={0: (A, Q), 1: (np.eye(d), R)},
                               meta={**base.meta, "A": A, "Q": Q, "R": R})


# ---- the refusals of mfr::prepare, stated once ---------------------------------------------------------------------------------------------
REFUSAL_T, REFUSAL_D = 4, 16      # the dim 16 chain of the cases below: 8 variables, factors 9 .. 15 (a raw call sizes its outputs for it)
HANDLE_CASES = ("small dim", "natural2", "structured vmp", "no graph", "small call", "state halo", "time block")
STREAM_CASES = ("captured", "never set")      # (a file with two refusal tests makes these in the second)
REFUSAL_CASES = HANDLE_CASES + STREAM_CASES


def refusal_device(case):
    """the handle of one case of assert_reader_refusals"""
    T = REFUSAL_T
    m16 = cx.synth.lgssm_chain(T, d=REFUSAL_D, seed=92)
    if case == "small dim":
        return swept_device(cx.synth.lgssm_chain(5, d=4, seed=91), L.SCHED_TREE)
    if case == "natural2":
        return cx.DeviceGraph(family=L.FAMILY_NATURAL2)
    if case == "structured vmp":
        dev = cx.DeviceGraph(schedule=L.SCHED_CHAIN_SCAN, family=L.FAMILY_VMP_STRUCTURED)
        cx.synth.load_vmp_into_device(cx.synth.vmp_ssm(8), dev)
        return dev
    if case == "no graph":
        return cx.DeviceGraph(dim=REFUSAL_D)
    if case == "state halo":
        dev = swept_device(m16, L.SCHED_FUSED, 2)
        dev.halo_configure_state([m16.x_ids[0]], [3 * T + 1], [], [])      # a halo list (x_1, the first transition): a partitioned handle
        return dev
    if case == "never set":
        # Rule tables not on the device: behind a graph they are missing only while a parameter set that a factor names was never set,
        # and that is refused first, under the call's own name (the guard behind it cannot be reached through the API)
        dev = cx.DeviceGraph(dim=REFUSAL_D, schedule=L.SCHED_TREE)
        dev.set_factor_matrices(0, *m16.psets[0])                # set 1, the likelihoods', is never set
        dev.graph_create(m16.edge_var, m16.edge_fac, m16.factor_ids, m16.factor_kind, m16.factor_var, edge_role=m16.edge_role)
        return dev
    return swept_device(m16, {"small call": L.SCHED_FUSED, "time block": L.SCHED_CHAIN_SCAN, "captured": L.SCHED_TREE}[case], 2)


class ReaderRig:
    """where assert_reader_refusals gets its handles and its capture: the device.  (tests/test_gpu_support_checker.py puts stubs here)"""
    device = staticmethod(refusal_device)
    under_capture = staticmethod(under_capture)


def assert_reader_refusals(who, small, call, small_call, raw, cases=REFUSAL_CASES, skip=(), rig=ReaderRig):
    """Every refusal that a matrix-core reader owes to mfr::prepare, each under the reader's own name.  who: the reader's C name; small:
    the C name of its dim 1 .. 4 counterpart; call(dev): the reader through DeviceGraph with its cheapest valid arguments (variable 1
    and factor 3 T + 1 = 13 exist in every model here); small_call(dev): the dim 1 .. 4 method, which keeps refusing dim 16; raw(dev):
    the reader through ctypes, its status returned, for the captured stream (outputs sized for the chain REFUSAL_T, REFUSAL_D).
    cases: HANDLE_CASES or STREAM_CASES where a file spreads them over its two refusal tests.  skip: the cases that the reader cannot
    meet — the caller's comment says why."""
    assert set(skip) <= set(REFUSAL_CASES) and set(cases) <= set(REFUSAL_CASES), (cases, skip)
    skip = tuple(skip) + tuple(c for c in REFUSAL_CASES if c not in cases)

    def refused(case, code, *words, before=None):
        if case in skip:
            return
        dev = rig.device(case)
        if before is not None:
            before(dev)
        got, msg = code_of(call, dev)
        assert got == code and msg.startswith(who + ":"), (case, got, msg)
        for w in words:
            assert w in msg, (case, w, msg)
        dev.close()
        return msg

    msg = refused("small dim", L.ERR_UNSUPPORTED, "5 .. 64")
    assert msg is None or small in msg.replace(who, ""), msg                    # names the call for dims 1 .. 4
    refused("natural2", L.ERR_UNSUPPORTED, "Gaussian family")
    refused("structured vmp", L.ERR_UNSUPPORTED, "Gaussian family")
    refused("no graph", L.ERR_STATE, "no graph")
    if "small call" not in skip:
        dev = rig.device("small call")
        assert code_of(small_call, dev)[0] == L.ERR_UNSUPPORTED                   # the old call keeps refusing these dims
        dev.close()
    refused("state halo", L.ERR_UNSUPPORTED, "partitioned handle")

    def becomes_a_time_block(dev):
        # a halo list through cx_halo_configure: at these dims it is accepted under the chain scan alone, where it makes the handle a
        # chain's time block (a plain per-sweep message halo is refused by cx_halo_configure itself at dim > 1)
        call(dev)                                                                 # (a handle whose plans the reader has already built)
        dev.halo_configure([1], [3 * REFUSAL_T + 1], [], [])

    refused("time block", L.ERR_UNSUPPORTED, "partitioned handle", "time block", before=becomes_a_time_block)
    if "captured" not in skip:
        dev = rig.device("captured")
        rc, msg = rig.under_capture(dev, lambda: raw(dev))
        assert rc == L.ERR_STATE and msg.startswith(who + ":") and "captured" in msg, (rc, msg)
        dev.close()
    refused("never set", L.ERR_STATE, "never set", "cx_set_factor_matrices")
