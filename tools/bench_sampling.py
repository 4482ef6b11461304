"""tools/bench_sampling.py — cost of one cx_sample_posterior call next to cx_log_evidence on the same handle: a C3-size
d = 4 chain (S = 8) and a C2-size scalar chain (S = 64) after one chain-scan sweep, a 200 k deep tree_model (S = 64) after one tree
sweep.  Median wall time of >= 20 synchronised calls after a warm-up call (the first call builds the plan), and apart from it the
device-to-host copy of an output of the same size (hipMemcpy into pageable host memory, as the call copies into the caller's
array).  The per-kernel device time comes from a separate run under rocprofv3 --kernel-trace --stats.  Prints one JSON line
per config.  Not the driver's bench."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import cortex.jl_amd as cx                      # noqa: E402
from cortex.jl_amd import _lib as L            # noqa: E402


def median_ms(fn, dev, calls: int) -> float:
    fn()                                        # warm-up: builds the plan
    ts = []
    for _ in range(calls):
        dev.sync()
        t = time.perf_counter()
        fn()                                    # synchronous: the samples are on the host at return
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e3


def copy_ms(n_doubles: int, calls: int) -> float:
    import ctypes as C

    hip = C.CDLL("libamdhip64.so")
    buf = C.c_void_p()
    assert hip.hipMalloc(C.byref(buf), C.c_size_t(n_doubles * 8)) == 0
    host = np.empty(n_doubles, np.float64)
    ts = []
    for _ in range(calls + 1):
        t = time.perf_counter()
        assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), buf, C.c_size_t(n_doubles * 8), 2) == 0      # hipMemcpyDeviceToHost
        ts.append(time.perf_counter() - t)
    hip.hipFree(buf)
    return float(np.median(ts[1:])) * 1e3


def run(name, model, schedule, S, calls, workload):
    dev = cx.DeviceGraph(dim=model.dim, schedule=schedule)
    cx.synth.load_into_device(model, dev)
    dev.sweep(1)
    dev.sync()
    d = model.dim
    ids = model.x_ids
    ms_ev = median_ms(dev.log_evidence, dev, calls)
    ms_s = median_ms(lambda: dev.sample_posterior(S, seed=1, variable_ids=ids), dev, calls)
    _, counts = dev.sample_posterior(S, seed=1, variable_ids=ids)
    out_doubles = S * len(ids) * d
    ms_copy = copy_ms(out_doubles, calls)
    out = {"config": name, "workload": workload, "samples": S, "calls": calls, "ms_log_evidence": ms_ev, "ms_sample_posterior": ms_s,
           "ms_d2h_copy_of_output": ms_copy, "ms_sample_posterior_minus_copy": ms_s - ms_copy, "output_MB": out_doubles * 8 / 1e6,
           "counts": counts}
    dev.close()
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--only", default="", help="comma-separated subset of C3,C2,tree")
    a = ap.parse_args()
    only = set(a.only.split(",")) if a.only else {"C3", "C2", "tree"}
    if "C3" in only:
        m = cx.synth.lgssm_chain(1_000_000, d=4)
        run("C3", m, L.SCHED_CHAIN_SCAN, 8, a.calls, "d=4 chain T=1000000 after one chain-scan sweep, S=8, the states")
    if "C2" in only:
        m = cx.synth.ssm_chain(250_001, seed=1234)
        run("C2", m, L.SCHED_CHAIN_SCAN, 64, a.calls, "scalar chain T=250001 after one chain-scan sweep, S=64, the states")
    if "tree" in only:
        m = cx.synth.tree_model(200_000, shape="deep", observe=0.2)
        run("tree", m, L.SCHED_TREE, 64, a.calls, "tree_model(200000, deep, observe=0.2) after one tree sweep, S=64, the latent variables")


if __name__ == "__main__":
    main()
