"""tools/bench_causal_mfma.py — cost of one cx_causal_marginals_mfma call on T = 1e5 chains at d = 16, 32 and 64 (config
C5) after one chain-scan sweep, for the states only (variable_ids = x_ids): predicted, filtered, and filtered with lag 1 and lag 8; and
beside them, in the same process on the same handle, one cx_predictive_mfma(CX_PREDICT_CAUSAL) call with rows (the same arithmetic plus
one factorisation, a payload of nearly the same size); then one fused sweep of the same model (a lag pass is one rule per transition:
about half a sweep's rules on a chain).  Median wall time of `calls` synchronised calls after a warm-up call (the first call of a
request builds its rows, the first with a lag allocates β).  The calls go to the C entry points with one host array made beforehand, so
that the time is the library's (kernels, chunks and device-to-host copies), not numpy's; the fused sweep: the median of 10 synchronised
single sweeps after 3.  Prints one JSON line per config.  Not the driver's bench (bench.py measures the C4 sweep)."""
from __future__ import annotations

import argparse
import ctypes as C
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


def median_time(fn, sync, n):
    ts = []
    for _ in range(n):
        sync()
        t = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts))


def run(name, d, T, calls):
    model = cx.synth.lgssm_chain(T, d=d, seed=5)
    dev = cx.DeviceGraph(dim=d, schedule=L.SCHED_CHAIN_SCAN)
    cx.synth.load_into_device(model, dev)
    dev.sweep(1)
    dev.sync()
    ids = np.ascontiguousarray(model.x_ids, dtype=np.int64)
    pid = ids.ctypes.data_as(C.POINTER(C.c_int64))
    rows = np.zeros((T, d + d * d))
    prow = rows.ctypes.data_as(C.POINTER(C.c_double))
    cnt = (C.c_int64 * 4)()
    out = {"config": name, "workload": f"d={d} chain T={T} ({len(model.edge_var)} edges) after one chain-scan sweep, the {T} states", "calls": calls,
           "row_bytes": int(rows.nbytes), "beta_bytes_per_buffer": int((T - 1) * (d + d * d) * 8)}
    for key, mode, lag in (("predicted", L.CAUSAL_PREDICTED, 0), ("filtered", L.CAUSAL_FILTERED, 0), ("lag1", L.CAUSAL_FILTERED, 1), ("lag8", L.CAUSAL_FILTERED, 8)):
        def call():
            rc = dev.lib.cx_causal_marginals_mfma(dev.h, mode, lag, T, pid, prow, cnt)
            assert rc == 0, dev.lib.cx_last_error(dev.h)
        call()                                      # warm-up: builds the rows of this request
        out[f"ms_{key}"] = median_time(call, dev.sync, calls) * 1e3
        out[f"{key}_counts"] = [int(x) for x in cnt]
    pre = np.zeros((T, d + d * d + 2))
    ppre = pre.ctypes.data_as(C.POINTER(C.c_double))
    tot = C.c_double()

    def predictive():
        rc = dev.lib.cx_predictive_mfma(dev.h, L.PREDICT_CAUSAL, 0, None, ppre, C.byref(tot), cnt)
        assert rc == 0, dev.lib.cx_last_error(dev.h)
    predictive()
    out["ms_predictive_causal_with_rows"] = median_time(predictive, dev.sync, calls) * 1e3
    dev.close()
    fused = cx.DeviceGraph(dim=d, schedule=L.SCHED_FUSED)
    cx.synth.load_into_device(model, fused, seed_variance=1e6)
    fused.sweep(3)
    out["ms_per_fused_sweep"] = median_time(lambda: fused.sweep(1), fused.sync, 10) * 1e3
    fused.close()
    out["ms_per_lag_pass"] = (out["ms_lag8"] - out["ms_lag1"]) / 7.0
    out["predicted_over_predictive"] = out["ms_predicted"] / out["ms_predictive_causal_with_rows"]
    out["filtered_over_predictive"] = out["ms_filtered"] / out["ms_predictive_causal_with_rows"]
    out["lag_pass_over_fused_sweep"] = out["ms_per_lag_pass"] / out["ms_per_fused_sweep"]
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30, help="calls per median (3.3 GB to the host per call at d = 64, T = 1e5)")
    ap.add_argument("--T", type=int, default=100_000)
    ap.add_argument("--only", default="", help="comma-separated subset of C5,d16,d32")
    a = ap.parse_args()
    only = set(a.only.split(",")) if a.only else {"C5", "d16", "d32"}
    for name, d in (("d16", 16), ("d32", 32), ("C5", 64)):
        if name in only:
            run(name, d, a.T, a.calls)


if __name__ == "__main__":
    main()
