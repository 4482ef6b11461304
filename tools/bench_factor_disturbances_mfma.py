"""tools/bench_factor_disturbances_mfma.py — cost of one cx_factor_disturbances_mfma call beside one
cx_factor_statistics_mfma call on the same handle: lgssm_chain(10**5, d), d = 16 / 32 / 64, after one chain-scan sweep.  Three calls
interleaved on one handle (S D R S D R …), a host clock around each call and a synchronise, after a warm-up call of each (the first call
builds its lists and allocates): the statistics by parameter set, the disturbances with out == NULL (scores, total and counts alone) and
the disturbances with rows, into arrays allocated once (the C entry point directly: DeviceGraph.factor_disturbances_mfma allocates and
copies its result, which at d = 64 is 6.7 GB).  Medians and the spread (min, max) of --calls calls each, the two ratios to the
statistics call with that call's own spread beside them, and the rate at which the payload reached the host: payload bytes over (rows -
scores only).  Prints one JSON line per dim.  Not the driver's bench (bench.py measures the C4 sweep)."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np


def _spread(ts):
    ts = np.asarray(ts) * 1e3
    return {"median_ms": float(np.median(ts)), "min_ms": float(ts.min()), "max_ms": float(ts.max())}


def _timed(call, dev):
    dev.sync()
    t = time.perf_counter()
    call()
    dev.sync()
    return time.perf_counter() - t


def run(cx, L, d, T, calls, with_rows):
    model = cx.synth.lgssm_chain(T, d=d, seed=5)
    dev = cx.DeviceGraph(dim=d, schedule=L.SCHED_CHAIN_SCAN)
    cx.synth.load_into_device(model, dev)
    dev.sweep(1)
    n = len(dev.factor_disturbance_rows_mfma())
    pd, p64 = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    scores, tot, c4 = np.zeros((n, 2)), C.c_double(), np.zeros(4, np.int64)
    rows = np.zeros((n, d + d * d)) if with_rows else None

    def disturbances(out):
        rc = dev.lib.cx_factor_disturbances_mfma(dev.h, 0, None, None if out is None else out.ctypes.data_as(pd), scores.ctypes.data_as(pd), C.byref(tot),
                                                 c4.ctypes.data_as(p64))
        assert rc == L.OK, dev.lib.cx_last_error(dev.h)

    todo = {"statistics": lambda: dev.factor_statistics_mfma(n_groups=2), "scores_only": lambda: disturbances(None)}
    if with_rows:
        todo["with_rows"] = lambda: disturbances(rows)
    for call in todo.values():      # warm-up: the lists, the workspace, the row buffer, the host pages of the arrays
        call()
    ts = {k: [] for k in todo}
    for _ in range(calls):
        for k, call in todo.items():
            ts[k].append(_timed(call, dev))
    out = {"d": d, "T": T, "rows": n, "calls": calls, "counts": [int(x) for x in c4], "total": float(tot.value)}
    for k in todo:
        out[k] = _spread(ts[k])
    st = out["statistics"]
    out["statistics_spread"] = (st["max_ms"] - st["min_ms"]) / st["median_ms"]
    out["scores_only_over_statistics"] = out["scores_only"]["median_ms"] / st["median_ms"]
    if with_rows:
        out["with_rows_over_statistics"] = out["with_rows"]["median_ms"] / st["median_ms"]
        out["payload_bytes"] = int(rows.nbytes)
        extra = (out["with_rows"]["median_ms"] - out["scores_only"]["median_ms"]) * 1e-3
        out["payload_GB_per_s"] = rows.nbytes / extra / 1e9 if extra > 0 else None
    dev.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--T", type=int, default=10**5)
    ap.add_argument("--dims", default="16,32,64")
    ap.add_argument("--no-rows", action="store_true", help="the statistics and the scores-only call alone")
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import cortex.jl_amd as cx
    from cortex.jl_amd import _lib as L

    for d in (int(x) for x in a.dims.split(",")):
        run(cx, L, d, a.T, a.calls, not a.no_rows)


if __name__ == "__main__":
    main()
