"""tools/bench_predictive_mfma.py — cost of one cx_predictive_mfma call on T = 1e5 chains at d = 16, 32 and 64 (config
C5) after one chain-scan sweep: CX_PREDICT_CAUSAL and CX_PREDICT_LOO, each with the total alone (out == NULL) and with the rows, and
beside them, in the same process on the same handle, one cx_log_evidence_mfma call.  Median wall time of 30 synchronised calls after a
warm-up call (the first call of a request builds its rows).  The calls with rows go to the C entry point with one host array made
beforehand, so that the time is the library's (kernel chunks and device-to-host copies), not numpy's.  Prints one JSON line per config.
Not the driver's bench (bench.py measures the C4 sweep)."""
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


def run(name, d, T, calls, row_calls):
    model = cx.synth.lgssm_chain(T, d=d, seed=5)
    dev = cx.DeviceGraph(dim=d, schedule=L.SCHED_CHAIN_SCAN)
    cx.synth.load_into_device(model, dev)
    dev.sweep(1)
    dev.sync()
    value, _ = dev.log_evidence_mfma()              # warm-up: builds the term lists
    out = {"config": name, "workload": f"d={d} chain T={T} ({len(model.edge_var)} edges) after one chain-scan sweep", "calls": calls, "row_calls": row_calls,
           "ms_log_evidence_mfma": median_time(dev.log_evidence_mfma, dev.sync, calls) * 1e3, "log_evidence": value}
    no = d + d * d + 2
    rows = np.zeros((T, no))
    out["row_bytes"] = int(rows.nbytes)
    tot, cnt = C.c_double(), (C.c_int64 * 4)()
    prow = rows.ctypes.data_as(C.POINTER(C.c_double))
    for mode, m in (("causal", L.PREDICT_CAUSAL), ("loo", L.PREDICT_LOO)):
        def call(p):
            rc = dev.lib.cx_predictive_mfma(dev.h, m, 0, None, p, C.byref(tot), cnt)
            assert rc == 0, dev.lib.cx_last_error(dev.h)
        call(None)                                  # warm-up: builds the rows of this mode
        out[f"ms_{mode}_total_only"] = median_time(lambda: call(None), dev.sync, calls) * 1e3
        lean = tot.value
        call(prow)
        out[f"ms_{mode}_with_rows"] = median_time(lambda: call(prow), dev.sync, row_calls) * 1e3
        assert np.float64(tot.value).tobytes() == np.float64(lean).tobytes()
        out[f"{mode}_total"] = tot.value
        out[f"{mode}_counts"] = [int(x) for x in cnt]
        out[f"{mode}_total_only_over_log_evidence"] = out[f"ms_{mode}_total_only"] / out["ms_log_evidence_mfma"]
    dev.close()
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--row-calls", type=int, default=30, help="calls with rows (3.3 GB to the host per call at d = 64, T = 1e5)")
    ap.add_argument("--T", type=int, default=100_000)
    ap.add_argument("--only", default="", help="comma-separated subset of C5,d16,d32")
    a = ap.parse_args()
    only = set(a.only.split(",")) if a.only else {"C5", "d16", "d32"}
    for name, d in (("d16", 16), ("d32", 32), ("C5", 64)):
        if name in only:
            run(name, d, a.T, a.calls, a.row_calls)


if __name__ == "__main__":
    main()
