"""tools/bench_functionals_mfma.py — cost of one cx_linear_moments_mfma call on T = 1e5 chains at d = 16, 32 and 64 after
one chain-scan sweep: K = 16 and K = 64 window means of 1,000 consecutive states (every component, windows spread evenly over the chain),
with the covariance and for the means alone; and beside it, in the same process on the same handle, cx_sample_posterior_mfma at S = K for
the states (the Monte-Carlo route to the same quantity) and one chain-scan sweep.  Median wall time of `calls` synchronised calls after a
warm-up call (the first call builds the plan and allocates the link workspace).  The calls go to the C entry points with host arrays made
beforehand, so that the time is the library's (the host merge of the entries, kernels, chunks and copies), not numpy's.  Prints one JSON
line per config.  --profile: one call of cx_linear_moments_mfma per K and nothing else, for a kernel trace.  Not the driver's bench
(bench.py measures the C4 sweep)."""
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


def windows(x_ids, K, width, d):
    """K window means of `width` consecutive states, CSR"""
    T = len(x_ids)
    starts = np.linspace(0, T - width, K).astype(np.int64)
    off = (np.arange(K + 1) * width).astype(np.int64)
    ids = np.concatenate([x_ids[s:s + width] for s in starts]).astype(np.int64)
    w = np.full((K * width, d), 1.0 / (width * d))
    return off, ids, w


def run(name, d, T, calls, Ks, width, profile):
    model = cx.synth.lgssm_chain(T, d=d, seed=5)
    dev = cx.DeviceGraph(dim=d, schedule=L.SCHED_CHAIN_SCAN)
    cx.synth.load_into_device(model, dev)
    dev.sweep(1)
    dev.sync()
    xid = np.ascontiguousarray(model.x_ids, dtype=np.int64)
    pxid = xid.ctypes.data_as(C.POINTER(C.c_int64))
    cnt = (C.c_int64 * 4)()
    out = {"config": name, "workload": f"d={d} chain T={T} after one chain-scan sweep, window means of {width} states", "calls": calls,
           "link_bytes": int(T * (2 * d * d + d) * 8)}
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    for K in Ks:
        off, ids, w = windows(xid, K, min(width, T), d)
        mean, cov = np.zeros(K), np.zeros((K, K))

        def fn(with_cov=True):
            rc = dev.lib.cx_linear_moments_mfma(dev.h, K, off.ctypes.data_as(pi), ids.ctypes.data_as(pi), w.ctypes.data_as(pd), mean.ctypes.data_as(pd),
                                                cov.ctypes.data_as(pd) if with_cov else None, cnt)
            assert rc == 0, dev.lib.cx_last_error(dev.h)
        fn()                                        # warm-up: the plan, the link workspace, g
        if profile:
            continue
        assert np.isfinite(mean).all() and np.isfinite(cov).all() and (np.diag(cov) > 0).all()
        out[f"ms_K{K}"] = median_time(fn, dev.sync, calls) * 1e3
        out[f"ms_means_K{K}"] = median_time(lambda: fn(False), dev.sync, calls) * 1e3
        out[f"counts_K{K}"] = [int(v) for v in cnt]
        out[f"out_bytes_K{K}"] = int(mean.nbytes + cov.nbytes)
        x = np.zeros((K, T, d))
        px = x.ctypes.data_as(pd)

        def sample():
            rc = dev.lib.cx_sample_posterior_mfma(dev.h, K, C.c_uint64(7), None, T, pxid, px, cnt)
            assert rc == 0, dev.lib.cx_last_error(dev.h)
        sample()
        out[f"ms_sample_S{K}"] = median_time(sample, dev.sync, max(3, calls // 2)) * 1e3
        out[f"sample_out_bytes_S{K}"] = int(x.nbytes)
        del x
    if not profile:
        out["ms_per_chain_scan_sweep"] = median_time(lambda: dev.sweep(1), dev.sync, 10) * 1e3
        print(json.dumps(out), flush=True)
    dev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=8, help="calls per median")
    ap.add_argument("--T", type=int, default=100_000)
    ap.add_argument("--width", type=int, default=1000, help="states per window")
    ap.add_argument("--only", default="", help="comma-separated subset of d16,d32,d64")
    ap.add_argument("--K", default="16,64", help="comma-separated numbers of functionals")
    ap.add_argument("--profile", action="store_true", help="one call per K and nothing else (for a kernel trace)")
    a = ap.parse_args()
    only = set(a.only.split(",")) if a.only else {"d16", "d32", "d64"}
    Ks = [int(s) for s in a.K.split(",")]
    for name, d in (("d16", 16), ("d32", 32), ("d64", 64)):
        if name in only:
            run(name, d, a.T, a.calls, Ks, a.width, a.profile)


if __name__ == "__main__":
    main()
