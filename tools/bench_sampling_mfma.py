"""tools/bench_sampling_mfma.py — cost of one cx_sample_posterior_mfma call on T = 1e5 chains at d = 16, 32 and 64 (config
C5) after one chain-scan sweep, for the states only (variable_ids = x_ids), S = 16 and S = 256 samples under a seed; and beside it, in
the same process on the same handle, one chain-scan sweep and the device-to-host copy of an output of that size on its own (a plain
hipMemcpy into the same pageable host array: what the call cannot go below).  Median wall time of `calls` synchronised calls after a
warm-up call (the first call builds the plan and allocates the link workspace).  The calls go to the C entry point with one host array
made beforehand, so that the time is the library's (kernels, chunks and device-to-host copies), not numpy's; the sweep: the median of 10
synchronised single sweeps after the first.  Prints one JSON line per config.  --profile: one call and nothing else, for a kernel trace
(rocprofv3 --kernel-trace --stats --output-format csv -- python tools/bench_sampling_mfma.py --only C5 --samples 16 --profile).  Not the driver's bench
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


def copy_time(nbytes, host, n):
    """median time of a plain device-to-host copy of nbytes into `host` (the HIP runtime the library has loaded)"""
    hip = C.CDLL([ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln][0])
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    p = C.c_void_p()
    if hip.hipMalloc(C.byref(p), nbytes) != 0:
        return None
    ts = []
    for _ in range(n + 1):
        t = time.perf_counter()
        assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), p, nbytes, 2) == 0      # hipMemcpyDeviceToHost
        ts.append(time.perf_counter() - t)
    hip.hipFree(p)
    return float(np.median(ts[1:]))


def run(name, d, T, calls, samples, profile):
    model = cx.synth.lgssm_chain(T, d=d, seed=5)
    dev = cx.DeviceGraph(dim=d, schedule=L.SCHED_CHAIN_SCAN)
    cx.synth.load_into_device(model, dev)
    dev.sweep(1)
    dev.sync()
    ids = np.ascontiguousarray(model.x_ids, dtype=np.int64)
    pid = ids.ctypes.data_as(C.POINTER(C.c_int64))
    cnt = (C.c_int64 * 4)()
    out = {"config": name, "workload": f"d={d} chain T={T} ({len(model.edge_var)} edges) after one chain-scan sweep, the {T} states", "calls": calls,
           "link_bytes": int(T * (2 * d * d + d) * 8)}
    for S in samples:
        x = np.zeros((S, T, d))
        px = x.ctypes.data_as(C.POINTER(C.c_double))

        def call():
            rc = dev.lib.cx_sample_posterior_mfma(dev.h, S, C.c_uint64(7), None, T, pid, px, cnt)
            assert rc == 0, dev.lib.cx_last_error(dev.h)
        call()                                      # warm-up: the plan, the link workspace, the host pages
        if profile:
            continue
        n = calls if S <= 16 else max(3, calls // 4)
        out[f"ms_S{S}"] = median_time(call, dev.sync, n) * 1e3
        out[f"counts_S{S}"] = [int(v) for v in cnt]
        out[f"out_bytes_S{S}"] = int(x.nbytes)
        c = copy_time(x.nbytes, x, 3)
        out[f"ms_copy_S{S}"] = None if c is None else c * 1e3
        assert np.isfinite(x).all()
        del x
    if not profile:
        out["ms_per_chain_scan_sweep"] = median_time(lambda: dev.sweep(1), dev.sync, 10) * 1e3
        for S in samples:
            out[f"S{S}_over_sweep"] = out[f"ms_S{S}"] / out["ms_per_chain_scan_sweep"]
            if out[f"ms_copy_S{S}"] is not None:
                out[f"S{S}_device_over_sweep"] = (out[f"ms_S{S}"] - out[f"ms_copy_S{S}"]) / out["ms_per_chain_scan_sweep"]
        print(json.dumps(out), flush=True)
    dev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=12, help="calls per median at S = 16 (a quarter of it, 3 at the least, beyond)")
    ap.add_argument("--T", type=int, default=100_000)
    ap.add_argument("--only", default="", help="comma-separated subset of C5,d16,d32")
    ap.add_argument("--samples", default="16,256", help="comma-separated sample counts")
    ap.add_argument("--profile", action="store_true", help="one call per sample count and nothing else (for a kernel trace)")
    a = ap.parse_args()
    only = set(a.only.split(",")) if a.only else {"C5", "d16", "d32"}
    samples = [int(s) for s in a.samples.split(",")]
    for name, d in (("d16", 16), ("d32", 32), ("C5", 64)):
        if name in only:
            run(name, d, a.T, a.calls, samples, a.profile)


if __name__ == "__main__":
    main()
