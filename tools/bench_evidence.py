"""tools/bench_evidence.py — cost of one cx_log_evidence call on three configs: C4 after 200 fused sweeps, a C2-size
scalar chain and a C3-size d = 4 chain under the chain scan.  Median wall time of >= 20 synchronised calls after a warm-up call (the
first call of a handle builds its work lists), the bytes the passes must move, and that traffic per second against 8 TB/s.
Prints one JSON line per config.  Not the driver's bench (bench.py measures the C4 sweep)."""
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

HBM = 8e12


def traffic(model, d: int) -> int:
    """bytes the passes must move at least: pass 1 reads every message into a non-observed variable once (the opaque ones twice), the
    per-variable tables (vbase, degree, flags, record: 13 B) and writes the scratch; pass 2 reads per two-variable factor its record
    (16 B + parameters), both flags, both messages and both scratch rows"""
    nt = d * (d + 1) // 2
    msg = 16 if d == 1 else 8 * (2 * ((d + nt + 1) // 2))
    row = 16 if d == 1 else 8 * (((d + nt + 1) + 1) // 2 * 2)
    obs = set(int(v) for v in model.data_var)
    ev = np.asarray(model.edge_var)
    into_free = int((~np.isin(ev, np.fromiter(obs, np.int64, len(obs)))).sum()) if obs else len(ev)
    nv = len(np.unique(ev))
    kinds = np.asarray(model.factor_kind)
    n_pair = int((kinds != L.FACTOR_OPAQUE).sum())
    n_opq = len(model.prior_var)
    par = 8 if d == 1 else 4
    p1 = into_free * msg + n_opq * msg + nv * 13 + (nv - len(obs)) * row
    p2 = n_pair * (16 + par + 2 * (1 + msg + row))
    return p1 + p2


def measure(dev, calls: int) -> float:
    dev.log_evidence()                          # warm-up: builds the work lists
    ts = []
    for _ in range(calls):
        dev.sync()
        t = time.perf_counter()
        dev.log_evidence()                      # synchronous: the value is on the host at return
        ts.append(time.perf_counter() - t)
    return float(np.median(ts))


def run(name, model, schedule, sweeps, calls, workload):
    dev = cx.DeviceGraph(dim=model.dim, schedule=schedule)
    cx.synth.load_into_device(model, dev, seed_variance=1e6 if schedule == L.SCHED_FUSED else None)
    dev.sweep(sweeps)
    dev.sync()
    value, counts = dev.log_evidence()
    dt = measure(dev, calls)
    b = traffic(model, model.dim)
    out = {"config": name, "workload": workload, "ms_per_call": dt * 1e3, "calls": calls, "bytes_per_call": b, "bytes_per_s": b / dt,
           "fraction_of_8TBps": b / dt / HBM, "log_evidence": value, "counts": counts}
    dev.close()
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--only", default="", help="comma-separated subset of C4,C2,C3")
    a = ap.parse_args()
    only = set(a.only.split(",")) if a.only else {"C4", "C2", "C3"}
    if "C4" in only:
        m = cx.synth.gaussian_grid(1415, 1415)
        run("C4", m, L.SCHED_FUSED, 200, a.calls, f"1415x1415 Gaussian grid ({len(m.edge_var)} edges) after 200 fused sweeps: the Bethe estimate")
    if "C2" in only:
        m = cx.synth.ssm_chain(250_001)
        run("C2", m, L.SCHED_CHAIN_SCAN, 1, a.calls, f"scalar chain T=250001 ({len(m.edge_var)} edges) after one chain-scan sweep: exact")
    if "C3" in only:
        m = cx.synth.lgssm_chain(1_000_000, d=4)
        run("C3", m, L.SCHED_CHAIN_SCAN, 1, a.calls, f"d=4 chain T=1000000 ({len(m.edge_var)} edges) after one chain-scan sweep: exact")


if __name__ == "__main__":
    main()
