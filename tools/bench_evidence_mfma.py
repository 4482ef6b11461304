"""tools/bench_evidence_mfma.py — cost of one cx_log_evidence_mfma call on T = 1e5 chains at d = 64 (config C5), 16 and
32 after one chain-scan sweep, and beside it, in the same process, one fused sweep of the same model.  Median wall time of 30
synchronised calls after a warm-up call (the first call of a handle builds its term lists); the fused sweep: the median of 10
synchronised single sweeps after 3 warm-up sweeps.  Also the message bytes the terms read (every source record once per term that
names it) and that traffic per second against 8 TB/s.  Prints one JSON line per config.  Not the driver's bench (bench.py measures the
C4 sweep)."""
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


def traffic(model, kd: int) -> int:
    """message bytes one call reads: a variable term every message of its variable, a factor term the other messages of each free end
    (records of kd + kd^2 doubles at the internal dim kd); the rule tables and data vectors are small beside them"""
    ev, ef = np.asarray(model.edge_var), np.asarray(model.edge_fac)
    ids, inv, deg = np.unique(ev, return_inverse=True, return_counts=True)
    free = ~np.isin(ids, np.asarray(model.data_var))
    rule = np.isin(ef, np.asarray(model.factor_ids)[np.asarray(model.factor_kind) != L.FACTOR_OPAQUE])
    n_rule = np.bincount(inv[rule], minlength=len(ids))
    records = int(deg[free & (n_rule != 1)].sum())               # variable terms
    records += int((deg[inv[rule]] - 1)[free[inv[rule]]].sum())  # factor terms: per free end, the variable's other messages
    return records * 8 * (kd + kd * kd)


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
    kd = 16 if d <= 16 else 32 if d <= 32 else 64
    dev = cx.DeviceGraph(dim=d, schedule=L.SCHED_CHAIN_SCAN)
    cx.synth.load_into_device(model, dev)
    dev.sweep(1)
    dev.sync()
    value, counts = dev.log_evidence_mfma()         # warm-up: builds the term lists
    dt = median_time(dev.log_evidence_mfma, dev.sync, calls)      # (synchronous: the value is on the host at return)
    dev.close()
    fused = cx.DeviceGraph(dim=d, schedule=L.SCHED_FUSED)
    cx.synth.load_into_device(model, fused, seed_variance=1e6)
    fused.sweep(3)
    ds = median_time(lambda: fused.sweep(1), fused.sync, 10)
    fused.close()
    b = traffic(model, kd)
    out = {"config": name, "workload": f"d={d} chain T={T} ({len(model.edge_var)} edges) after one chain-scan sweep", "ms_per_call": dt * 1e3, "calls": calls,
           "ms_per_fused_sweep": ds * 1e3, "call_over_fused_sweep": dt / ds, "message_bytes_per_call": b, "bytes_per_s": b / dt,
           "fraction_of_8TBps": b / dt / HBM, "log_evidence": value, "counts": counts}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--T", type=int, default=100_000)
    ap.add_argument("--only", default="", help="comma-separated subset of C5,d16,d32")
    a = ap.parse_args()
    only = set(a.only.split(",")) if a.only else {"C5", "d16", "d32"}
    for name, d in (("C5", 64), ("d16", 16), ("d32", 32)):
        if name in only:
            run(name, d, a.T, a.calls)


if __name__ == "__main__":
    main()
