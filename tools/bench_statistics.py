"""tools/bench_statistics.py — cost of one cx_factor_statistics and one cx_factor_beliefs call next to cx_log_evidence on
the same handle: a C3-size d = 4 chain under the chain scan (one group per parameter set) and C4 after 200 fused sweeps (one group for
every factor).  Median wall time of >= 20 synchronised calls after a warm-up call (the first call builds the work lists), the bytes
the passes must move (tools/bench_evidence.py's count plus the statistics rows) and that traffic per second against 8 TB/s.  The
beliefs are those of a fixed, evenly spaced subset of 2^17 factors (their cost is the variable pass plus per-factor work; all of a
C3 chain's beliefs are 1.2 GB to copy to the host).  Prints one JSON line per config.  Not the driver's bench."""
from __future__ import annotations

import argparse
import importlib.util
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

_spec = importlib.util.spec_from_file_location("bench_evidence", os.path.join(ROOT, "tools", "bench_evidence.py"))
bench_evidence = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bench_evidence)
HBM = bench_evidence.HBM
N_BELIEFS = 1 << 17


def median_ms(fn, dev, calls: int) -> float:
    fn()                                        # warm-up: builds the work lists
    ts = []
    for _ in range(calls):
        dev.sync()
        t = time.perf_counter()
        fn()                                    # synchronous: the result is on the host at return
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e3


def run(name, model, schedule, sweeps, calls, workload, stats_call):
    dev = cx.DeviceGraph(dim=model.dim, schedule=schedule)
    cx.synth.load_into_device(model, dev, seed_variance=1e6 if schedule == L.SCHED_FUSED else None)
    dev.sweep(sweeps)
    dev.sync()
    d = model.dim
    rule = np.asarray(model.factor_ids)[np.asarray(model.factor_kind) != L.FACTOR_OPAQUE]
    sub = rule[np.linspace(0, len(rule) - 1, min(N_BELIEFS, len(rule))).astype(np.int64)]
    ms_ev = median_ms(dev.log_evidence, dev, calls)
    ms_st = median_ms(lambda: stats_call(dev), dev, calls)
    ms_be = median_ms(lambda: dev.factor_beliefs(sub), dev, calls)
    stats, counts = stats_call(dev)
    nw = 3 + 2 * d + 3 * d * d
    b = bench_evidence.traffic(model, d)
    b_st = b + (len(rule) + 63) // 64 * 2 * nw * 8 * 2                  # + the chunk rows, written and read once
    out = {"config": name, "workload": workload, "calls": calls, "ms_log_evidence": ms_ev, "ms_factor_statistics": ms_st,
           "ms_factor_beliefs_2^17": ms_be, "statistics_over_evidence": ms_st / ms_ev, "bytes_statistics": b_st,
           "fraction_of_8TBps_statistics": b_st / (ms_st * 1e-3) / HBM, "counts": counts, "n_per_group": stats["n"].tolist()}
    dev.close()
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--only", default="", help="comma-separated subset of C3,C4")
    a = ap.parse_args()
    only = set(a.only.split(",")) if a.only else {"C3", "C4"}
    if "C3" in only:
        m = cx.synth.lgssm_chain(1_000_000, d=4)
        run("C3", m, L.SCHED_CHAIN_SCAN, 1, a.calls, f"d=4 chain T=1000000 ({len(m.edge_var)} edges) after one chain-scan sweep, one group per set",
            lambda dev: dev.factor_statistics(n_groups=2))
    if "C4" in only:
        m = cx.synth.gaussian_grid(1415, 1415)
        fids = np.asarray(m.factor_ids)[np.asarray(m.factor_kind) != L.FACTOR_OPAQUE]
        groups = np.zeros(len(fids), np.int64)
        run("C4", m, L.SCHED_FUSED, 200, a.calls, f"1415x1415 Gaussian grid ({len(m.edge_var)} edges) after 200 fused sweeps, one group",
            lambda dev: dev.factor_statistics(fids, groups, n_groups=1))


if __name__ == "__main__":
    main()
