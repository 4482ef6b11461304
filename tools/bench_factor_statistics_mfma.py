"""tools/bench_factor_statistics_mfma.py — cost of one cx_factor_statistics_mfma call with the parameter-set grouping on
T = 1e5 chains at d = 64 (config C5), 16 and 32 after one chain-scan sweep, and beside it, in the same process and on the same handle,
one cx_log_evidence_mfma call; then one fused sweep of the same model.  Median wall time of `calls` synchronised calls after a warm-up
call (the first call of a handle builds its lists and allocates its workspace); the fused sweep: the median of 10 synchronised single
sweeps after 3 warm-up sweeps.  Also the device workspace of the statistics in bytes, from the layout the header states (wave
workspaces of 6 KD² + 4 KD doubles, one row of 2d + 3d² doubles per partial) and, as a check, the growth of the handle's
device_bytes over the first call.  Prints one JSON line per config.  Not the driver's bench (bench.py measures the C4 sweep)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import cortex.jl_amd as cx                      # noqa: E402
from cortex.jl_amd import _lib as L            # noqa: E402
from tools.bench_evidence_mfma import median_time      # noqa: E402

def max_waves(kd):      # cx_learn_mfma.hip: max_waves
    return 1024 if kd == 64 else 2048


def workspace_bytes(n_factors_per_group, d, kd):
    total = sum(n_factors_per_group)
    per = max(1, -(-total // max_waves(kd)))
    partials = sum(-(-n // per) for n in n_factors_per_group if n)
    waves = min(partials, max_waves(kd))
    return 8 * (waves * (6 * kd * kd + 4 * kd) + partials * (2 * d + 3 * d * d)), partials, waves


def run(name, d, T, calls):
    model = cx.synth.lgssm_chain(T, d=d, seed=5)
    kd = 16 if d <= 16 else 32 if d <= 32 else 64
    dev = cx.DeviceGraph(dim=d, schedule=L.SCHED_CHAIN_SCAN)
    cx.synth.load_into_device(model, dev)
    dev.sweep(1)
    dev.sync()
    value, _ = dev.log_evidence_mfma()                   # warm-up: builds the term lists
    before = dev.stats()["device_bytes"]
    stats, counts = dev.factor_statistics_mfma(n_groups=2)      # warm-up: builds the lists, allocates the workspace
    grown = dev.stats()["device_bytes"] - before
    dt = median_time(lambda: dev.factor_statistics_mfma(n_groups=2), dev.sync, calls)      # (synchronous: the rows are on the host at return)
    de = median_time(dev.log_evidence_mfma, dev.sync, calls)
    dev.close()
    fused = cx.DeviceGraph(dim=d, schedule=L.SCHED_FUSED)
    cx.synth.load_into_device(model, fused, seed_variance=1e6)
    fused.sweep(3)
    ds = median_time(lambda: fused.sweep(1), fused.sync, 10)
    fused.close()
    ws, partials, waves = workspace_bytes([T - 1, T], d, kd)
    out = {"config": name, "workload": f"d={d} chain T={T} ({len(model.edge_var)} edges) after one chain-scan sweep", "calls": calls,
           "ms_per_statistics_call": dt * 1e3, "ms_per_evidence_call": de * 1e3, "ms_per_fused_sweep": ds * 1e3,
           "statistics_over_evidence": dt / de, "statistics_over_fused_sweep": dt / ds, "workspace_bytes": ws, "partials": partials, "waves": waves,
           "device_bytes_grown_by_first_call": int(grown), "counts": counts, "log_evidence": value,
           "trace_Srr_over_n": [float(np.trace(stats["S_rr"][g]) / stats["n"][g]) for g in range(2)]}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--T", type=int, default=100_000)
    ap.add_argument("--only", default="", help="comma-separated subset of C5,d16,d32")
    a = ap.parse_args()
    only = set(a.only.split(",")) if a.only else {"C5", "d16", "d32"}
    for name, d in (("d16", 16), ("d32", 32), ("C5", 64)):
        if name in only:
            run(name, d, a.T, a.calls)


if __name__ == "__main__":
    main()
