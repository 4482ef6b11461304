"""tools/bench_evidence_components.py — cost of one cx_log_evidence_components call next to cx_log_evidence on the same
handle in the same run, for the two extremes of the segmented sum and one in between:

  a  4096 x lgssm_chain(256, d=2) in one handle, chain scan     many components of ~ 1000 terms
  b  lgssm_chain(10**6, d=4), chain scan                        one component of 3 x 10^6 terms
  c  the C4 grid (1415 x 1415) after 20 fused sweeps            one component of ~ 6 x 10^6 terms

Per call a host clock around the synchronous call, after a warm-up call of each (the first component call builds the plan; its time is
reported as plan_ms), the two functions interleaved, medians and the spread (min, max) of --calls calls each.  --total-only times
cx_log_evidence alone: with --root it imports the package from another tree (an A/B build of another commit, which may lack the new
symbols).  Prints one JSON line per workload.  Not the driver's bench (bench.py measures the C4 sweep)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np


def _spread(ts):
    ts = np.asarray(ts) * 1e3
    return {"median_ms": float(np.median(ts)), "min_ms": float(ts.min()), "max_ms": float(ts.max())}


def run(cx, L, name, model, schedule, sweeps, calls, total_only, seed_variance=None):
    dev = cx.DeviceGraph(dim=model.dim, schedule=schedule)
    cx.synth.load_into_device(model, dev, seed_variance=seed_variance)
    dev.sweep(sweeps)
    dev.sync()
    out = {"workload": name, "calls": calls, "variables": int(dev.stats()["n_variables"]), "factors": int(dev.stats()["n_factors"])}
    dev.log_evidence()                                   # warm-up: builds the work lists
    if not total_only:
        t = time.perf_counter()
        values, _, _ = dev.log_evidence_components()     # warm-up: builds the component plan
        out["plan_ms"] = (time.perf_counter() - t) * 1e3
        out["components"] = int(len(values))
    tot, comp = [], []
    for _ in range(calls):
        dev.sync()
        t = time.perf_counter()
        dev.log_evidence()
        tot.append(time.perf_counter() - t)
        if not total_only:
            dev.sync()
            t = time.perf_counter()
            dev.log_evidence_components()
            comp.append(time.perf_counter() - t)
    out["log_evidence"] = _spread(tot)
    if not total_only:
        out["log_evidence_components"] = _spread(comp)
        out["components_over_total"] = out["log_evidence_components"]["median_ms"] / out["log_evidence"]["median_ms"]
    dev.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--only", default="a,b,c", help="comma-separated subset of a,b,c")
    ap.add_argument("--total-only", action="store_true", help="time cx_log_evidence alone")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the tree to import cortex.jl_amd from")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import cortex.jl_amd as cx
    from cortex.jl_amd import _lib as L

    only = set(a.only.split(","))
    if "a" in only:
        first = cx.synth.lgssm_chain(256, d=2, seed=1)
        A, Q, R = first.meta["A"], first.meta["Q"], first.meta["R"]
        kinds = [first] + [cx.synth.lgssm_chain(256, d=2, seed=1 + i, A=A, Q=Q, R=R) for i in range(1, 16)]
        run(cx, L, "a: 4096 x lgssm_chain(256, d=2), chain scan", cx.synth.concat_models([kinds[i % 16] for i in range(4096)]), L.SCHED_CHAIN_SCAN, 1,
            a.calls, a.total_only)
    if "b" in only:
        run(cx, L, "b: lgssm_chain(10**6, d=4), chain scan", cx.synth.lgssm_chain(10**6, d=4), L.SCHED_CHAIN_SCAN, 1, a.calls, a.total_only)
    if "c" in only:
        run(cx, L, "c: gaussian_grid(1415, 1415) after 20 fused sweeps", cx.synth.gaussian_grid(1415, 1415), L.SCHED_FUSED, 20, a.calls, a.total_only,
            seed_variance=1e6)


if __name__ == "__main__":
    main()
