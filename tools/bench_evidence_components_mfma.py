"""tools/bench_evidence_components_mfma.py — cost of one cx_log_evidence_components_mfma call next to cx_log_evidence_mfma
on the same handle in the same process, for the two extremes of the segmented sum at the matrix-core dims:

  a16, a32, a64  lgssm_chain(10**5, d) after one chain-scan sweep, d = 16 / 32 / 64     one component of ~ 3 x 10^5 terms (k_ev_span)
  b              1000 x lgssm_chain(100, d=16) in one handle, chain scan                1000 components of 299 terms

Per call a host clock around the synchronous call, after a warm-up call of each (the first component call builds the plan; its time is
reported as plan_ms), the two functions interleaved, medians and the spread (min, max) of --calls calls each.  Prints one JSON line per
workload.  --profile: after the warm-up, --calls component calls and nothing else, for a kernel trace in a run of its own.  Not the
driver's bench (bench.py measures the C4 sweep)."""
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


def run(cx, L, name, model, calls, profile):
    dev = cx.DeviceGraph(dim=model.dim, schedule=L.SCHED_CHAIN_SCAN)
    cx.synth.load_into_device(model, dev)
    dev.sweep(1)
    dev.sync()
    out = {"workload": name, "calls": calls, "variables": int(dev.stats()["n_variables"]), "factors": int(dev.stats()["n_factors"])}
    total, cnt = dev.log_evidence_mfma()                      # warm-up: builds the term lists
    t = time.perf_counter()
    values, _, counts = dev.log_evidence_components_mfma()    # warm-up: builds the component plan
    out["plan_ms"] = (time.perf_counter() - t) * 1e3
    out["components"] = int(len(values))
    out["terms"] = int(cnt["factor_terms"] + cnt["variable_terms"])
    out["sum_gap_relative"] = float(abs(float(np.sum(values)) - total) / np.abs(values).sum())
    if counts != cnt or not np.isfinite(values).all():
        raise SystemExit(f"{name}: the component call and the total disagree: {counts} {cnt}")
    tot, comp = [], []
    for _ in range(calls):
        if not profile:
            dev.sync()
            t = time.perf_counter()
            dev.log_evidence_mfma()
            tot.append(time.perf_counter() - t)
        dev.sync()
        t = time.perf_counter()
        dev.log_evidence_components_mfma()
        comp.append(time.perf_counter() - t)
    out["log_evidence_components_mfma"] = _spread(comp)
    if not profile:
        out["log_evidence_mfma"] = _spread(tot)
        out["components_over_total"] = out["log_evidence_components_mfma"]["median_ms"] / out["log_evidence_mfma"]["median_ms"]
    dev.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--only", default="a16,a32,a64,b", help="comma-separated subset of a16,a32,a64,b")
    ap.add_argument("--profile", action="store_true", help="component calls alone after the warm-up (for a kernel trace)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import cortex.jl_amd as cx
    from cortex.jl_amd import _lib as L

    only = set(a.only.split(","))
    for d in (16, 32, 64):
        if f"a{d}" in only:
            run(cx, L, f"a{d}: lgssm_chain(10**5, d={d}), chain scan", cx.synth.lgssm_chain(10**5, d=d, seed=33), a.calls, a.profile)
    if "b" in only:
        first = cx.synth.lgssm_chain(100, d=16, seed=1)
        A, Q, R = first.meta["A"], first.meta["Q"], first.meta["R"]
        kinds = [first] + [cx.synth.lgssm_chain(100, d=16, seed=1 + i, A=A, Q=Q, R=R) for i in range(1, 16)]
        run(cx, L, "b: 1000 x lgssm_chain(100, d=16), chain scan", cx.synth.concat_models([kinds[i % 16] for i in range(1000)]), a.calls, a.profile)


if __name__ == "__main__":
    main()
