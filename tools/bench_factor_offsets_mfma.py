"""tools/bench_factor_offsets_mfma.py — what a handle with factor offsets at the matrix-core dims pays (cx_set_factor_offsets_mfma, DESIGN.md
§4u): ms per fused sweep and per chain-scan sweep on lgssm_chain(10**5, d), d = 16 / 32 / 64, for a handle that never called the function,
one whose offsets are all zero and one with a random offset on every factor, in one process.  A host clock around one sweep and a
synchronise, after warm-up sweeps; medians and the spread (min, max) of --sweeps sweeps each, the three handles interleaved.  Also the
evidence and the statistics call on the chain-scan handles.  Prints one JSON line per dim and schedule.  --plain: the handle without
offsets alone (what runs on a library that has no such function: the parent of a comparison).  Not the driver's bench (bench.py measures
the C4 sweep)."""
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


def _timed(call, dev):
    dev.sync()
    t = time.perf_counter()
    call()
    dev.sync()
    return time.perf_counter() - t


def run(cx, L, d, T, schedule, name, sweeps, plain):
    model = cx.synth.lgssm_chain(T, d=d, seed=5)
    ids = np.asarray(model.factor_ids)[np.asarray(model.factor_kind) == L.FACTOR_GAUSS_LINEAR]
    handles = {}
    for kind in ("none",) if plain else ("none", "zero", "random"):
        dev = cx.DeviceGraph(dim=d, schedule=schedule)
        cx.synth.load_into_device(model, dev, seed_variance=1e6 if schedule == L.SCHED_FUSED else None)
        if kind == "zero":
            dev.set_factor_offsets_mfma(ids, np.zeros((len(ids), d)))
        if kind == "random":
            dev.set_factor_offsets_mfma(ids, 0.1 * np.random.default_rng(1).standard_normal((len(ids), d)))
        dev.sweep(3)
        handles[kind] = dev
    out = {"d": d, "T": T, "schedule": name, "sweeps": sweeps, "factors_with_offsets": int(len(ids))}
    ts = {k: [] for k in handles}
    for _ in range(sweeps):
        for k, dev in handles.items():
            ts[k].append(_timed(lambda: dev.sweep(1), dev))
    for k in handles:
        out["sweep_" + k] = _spread(ts[k])
    if not plain:
        out["random_over_none"] = out["sweep_random"]["median_ms"] / out["sweep_none"]["median_ms"]
        if schedule == L.SCHED_CHAIN_SCAN:      # exact messages: the readers
            for call_name, call in (("log_evidence_mfma", lambda h: h.log_evidence_mfma()), ("factor_statistics_mfma", lambda h: h.factor_statistics_mfma(n_groups=2))):
                for k in ("none", "random"):
                    call(handles[k])      # warm-up: the caches
                    out[f"{call_name}_{k}"] = _spread([_timed(lambda: call(handles[k]), handles[k]) for _ in range(5)])
    for dev in handles.values():
        dev.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=20)
    ap.add_argument("--T", type=int, default=10**5)
    ap.add_argument("--dims", default="16,32,64")
    ap.add_argument("--plain", action="store_true", help="the handle without offsets alone")
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import cortex.jl_amd as cx
    from cortex.jl_amd import _lib as L

    for d in (int(x) for x in a.dims.split(",")):
        run(cx, L, d, a.T, L.SCHED_FUSED, "fused", a.sweeps, a.plain)
        run(cx, L, d, a.T, L.SCHED_CHAIN_SCAN, "chain-scan", a.sweeps, a.plain)


if __name__ == "__main__":
    main()
