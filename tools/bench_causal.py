"""tools/bench_causal.py — cost of one cx_causal_marginals call next to cx_log_evidence and cx_predictive(rows=False), the
other readers of the same messages, on the same handle in the same run: a C2-size scalar chain and a C3-size d = 4 chain under the chain
scan.  The three modes for every variable: predicted, filtered, filtered with lag 8.  Per mode the median wall time of synchronised
calls after a warm-up call (the first call builds the plan) — end to end, the copy of the n x (d + d²) rows to the host included — and
of the same call for ONE row: the split and lag passes run whatever rows are asked for, so that is the device side of the passes over
the graph plus one launch sequence and one synchronisation, without the row pass over n rows and their copy.  Prints one JSON line per
config.  Not the driver's bench (bench.py measures the C4 sweep)."""
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


def traffic(model, d: int, lag: int) -> dict:
    """bytes one call must move at least: split (every message into a non-observed variable that is not of class T once, a class byte per
    slot, the scratch written), each lag pass (per transition its record, one scratch row, the class bytes and table entries of the
    successor's slots, one β read and one written), the row pass (the scratch rows, β of the T slots, d + d² doubles out) and the copy"""
    nt = d * (d + 1) // 2
    nc = d + nt
    msg = 16 if d == 1 else 8 * (2 * ((nc + 1) // 2))
    obs = np.asarray(model.data_var)
    ev = np.asarray(model.edge_var)
    nv = len(np.unique(ev))
    free = nv - len(obs)
    into_free = int((~np.isin(ev, obs)).sum())
    n_t = free - 1                               # a chain: one transition onward per state but the last
    split = (into_free - n_t) * msg + into_free + free * 2 * nc * 8
    back = n_t * (16 + nc * 8 + 3 * 5 + 2 * nc * 8)
    out = free * 2 * nc * 8 + (n_t * (nc * 8 + 5) if lag else 0) + nv * (d + d * d) * 8
    return {"split": split, "back_per_lag": back, "out": out, "host_copy": nv * (d + d * d) * 8, "total": split + lag * back + out}


def median_ms(fn, dev, calls: int) -> float:
    fn()                                         # warm-up: builds the plan
    ts = []
    for _ in range(calls):
        dev.sync()
        t = time.perf_counter()
        fn()                                     # synchronous: the result is on the host at return
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e3


def run(name, model, calls, workload):
    d = model.dim
    dev = cx.DeviceGraph(dim=d, schedule=L.SCHED_CHAIN_SCAN)
    cx.synth.load_into_device(model, dev)
    dev.sweep(1)
    dev.sync()
    nv = dev.stats()["n_variables"]
    out = {"config": name, "workload": workload, "calls": calls, "rows": int(nv),
           "ms_log_evidence": median_ms(dev.log_evidence, dev, calls),
           "ms_predictive_causal_total_only": median_ms(lambda: dev.predictive("causal", rows=False), dev, calls)}
    one = np.asarray(model.x_ids[:1])
    for key, mode, lag in (("predicted", "predicted", 0), ("filtered", "filtered", 0), ("filtered_lag8", "filtered", 8)):
        ms = median_ms(lambda: dev.causal_marginals(mode, lag), dev, calls)
        ms_one = median_ms(lambda: dev.causal_marginals(mode, lag, one), dev, calls)      # the passes over the graph, one row out
        b = traffic(model, d, lag)
        res = dev.causal_marginals(mode, lag)
        out[key] = {"ms_end_to_end": ms, "ms_one_row": ms_one, "bytes": b, "fraction_of_8TBps_one_row": (b["total"] - b["out"]) / (ms_one * 1e-3) / HBM,
                    "over_evidence": ms / out["ms_log_evidence"], "one_row_over_evidence": ms_one / out["ms_log_evidence"], "counts": res["counts"]}
    dev.close()
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--only", default="", help="comma-separated subset of C2,C3")
    a = ap.parse_args()
    only = set(a.only.split(",")) if a.only else {"C2", "C3"}
    if "C2" in only:
        m = cx.synth.ssm_chain(250_001)
        run("C2", m, a.calls, f"scalar chain T=250001 ({len(m.edge_var)} edges) after one chain-scan sweep")
    if "C3" in only:
        m = cx.synth.lgssm_chain(1_000_000, d=4)
        run("C3", m, a.calls, f"d=4 chain T=1000000 ({len(m.edge_var)} edges) after one chain-scan sweep")


if __name__ == "__main__":
    main()
