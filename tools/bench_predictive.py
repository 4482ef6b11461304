"""tools/bench_predictive.py — cost of one cx_predictive call next to cx_log_evidence on the same handle, measured in
the same run: a C2-size scalar chain and a C3-size d = 4 chain under the chain scan, and a 200 k-factor tree_model under the tree
schedule.  Both modes, with the rows and with out = NULL (total and counters only).  Median wall time of >= 30 synchronised calls after
a warm-up call (the first call of a (mode, ids) builds its rows), the bytes the passes must move, and that traffic per second against
8 TB/s.  Prints one JSON line per config.  Not the driver's bench (bench.py measures the C4 sweep)."""
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


def traffic(model, d: int, n_rows: int, n_inputs: int, n_excluded: int, rows: bool) -> int:
    """bytes one call must move at least: the variable pass (every message into a non-observed variable once, the per-variable tables,
    the scratch written) and per row its record (16 B), the factor's record and parameters, the datum, and per input the factor's own
    message, the scratch row and (causal) the list entry and message of every excluded slot; with the rows, d + d² + 2 doubles out
    (written on the device, then copied to the host: counted once)"""
    nt = d * (d + 1) // 2
    msg = 16 if d == 1 else 8 * (2 * ((d + nt + 1) // 2))
    row = 16 if d == 1 else 8 * (((d + nt + 1) + 1) // 2 * 2)
    obs = np.asarray(model.data_var)
    ev = np.asarray(model.edge_var)
    into_free = int((~np.isin(ev, obs)).sum()) if len(obs) else len(ev)
    nv = len(np.unique(ev))
    p1 = into_free * msg + nv * 13 + (nv - len(obs)) * row
    p2 = n_rows * (16 + 16 + (24 if d == 1 else 4) + msg) + n_inputs * (msg + row + 1) + n_excluded * (4 + msg) + (n_inputs * 8 if n_excluded else 0)
    return p1 + p2 + (n_rows * (d + d * d + 2) * 8 if rows else 0)


def row_counts(model, ids):
    """(inputs, slots the causal mode leaves out) of the rows `ids`, counted on the host from the model: what the plan's lists hold"""
    kinds = dict(zip(np.asarray(model.factor_ids).tolist(), np.asarray(model.factor_kind).tolist()))
    role = model.edge_role if model.edge_role is not None else np.zeros(len(model.edge_var), np.int32)
    is_row = np.isin(model.edge_fac, ids)
    obs = np.isin(model.edge_var, model.data_var)
    n_inputs = int((is_row & ~obs).sum())
    rule = np.array([kinds[int(f)] != L.FACTOR_OPAQUE for f in model.edge_fac])
    additive = np.array([kinds[int(f)] == L.FACTOR_GAUSS_ADDITIVE for f in model.edge_fac])
    order = np.lexsort((model.edge_var, model.edge_fac))
    second = np.zeros(len(order), bool)
    second[order[1:]] = np.asarray(model.edge_fac)[order[1:]] == np.asarray(model.edge_fac)[order[:-1]]      # the higher variable id of an additive factor
    is_in = rule & np.where(additive, second, role == L.ROLE_IN)
    n_in_of_var = np.bincount(np.asarray(model.edge_var)[is_in], minlength=int(np.max(model.edge_var)) + 1)
    inp = is_row & ~obs
    n_excluded = int((n_in_of_var[np.asarray(model.edge_var)[inp]] - is_in[inp]).sum())
    return n_inputs, n_excluded


def median_ms(fn, dev, calls: int) -> float:
    fn()                                         # warm-up: builds the rows
    ts = []
    for _ in range(calls):
        dev.sync()
        t = time.perf_counter()
        fn()                                     # synchronous: the result is on the host at return
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e3


def run(name, model, schedule, calls, workload):
    d = model.dim
    dev = cx.DeviceGraph(dim=d, schedule=schedule)
    cx.synth.load_into_device(model, dev)
    dev.sweep(1)
    dev.sync()
    ids = dev.predictive_rows()
    n_inputs, n_excluded = row_counts(model, ids)
    ms_ev = median_ms(dev.log_evidence, dev, calls)
    out = {"config": name, "workload": workload, "calls": calls, "rows": int(len(ids)), "ms_log_evidence": ms_ev}
    for mode, nx in (("loo", 0), ("causal", n_excluded)):
        for rows in (True, False):
            ms = median_ms(lambda: dev.predictive(mode, rows=rows), dev, calls)
            b = traffic(model, d, len(ids), n_inputs, nx, rows)
            key = mode + ("" if rows else "_total_only")
            out[key] = {"ms": ms, "bytes": b, "fraction_of_8TBps": b / (ms * 1e-3) / HBM, "over_evidence": ms / ms_ev}
        res = dev.predictive(mode, rows=False)
        out[mode]["total"], out[mode]["counts"] = res["total"], res["counts"]
    dev.close()
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--only", default="", help="comma-separated subset of C2,C3,tree")
    a = ap.parse_args()
    only = set(a.only.split(",")) if a.only else {"C2", "C3", "tree"}
    if "C2" in only:
        m = cx.synth.ssm_chain(250_001)
        run("C2", m, L.SCHED_CHAIN_SCAN, a.calls, f"scalar chain T=250001 ({len(m.edge_var)} edges) after one chain-scan sweep")
    if "C3" in only:
        m = cx.synth.lgssm_chain(1_000_000, d=4)
        run("C3", m, L.SCHED_CHAIN_SCAN, a.calls, f"d=4 chain T=1000000 ({len(m.edge_var)} edges) after one chain-scan sweep")
    if "tree" in only:
        m = cx.synth.tree_model(200_000, shape="deep", observe=0.2)
        run("tree", m, L.SCHED_TREE, a.calls, f"tree_model(200000, deep, observe 0.2) ({len(m.edge_var)} edges) after one tree sweep")


if __name__ == "__main__":
    main()
