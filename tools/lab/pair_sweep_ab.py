"""lab: the paired sweep (cx_sweep_pair.hip) against plain sweeps on one grid, interleaved in one process, and the two forms' results compared
bit for bit.  The levers are environment variables read when the handle first pairs: CX_PAIR_ROWS (rows per segment), CX_PAIR_NT=1
(nontemporal stores).
python tools/lab/pair_sweep_ab.py [N] [sweeps per region] [regions] [rows,rows,...]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import cortex.jl_amd as cx  # noqa: E402
from cortex.jl_amd import _lib as L  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1415
K = int(sys.argv[2]) if len(sys.argv) > 2 else 201
REGIONS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
ROWS = [r for r in (sys.argv[4].split(",") if len(sys.argv) > 4 else [""])]

model = cx.synth.gaussian_grid(N, N, seed=1234)


def device(rows):
    if rows:
        os.environ["CX_PAIR_ROWS"] = rows
    else:
        os.environ.pop("CX_PAIR_ROWS", None)
    dev = cx.DeviceGraph(schedule=L.SCHED_FUSED)
    cx.synth.load_into_device(model, dev, 1e6)
    return dev


def region(dev, pairs):
    os.environ["CX_SWEEP_PAIRS"] = "1" if pairs else "0"
    dev.sync()
    t0 = time.perf_counter()
    dev.sweep(K)
    dev.sync()
    return (time.perf_counter() - t0) / K * 1e6


for rows in ROWS:
    plain = device("")
    region(plain, False)
    dev = device(rows)
    region(dev, True)
    a, b = [], []
    for _ in range(REGIONS):
        a.append(region(dev, True))
        b.append(region(plain, False))
    same = np.array_equal(dev.get_marginals(model.x_ids), plain.get_marginals(model.x_ids), equal_nan=True)
    sample = np.arange(0, len(model.edge_var), 97)
    same_msg = np.array_equal(dev.get_messages(model.edge_var[sample], model.edge_fac[sample], L.TO_VARIABLE, L.FORM_NATURAL),
                              plain.get_messages(model.edge_var[sample], model.edge_fac[sample], L.TO_VARIABLE, L.FORM_NATURAL), equal_nan=True)
    print(f"N = {N}, rows per segment {rows or 'by occupancy'}, nontemporal stores {os.environ.get('CX_PAIR_NT', '0')}: paired {sorted(a)[len(a) // 2]:.2f} us per sweep "
          f"({min(a):.2f} - {max(a):.2f}), plain {sorted(b)[len(b) // 2]:.2f} ({min(b):.2f} - {max(b):.2f}); paired launches {dev.sweep_stats()['paired_launches']}; "
          f"marginals identical: {same}, sampled messages identical: {same_msg}", flush=True)
    dev.close()
    plain.close()
