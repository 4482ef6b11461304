"""lab: two to six sweeps per launch (cx_sweep_pair.hip, cx_sweep_deep.hip) on one grid, regions of every form alternating in one
process, and every form's results compared bit for bit with a handle that swept the same number of sweeps under CX_SWEEP_PAIRS=0.
The levers are environment variables: CX_SWEEP_DEPTH (read per call), CX_DEEP_ROWS / CX_PAIR_ROWS (rows per segment, read when the handle's
geometry is chosen: one handle per setting).
python tools/lab/deep_sweep_ab.py [N] [sweeps per region] [regions] [depth:rows,depth:rows,...]   (rows 0: chosen by occupancy)"""
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
FORMS = [tuple(int(x) for x in f.split(":")) for f in (sys.argv[4] if len(sys.argv) > 4 else "2:0,3:0,4:0").split(",")]

model = cx.synth.gaussian_grid(N, N, seed=1234)


def device(rows, depth):
    """a handle whose first region (where its geometry is chosen) has run under this rows setting"""
    for name in ("CX_DEEP_ROWS", "CX_PAIR_ROWS"):
        if rows:
            os.environ[name] = str(rows)
        else:
            os.environ.pop(name, None)
    dev = cx.DeviceGraph(schedule=L.SCHED_FUSED)
    cx.synth.load_into_device(model, dev, 1e6)
    region(dev, depth)
    return dev


def region(dev, depth):
    os.environ["CX_SWEEP_PAIRS"] = "1" if depth else "0"
    os.environ["CX_SWEEP_DEPTH"] = str(depth or 2)
    dev.sync()
    t0 = time.perf_counter()
    dev.sweep(K)
    dev.sync()
    return (time.perf_counter() - t0) / K * 1e6


plain = device(0, 0)
devs = [device(rows, depth) for depth, rows in FORMS]
times = [[] for _ in FORMS]
plain_t = []
for _ in range(REGIONS):
    for i, ((depth, _), dev) in enumerate(zip(FORMS, devs)):
        times[i].append(region(dev, depth))
    plain_t.append(region(plain, 0))
want = plain.get_marginals(model.x_ids)
sample = np.arange(0, len(model.edge_var), 97)
want_msg = plain.get_messages(model.edge_var[sample], model.edge_fac[sample], L.TO_VARIABLE, L.FORM_NATURAL)
print(f"N = {N}, {K} sweeps per region, {REGIONS} regions; plain {sorted(plain_t)[len(plain_t) // 2]:.2f} us per sweep ({min(plain_t):.2f} - {max(plain_t):.2f})", flush=True)
for (depth, rows), dev, t in zip(FORMS, devs, times):
    same = np.array_equal(dev.get_marginals(model.x_ids), want, equal_nan=True)
    same_msg = np.array_equal(dev.get_messages(model.edge_var[sample], model.edge_fac[sample], L.TO_VARIABLE, L.FORM_NATURAL), want_msg, equal_nan=True)
    st = dev.sweep_deep_stats()
    print(f"depth {depth}, rows per segment {st['rows']}{'' if rows else ' (by occupancy)'}: {sorted(t)[len(t) // 2]:.2f} us per sweep ({min(t):.2f} - {max(t):.2f}); "
          f"launches of 2 / 3 / 4 / 5 / 6 sweeps {' / '.join(str(x) for x in dev.sweep_deep_launches()[2:])}; "
          f"marginals identical: {same}, sampled messages identical: {same_msg}", flush=True)
