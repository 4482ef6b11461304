"""-m gpu: bench.py end to end on a small grid.  A plain run prints the contract's keys and nothing measured beside them;
--dump-outputs writes the same float64 arrays in two runs with the same arguments, and they are what W + K sweeps of the
same grid leave in a device handle driven directly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, steps, warmup, grid):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--grid", str(grid), "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plain_run_prints_the_contract_and_dumps_what_the_timed_sweeps_computed(hip_lib, tmp_path):
    import cortex.jl_amd as cx
    from cortex.jl_amd import _lib as L

    steps, warmup, grid = 7, 3, 64
    lines = [_bench(tmp_path / d, steps, warmup, grid) for d in ("a", "b")]
    for line in lines:
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in line, k
        assert line["steps"] == steps and line["warmup"] == warmup and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["details"] is None and "roofline" not in line and "cpu_baseline" not in line and "parity" not in line
    arrays = {}
    for name in ("marginals", "messages_to_variable"):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float64 and a.shape[1] == 2 and np.array_equal(a, b, equal_nan=True), name
        arrays[name] = a

    model = cx.synth.gaussian_grid(grid, grid, seed=1234)
    dev = cx.DeviceGraph(device=0, schedule=L.SCHED_FUSED, marginals_in_sweep=True)
    try:
        cx.synth.load_into_device(model, dev, seed_variance=1e6)
        dev.sweep(warmup + steps)
        assert np.array_equal(arrays["marginals"], dev.get_marginals(model.x_ids))
        assert np.array_equal(arrays["messages_to_variable"], dev.get_messages(model.edge_var, model.edge_fac, L.TO_VARIABLE))
    finally:
        dev.close()
