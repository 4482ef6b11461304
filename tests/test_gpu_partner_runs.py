"""-m gpu: the packed fused sweep with its partners read as wave-uniform runs (cx_partner_runs.h) against the per-lane 16-bit differences
(CX_PARTNER_RUNS=0) and the unpacked kernel (CX_PACK=0, read once per process: a child process).  The same values go to the same slots,
so every comparison is bit for bit on the float64 read-backs, NaN pattern included."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from tests.sweep_graphs import PARTNER_RUN_GRAPHS, read_back

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(name):
    build, sv = PARTNER_RUN_GRAPHS[name]
    model = build()
    dev = cx.DeviceGraph(schedule=L.SCHED_FUSED)
    cx.synth.load_into_device(model, dev, sv)
    dev.sweep(3)
    out = read_back(dev, model), dev.sweep_stats()
    dev.close()
    return out


@pytest.mark.parametrize("name", sorted(PARTNER_RUN_GRAPHS))
def test_runs_equal_per_lane_differences(hip_lib, monkeypatch, name):
    monkeypatch.delenv("CX_PARTNER_RUNS", raising=False)
    a, st = _run(name)
    monkeypatch.setenv("CX_PARTNER_RUNS", "0")
    b, _ = _run(name)
    for x, y, what in zip(a, b, ("messages to variables", "marginals")):
        assert np.array_equal(x, y, equal_nan=True), f"{name}: {what} differ between partner runs and per-lane differences"
    if name == "far_pair":
        assert st["partner_run_entries"] == 0, "partners beyond 16-bit differences: no table, the unpacked kernel"
    else:
        assert st["partner_run_entries"] > 0
    if name == "random600":
        assert st["partner_run_fallback"] > 0, st      # random partners: waves with three and more pieces take the per-lane path


def test_grid_equals_the_unpacked_kernel(hip_lib, monkeypatch, tmp_path):
    monkeypatch.delenv("CX_PARTNER_RUNS", raising=False)
    (msg, marg), _ = _run("grid20x37")
    code = ("import sys, numpy as np; sys.path.insert(0, %r)\n"
            "from tests.test_gpu_partner_runs import _run\n"
            "(m, g), _ = _run('grid20x37'); np.save(%r, m); np.save(%r, g)\n") % (ROOT, str(tmp_path / "m.npy"), str(tmp_path / "g.npy"))
    subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, CX_PACK="0"), timeout=120)
    assert np.array_equal(msg, np.load(tmp_path / "m.npy"), equal_nan=True)
    assert np.array_equal(marg, np.load(tmp_path / "g.npy"), equal_nan=True)
