"""-m gpu: cx_sweep(h, n) stores marginals in the LAST sweep of the call only (fused and flooding, dims 1 - 4; CX_MARG_EVERY_SWEEP=1: in
every sweep).  Nothing in the arithmetic changes, so every comparison here is bit for bit on the float64 read-backs, NaN pattern
included; only the parity check against the CPU checker uses the tolerance of tests/test_gpu_scalar_parity.py."""
import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from cortex.jl_amd import partition
from tests.helpers import assert_close, flood_oracle_from_model
from tests.sweep_graphs import grid_with_star, read_back
from tests.test_gpu_scalar_parity import RTOL

pytestmark = pytest.mark.gpu

CASES = {
    "grid20x37-fused": (lambda: cx.synth.gaussian_grid(20, 37, seed=7), L.SCHED_FUSED, 1e6),
    "grid20x37-flooding": (lambda: cx.synth.gaussian_grid(20, 37, seed=7), L.SCHED_FLOODING, 1e6),
    "lgssm300-d2-fused": (lambda: cx.synth.lgssm_chain(300, d=2, seed=3), L.SCHED_FUSED, 50.0),
    "lgssm300-d4-fused": (lambda: cx.synth.lgssm_chain(300, d=4, seed=3), L.SCHED_FUSED, 50.0),
}


def _device(model, schedule, seed_variance):
    dev = cx.DeviceGraph(schedule=schedule, dim=model.dim)
    cx.synth.load_into_device(model, dev, seed_variance)
    return dev


def _same(a, b, what):
    for x, y, name in zip(a, b, ("messages to variables", "marginals")):
        assert np.array_equal(x, y, equal_nan=True), f"{what}: {name} differ"


@pytest.mark.parametrize("every_sweep", [False, True])
@pytest.mark.parametrize("case", sorted(CASES))
def test_one_call_of_n_sweeps_equals_n_calls_of_one(hip_lib, monkeypatch, case, every_sweep):
    if every_sweep:
        monkeypatch.setenv("CX_MARG_EVERY_SWEEP", "1")
    else:
        monkeypatch.delenv("CX_MARG_EVERY_SWEEP", raising=False)
    build, schedule, sv = CASES[case]
    model = build()
    for n in (1, 2, 3, 7):      # odd and even: both parities of the double buffer
        a, b = _device(model, schedule, sv), _device(model, schedule, sv)
        a.sweep(n)
        for _ in range(n):
            b.sweep(1)
        _same(read_back(a, model), read_back(b, model), f"{case}: sweep({n}) against {n} x sweep(1)")
        assert a.stats()["sweeps_done"] == b.stats()["sweeps_done"] == n
        # the store IS skipped: every sweep of the one call but its last (none with the switch, none in calls of one sweep)
        assert a.sweep_stats()["sweeps_without_marginals"] == (0 if every_sweep else n - 1)
        assert b.sweep_stats()["sweeps_without_marginals"] == 0
        a.close(); b.close()


def test_sweep_of_zero_leaves_the_marginals(hip_lib):
    model = cx.synth.gaussian_grid(20, 37, seed=7)
    dev = _device(model, L.SCHED_FUSED, 1e6)
    dev.sweep(3)
    before = read_back(dev, model)
    dev.sweep(0)
    _same(read_back(dev, model), before, "sweep(0)")
    assert dev.stats()["sweeps_done"] == 3


@pytest.mark.parametrize("schedule", [L.SCHED_FUSED, L.SCHED_FLOODING])
def test_marginals_of_the_last_sweep_match_the_cpu_checker(hip_lib, schedule):
    """the marginals a sweep writes are those of the messages it read: after sweep(5), those of the checker's state after 4 sweeps"""
    model = cx.synth.gaussian_grid(20, 37, seed=7)
    dev = _device(model, schedule, 1e6)
    g = flood_oracle_from_model(model, seed_variance=1e6)
    dev.sweep(5)
    g.sweep(4)
    marg = dev.get_marginals(model.x_ids)
    m, v = g.marginals()
    assert_close(marg[:, 0], m, RTOL, "marginal mean after sweep(5)")
    assert_close(marg[:, 1], v, RTOL, "marginal variance after sweep(5)")


@pytest.mark.parametrize("schedule", [L.SCHED_FUSED, L.SCHED_FLOODING])
def test_high_degree_variable(hip_lib, schedule):
    """a variable of degree 17 (the wave-per-variable kernel writes its marginal): sweep(4) against four sweep(1)"""
    model = grid_with_star()
    a, b = _device(model, schedule, 1e6), _device(model, schedule, 1e6)
    assert a.stats()["n_big_variables"] == 1
    a.sweep(4)
    for _ in range(4):
        b.sweep(1)
    _same(read_back(a, model), read_back(b, model), "grid with a star: sweep(4) against 4 x sweep(1)")


def test_partitioned_handle_is_left_as_it_was(hip_lib, monkeypatch):
    """a handle with a state halo runs trimmed sweeps and keeps a marginal store in every one of them: the same with and without the switch"""
    part = partition.deep_self(12, 16, 2, seed=1)      # (the smallest the partition tests use: tests/test_gpu_halo_ipc.py)
    m = part.model

    def run():
        dev = cx.DeviceGraph(schedule=L.SCHED_FUSED)
        cx.synth.load_into_device(m, dev, seed_variance=1e6)
        partition.DeepHaloRccl(dev, part, overlap=False).sweep(11)
        assert dev.sweep_stats()["sweeps_without_marginals"] == 0
        return read_back(dev, m)
    monkeypatch.delenv("CX_MARG_EVERY_SWEEP", raising=False)
    a = run()
    monkeypatch.setenv("CX_MARG_EVERY_SWEEP", "1")
    b = run()
    _same(a, b, "deep halo, 11 sweeps")
