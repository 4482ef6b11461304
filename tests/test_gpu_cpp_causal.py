"""-m gpu: cortex::Handle::causal_marginals of include/cortex_hip.hpp (g++ + the C ABI, nothing else) on a scalar SSM chain, against
DeviceGraph.causal_marginals on the same model and the reverse-time Kalman filter (tests/cpp/causal_demo.cpp)."""

import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from tests import missing_data as MD
from tests import predictive_support as P
from tests.gpu_support import run_demo

pytestmark = pytest.mark.gpu


def test_cpp_host_class_causal_marginals(hip_lib, tmp_path):
    out_lines = run_demo("causal_demo", tmp_path)
    lines = [line.split() for line in out_lines]
    T = 50
    model = cx.synth.ssm_chain(T, seed=1)
    model.data_y = np.array([0.5 * t + (7 * t) % 5 for t in range(1, T + 1)], dtype=np.float64)
    dev = cx.DeviceGraph(schedule=L.SCHED_CHAIN_SCAN)
    cx.synth.load_into_device(model, dev)
    dev.sweep(1)
    for name, mode, lag in (("predicted", "predicted", 0), ("filtered", "filtered", 0), ("lag5", "filtered", 5)):
        want = dev.causal_marginals(mode, lag, model.x_ids)
        rows = np.array([[float(v) for v in l[2:]] for l in lines if l[0] == name], dtype=np.float64)
        assert [int(l[1]) for l in lines if l[0] == name] == list(model.x_ids)
        assert P.scaled_err(rows[:, :1], want["mean"]) <= 1e-12 and P.scaled_err(rows[:, 1:].reshape(T, 1, 1), want["cov"]) <= 1e-12
        cnt = [l for l in lines if l[0] == name + "_counts"][0]
        assert [int(v) for v in cnt[1:]] == list(want["counts"].values())
    # additive transitions: the causal order runs backwards in time (the lower id is `out`) — the filter of the reversed series
    s = MD.chain_spec(model)
    r = MD.kalman_filter(s["A"][::-1], s["b"][::-1], s["Q"][::-1], s["H"], s["R"][::-1], s["y"][::-1], s["keep"][::-1])
    flt = dev.causal_marginals("filtered", 0, model.x_ids)
    assert P.scaled_err(flt["mean"], r["mf"][::-1]) <= 1e-9 and P.scaled_err(flt["cov"], r["Pf"][::-1]) <= 1e-9
    dev.close()
