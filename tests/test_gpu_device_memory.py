"""-m gpu: device memory over the life of handles ("ownership"): whatever a handle allocates, cx_destroy gives back, and
stats()["device_bytes"] is the sum of what is live.

What is NOT reached from here: cxh::dev_free_all on a cx_graph_create that failed halfway (cx_graph_create refuses a handle that has a
graph, so that is the only other caller besides cx_destroy).  Reaching it needs a forced allocation failure; that path is checked by
reading (dev_free_all assigns a default-constructed device state: a buffer has no second mention to forget)."""
import os

import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L

pytestmark = pytest.mark.gpu

SCHEDULES = (L.SCHED_FUSED, L.SCHED_CHAIN_SCAN, L.SCHED_TREE)


def _model(dim):
    return cx.synth.ssm_chain(200_000, seed=11) if dim == 1 else cx.synth.lgssm_chain(40_000, d=4, seed=14)


def _statistics(dev, model):
    if model.dim > 1:
        return dev.factor_statistics(n_groups=2)                             # one group per parameter set
    fids = np.asarray(model.factor_ids)[np.asarray(model.factor_kind) != L.FACTOR_OPAQUE]
    return dev.factor_statistics(fids, np.arange(len(fids)) % 7, n_groups=7)


def _handle_life(model, schedule):
    """create, sweep, evidence, statistics, samples of two sizes (the per-call scratch grows once), destroy; the peak device_bytes"""
    dev = cx.DeviceGraph(dim=model.dim, schedule=schedule)
    cx.synth.load_into_device(model, dev, seed_variance=1e6 if schedule == L.SCHED_FUSED else None)
    dev.sweep(2)
    dev.log_evidence()
    _statistics(dev, model)
    dev.sample_posterior(2, seed=1)
    dev.sample_posterior(5, seed=2)
    dev.sync()
    peak = dev.stats()["device_bytes"]
    dev.close()
    return peak


def _vram_in_use():
    """(bytes of device memory in use, which figure): this process's own where the driver shows one, the device's otherwise"""
    import torch

    path = f"/sys/class/kfd/kfd/proc/{os.getpid()}"
    try:
        files = sorted(f for f in os.listdir(path) if f.startswith("vram_"))
        if files:
            return sum(int(open(os.path.join(path, f)).read()) for f in files), "kfd per-process vram_*"
    except (OSError, ValueError):
        pass
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    return total - free, "torch.cuda.mem_get_info (device-wide)"


def test_destroy_gives_back_what_a_handle_allocated(hip_lib):
    """12 cycles of (a handle per schedule and dim, each destroyed before the next is made); memory in use after cycle 12 exceeds that
    after cycle 2 by less than ONE cycle's peak device_bytes (the largest single handle's): a handle that kept a tenth of what it
    allocates would exceed that over ten cycles of six handles, allocator granularity is far below it"""
    models = [_model(1), _model(4)]
    peak = 0
    used = {}
    for cycle in range(1, 13):
        for model in models:
            for s in SCHEDULES:
                p = _handle_life(model, s)
                assert p >= 10 << 20, (model.dim, s, p)                       # (a model of tens of MB: the bound below means something)
                peak = max(peak, p)
        if cycle in (2, 12):
            used[cycle], source = _vram_in_use()
    grown = used[12] - used[2]
    print(f"device memory in use after cycle 2: {used[2]}, after cycle 12: {used[12]} (grown {grown}); one handle's peak device_bytes {peak}; read from {source}")
    assert grown < peak, (used, peak, source)


@pytest.mark.parametrize("dim", [1, 4])
def test_sample_scratch_is_counted_once(hip_lib, dim):
    """the per-call scratch of cx_sample_posterior only grows, and device_bytes follows it: S = 4, 64, 4 ends where S = 64 left it"""
    model = _model(dim)
    dev = cx.DeviceGraph(dim=dim, schedule=L.SCHED_TREE)
    cx.synth.load_into_device(model, dev)
    dev.sweep(1)
    b0 = dev.stats()["device_bytes"]
    dev.sample_posterior(4, seed=1)
    b4 = dev.stats()["device_bytes"]
    dev.sample_posterior(64, seed=1)
    b64 = dev.stats()["device_bytes"]
    dev.sample_posterior(4, seed=1)
    b4_again = dev.stats()["device_bytes"]
    dev.sample_posterior(64, seed=3)
    print(f"dim {dim}: device_bytes {b0} -> S=4 {b4} -> S=64 {b64} -> S=4 {b4_again} -> S=64 {dev.stats()['device_bytes']}")
    assert b0 < b4 < b64
    assert b4_again == b64
    assert dev.stats()["device_bytes"] == b64
    dev.close()
