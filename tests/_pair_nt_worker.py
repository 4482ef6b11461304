"""The child of tests/test_gpu_grid_between_calls.py::test_nontemporal_stores_in_a_process_of_their_own: CX_PAIR_NT is read once per
process, so the nontemporal stores of the paired sweep get a process of their own.  Sweeps a seeded grid n times in one call and dumps the
read-backs for the parent to compare."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    rows, cols, n, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    import numpy as np

    import cortex.jl_amd as cx
    from cortex.jl_amd import _lib as L
    from tests.sweep_graphs import read_back

    model = cx.synth.gaussian_grid(rows, cols, seed=7)
    dev = cx.DeviceGraph(schedule=L.SCHED_FUSED)
    cx.synth.load_into_device(model, dev, seed_variance=1e6)
    dev.sweep(n)
    f2v, marg = read_back(dev, model)
    v2f = dev.get_messages(model.edge_var, model.edge_fac, L.TO_FACTOR, L.FORM_NATURAL)
    info = {"nt": os.environ.get("CX_PAIR_NT"), "paired_launches": dev.sweep_stats()["paired_launches"], "sweeps_done": dev.stats()["sweeps_done"]}
    dev.close()
    np.savez(out, f2v=f2v, marg=marg, v2f=v2f, info=json.dumps(info))


if __name__ == "__main__":
    main()
