"""-m gpu: a buffer that a captured HIP graph names moves AFTER the graph was captured and replayed ("ownership":
cxh::captured_graphs_drop).  One case per site that moves such a buffer: the rule tables of dim > 1 (cx_set_factor_matrices with one
more parameter set: d_ptab, and d_ptab_bt at a matrix-core dim), the A | Q table of factors with more than two edges (d_kary_aq), the
product and joint stores of the batched API at dim 1 (grow_store) and the product table at dim > 1 (mv_ensure_prod_store).

Each case runs twice, each time in a process of its own (the switches are read once per process): with captured graphs, and with
CX_TREE_GRAPH=0 CX_REF_GRAPH=0, i.e. plain launches.  Plain launches run the same kernels with the same arguments in the same order,
so the marginals are required to be bit-identical, before and after the move."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case_ptab(d, n, b):
    """tree schedule: two sweeps (captured, replayed), one more parameter set than the tables hold and new matrices for set 0, a sweep"""
    from tests.test_gpu_mv import _branching_lgssm

    model, _mean, _cov = _branching_lgssm(n, d, seed=31, b=b, solve=False)
    dev = cx.DeviceGraph(dim=d, schedule=L.SCHED_TREE)
    cx.synth.load_into_device(model, dev)
    dev.sweep(2)
    before = dev.get_marginals(model.x_ids)
    A_new = 0.7 * np.linalg.qr(np.random.default_rng(7).standard_normal((d, d)))[0]
    dev.set_factor_matrices(len(model.psets), np.eye(d), np.eye(d))      # the tables move
    dev.set_factor_matrices(0, A_new, 0.5 * np.eye(d))
    dev.sweep(1)
    after = dev.get_marginals(model.x_ids)
    dev.sweep(1)                                                         # (the graph captured over the new tables, replayed)
    again = dev.get_marginals(model.x_ids)
    dev.close()
    assert np.max(np.abs(after - before)) > 1e-3 and np.array_equal(after, again)
    return {"before": before, "after": after}


def _case_kary_aq():
    """tree schedule, factors of three and four d-dimensional variables: the same, for the A | Q table their rule reads"""
    from tests.test_gpu_kary_mv import _kary_tree, _load

    d = 4
    model, prior, facs, fid, sets, _mean, _cov = _kary_tree(12, d, seed=3)
    dev = _load(model, prior, facs, fid, sets, L.SCHED_TREE)
    dev.sweep(2)
    assert dev.tree_plan_stats()["kary_entries"] > 0
    before = dev.get_marginals(model.x_ids)
    dev.set_factor_matrices(len(sets), np.eye(d), np.eye(d))             # one more set: the A | Q table (and the rule tables) move
    dev.set_factor_matrices(0, 0.5 * sets[0][0], 2.0 * sets[0][1])
    dev.sweep(1)
    after = dev.get_marginals(model.x_ids)
    dev.sweep(1)
    again = dev.get_marginals(model.x_ids)
    dev.close()
    assert np.max(np.abs(after - before)) > 1e-6 and np.array_equal(after, again)
    return {"before": before, "after": after}


def _replayed_calls(dev, call):
    """the steady state of an iteration under CX_SCHED_REFERENCE: the same plan hit again and again, of more than one launch (the
    launches of such a plan are what a graph captures)"""
    out = [call() for _ in range(4)][-1]
    st = dev.ref_plan_stats()
    assert st["hits"] >= 2 and st["launches"] > 1, st
    return out, st["hits"]


def _case_ref_stores_dim1():
    """reference order, dim 1, a random tree of 20,000 pairwise factors (variables of degree > 5: their segment-tree nodes live in the
    product store, which the plan's launches name): 300 more ProductOfMessages nodes and 300 more JointMarginal nodes than the stores
    hold are registered by cx_update_batch, on signals the wiring does not know, so that the next call replays the SAME plan"""
    model = cx.synth.tree_model(20_000, seed=5, k_choices=(1,), observe=0.25)
    dev = cx.DeviceGraph(schedule=L.SCHED_REFERENCE)
    cx.synth.load_into_device(model, dev)

    def call():
        dev.set_messages(model.data_var, model.data_fac, L.TO_FACTOR, L.FORM_POINT, model.data_y)
        dev.set_messages(model.prior_var, model.prior_fac, L.TO_VARIABLE, L.FORM_MOMENT, np.stack([model.prior_mean, model.prior_variance], axis=1))
        dev.sweep(1)
        return dev.get_marginals(model.x_ids)

    deg = np.bincount(model.edge_var)
    assert deg.max() > 5, "the test needs segment-tree nodes in the product store"
    thin = [int(v) for v in model.x_ids if deg[v] == 2][:300]             # (degree <= 5: no segment tree, ProductOfMessages(v, 1:2) is no signal of the wiring)
    pair = [int(f) for f in model.meta["kary_ids"][:310]]
    assert len(thin) == 300
    dev.update_batch([L.ITEM_JOINT_MARGINAL] * 10, [0] * 10, pair[:10])  # the joint store exists (256 records) before the plan is captured
    before, hits = _replayed_calls(dev, call)
    dev.update_batch([L.ITEM_PRODUCT_OF_MESSAGES] * 300, thin, [L.item_range(1, 2)] * 300)      # the product store moves
    dev.update_batch([L.ITEM_JOINT_MARGINAL] * 300, [0] * 300, pair[10:])                         # the joint store moves
    after = call()
    assert dev.ref_plan_stats()["hits"] == hits + 1, "the same plan, replayed over the moved stores"
    prods = dev.get_products(thin, [1] * 300, [2] * 300)
    jm, jc = dev.get_joint_marginals(pair)
    dev.close()
    assert not np.any(np.isnan(prods)) and not np.any(np.isnan(before))
    return {"before": before, "after": after, "products": prods, "joint_mean": np.asarray(jm), "joint_cov": np.asarray(jc)}


def _case_ref_prod_dim3():
    """reference order, dim 3, a tree with five children per node (degree 7: segment-tree nodes in the product table): 300 more
    ProductOfMessages nodes, on leaves, than the table holds"""
    from tests.test_gpu_mv import _branching_lgssm

    d, n = 3, 8000
    model, _mean, _cov = _branching_lgssm(n, d, seed=9, b=5, solve=False)
    dev = cx.DeviceGraph(dim=d, schedule=L.SCHED_REFERENCE)
    cx.synth.load_into_device(model, dev)

    def call():
        dev.set_messages(model.data_var, model.data_fac, L.TO_FACTOR, L.FORM_POINT, model.data_y)
        dev.sweep(1)
        return dev.get_marginals(model.x_ids)

    before, hits = _replayed_calls(dev, call)
    leaves = [int(v) for v in model.x_ids[-300:]]                         # (degree 2: parent and likelihood)
    dev.update_batch([L.ITEM_PRODUCT_OF_MESSAGES] * 300, leaves, [L.item_range(1, 2)] * 300)
    after = call()
    assert dev.ref_plan_stats()["hits"] == hits + 1, "the same plan, replayed over the moved table"
    prods = dev.get_products(leaves, [1] * 300, [2] * 300, L.FORM_NATURAL)
    dev.close()
    assert not np.any(np.isnan(prods)) and not np.any(np.isnan(before))
    return {"before": before, "after": after, "products": prods}


CASES = {
    "ptab-dim3": lambda: _case_ptab(3, 40, 3),
    "ptab-dim16": lambda: _case_ptab(16, 9, 2),
    "kary-aq-dim4": _case_kary_aq,
    "ref-stores-dim1": _case_ref_stores_dim1,
    "ref-prod-dim3": _case_ref_prod_dim3,
}


def _run(case, path, graphs):
    env = dict(os.environ, CX_REF_CLUSTER="0")      # (a wide and deep plan would otherwise run on the cluster, which captures nothing)
    for name in ("CX_TREE_GRAPH", "CX_REF_GRAPH"):
        env.pop(name, None)
        if not graphs:
            env[name] = "0"
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_captured_graphs", case, path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(path)


@pytest.mark.parametrize("case", sorted(CASES))
def test_marginals_after_a_named_buffer_moved_equal_plain_launches_bit_for_bit(hip_lib, tmp_path, case):
    captured = _run(case, str(tmp_path / "captured.npz"), graphs=True)
    plain = _run(case, str(tmp_path / "plain.npz"), graphs=False)
    assert sorted(captured.files) == sorted(plain.files)
    assert not np.any(np.isnan(captured["after"]))
    for name in captured.files:
        assert np.array_equal(captured[name], plain[name], equal_nan=True), (case, name, np.nanmax(np.abs(captured[name] - plain[name])))


if __name__ == "__main__":
    np.savez(sys.argv[2], **CASES[sys.argv[1]]())
