"""CPU: the helpers of tests/components_support.py that the per-component log-evidence GPU tests rely on, and the product's host
labelling (cx_components.h through cx_hostlogic.cpp's cxh_flat_components) against them."""
import ctypes as C
import os
import subprocess

import numpy as np

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from tests import components_support as CS
from tests import evidence_support as E
from tests import hostlogic as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_labels(model):
    """(var_ids, label per variable, label per factor id ascending, C) from the product's host logic"""
    g = H.FlatGraph(model.edge_var, model.edge_fac, model.factor_ids, model.factor_kind, model.factor_var, edge_role=model.edge_role, dim=model.dim,
                    schedule=L.SCHED_TREE)
    assert g.status == 0, g.error
    fn = g.L.cxh_flat_components            # (the named entry is bound here: tests/hostlogic.py binds the numbered ones)
    fn.restype = C.c_int64
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    vl, fl = np.full(g.scalar("nv"), -7, np.int64), np.full(g.scalar("nf"), -7, np.int64)
    n = int(fn(g.p, vl.ctypes.data, fl.ctypes.data))
    assert int(fn(g.p, None, None)) == n
    return g.arr("var_ids"), vl, fl, n


def _chain(T, q=1.0):
    return cx.synth.ssm_chain(T, seed=3, q=q)


def test_labels_on_three_tiny_graphs_by_hand():
    # two chains of 2 and 3 states: ids 1..2 states, 3..4 data (+ shift 7 for the second: states 8..10, data 11..13)
    two = CS.join_scalar([_chain(2), _chain(3)])
    ids, lab, n = CS.labels(two)
    assert n == 2 and list(ids) == [1, 2, 3, 4, 8, 9, 10, 11, 12, 13] and list(lab) == [0, 0, 0, 0, 1, 1, 1, 1, 1, 1]
    # a chain and a lone variable with a prior (variable 8, opaque factor 9)
    lone, _ = CS.lone_variable(1)
    both = CS.join_scalar([_chain(2), lone])
    ids, lab, n = CS.labels(both)
    assert n == 2 and list(ids) == [1, 2, 3, 4, 8] and list(lab) == [0, 0, 0, 0, 1]
    # two chains joined by a shared OBSERVED variable: the datum of the second chain's first state is the first chain's variable 3
    m = CS.join_scalar([_chain(2), _chain(2)])
    assert list(m.data_var) == [3, 4, 10, 11]
    for name in ("edge_var", "data_var"):
        a = getattr(m, name).copy()
        a[a == 10] = 3
        setattr(m, name, a)
    m.data_y[2] = m.data_y[0]
    ids, lab, n = CS.labels(m)
    assert n == 1 and list(ids) == [1, 2, 3, 4, 8, 9, 11] and not lab.any()
    hv, hl, _, hn = _host_labels(m)
    assert hn == 1 and list(hv) == list(ids) and not hl.any()


def test_labels_equal_the_host_labelling():
    rng = np.random.default_rng(5)
    tree = CS.relabel(cx.synth.tree_model(60, seed=23, k_choices=(1, 2, 3, 4, 5, 6), observe=0.2, components=5), rng)
    chains = cx.synth.concat_models(CS.chain_parts(2, (2, 3, 65, 300)))
    for model, want_c in ((tree, 5), (chains, 4)):
        ids, lab, n = CS.labels(model)
        hv, hl, hf, hn = _host_labels(model)
        assert n == hn == want_c and (hv == ids).all() and (hl == lab).all()
        # a factor has the label of its variables
        fac_ids = np.unique(model.factor_ids)
        assert (hf[np.searchsorted(fac_ids, model.edge_fac)] == lab[np.searchsorted(ids, model.edge_var)]).all()
        # numbered by least variable id
        first = [ids[lab == k].min() for k in range(n)]
        assert first == sorted(first)
    assert len(np.unique(CS.labels(tree)[1][:5])) > 1        # the relabelled ids interleave the components


def test_host_labelling_and_term_sort_under_the_sanitizers(tmp_path):
    """tests/cpp/components_host.cpp: cx_components.h alone in a stand-alone program built with -fsanitize=address,undefined (CPU only)"""
    exe = str(tmp_path / "components_host")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "cortex.jl_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "components_host.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "components_host: ok" in out.stdout, out.stderr


def test_restrict_splits_the_dense_log_z():
    model = cx.synth.tree_model(60, seed=23, k_choices=(1, 2, 3, 4, 5, 6), observe=0.2, components=5)
    gm = E.gmodel(model)
    lab, n = CS.gm_labels(gm)
    assert n == 5 and (lab == CS.labels(model)[1]).all()
    parts = [E.dense_log_z(CS.restrict(gm, k, lab)) for k in range(n)]
    whole = E.dense_log_z(gm)
    assert abs(sum(parts) - whole) <= 1e-12 * abs(whole), (parts, whole)
    assert sum(len(CS.restrict(gm, k, lab).var_ids) for k in range(n)) == len(gm.var_ids) == 214


def test_restrict_splits_the_bethe_log_z_of_two_grids():
    model = CS.join_scalar([cx.synth.gaussian_grid(4, 3, seed=5), cx.synth.gaussian_grid(3, 3, seed=6)])
    gm = E.gmodel(model)
    lab, n = CS.gm_labels(gm)
    assert n == 2
    f2v = E.numpy_bp(gm, max_iter=300, seed_precision=1e-6)
    whole = E.bethe_log_z(gm, f2v)
    parts = []
    for k in range(n):
        fk, ok = CS.restrict_messages(gm, f2v, (gm.opq_eta, gm.opq_lam), k, lab)
        parts.append(E.bethe_log_z(CS.restrict(gm, k, lab), fk, ok))
    assert np.isfinite(whole) and abs(sum(parts) - whole) <= 1e-12 * abs(whole), (parts, whole)


def test_relabel_keeps_the_model():
    rng = np.random.default_rng(11)
    for model in (cx.synth.tree_model(40, seed=9, k_choices=(1, 2, 3), observe=0.2, components=3), cx.synth.lgssm_chain(12, d=2, seed=4)):
        want = E.dense_log_z(E.gmodel(model))
        other = CS.relabel(model, rng)
        old, new = other.meta["relabel"]
        assert sorted(new) == list(old) and (new != old).any()
        assert not set(other.edge_var.tolist()) & set(other.factor_ids.tolist())          # variables and factors stay distinct
        got = E.dense_log_z(E.gmodel(other))
        assert abs(got - want) <= 1e-12 * abs(want), (got, want)
