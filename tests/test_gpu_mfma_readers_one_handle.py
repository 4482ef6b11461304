"""-m gpu: the four readers of the stored messages at the matrix-core dims on ONE handle across changes — cx_log_evidence_mfma,
cx_factor_beliefs_mfma / cx_factor_statistics_mfma, cx_predictive_mfma and cx_causal_marginals_mfma keep plans, request keys and
parameter tables between calls (cx_mfma_reader.h).  Whatever a handle has kept, it must answer what a fresh handle answers: after a
state becomes observed, after the rule parameters change, and when the requests come in another order.  The fresh handle has the same
graph, the current parameters and the reused handle's exported state; the comparison is byte for byte, the counters included.

No tolerance: both handles run the same kernels on the same messages, and every reader sums in a fixed order."""
import dataclasses

import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L

pytestmark = pytest.mark.gpu
T = 6


def _requests(model):
    lik, tr = model.factor_ids[:T], model.factor_ids[T:]
    return [
        ("evidence", lambda dev: dev.log_evidence_mfma()),
        ("beliefs", lambda dev: dev.factor_beliefs_mfma([tr[1], lik[4]])),
        ("statistics by parameter set", lambda dev: dev.factor_statistics_mfma()),
        ("statistics by the caller's groups", lambda dev: dev.factor_statistics_mfma(tr, [0, 1, 0, -1, 1], 2)),
        ("predictive loo", lambda dev: dev.predictive_mfma("loo")),
        ("predictive loo, no rows", lambda dev: dev.predictive_mfma("loo", rows=False)),
        ("predictive causal", lambda dev: dev.predictive_mfma("causal")),
        ("predictive causal, no rows", lambda dev: dev.predictive_mfma("causal", rows=False)),
        ("causal predicted", lambda dev: dev.causal_marginals_mfma("predicted", 0)),
        ("causal filtered", lambda dev: dev.causal_marginals_mfma("filtered", 0)),
        ("causal filtered lag 2", lambda dev: dev.causal_marginals_mfma("filtered", 2)),
    ]


def _flat(x, name, out):
    """every array and number of a result, by name, as bytes (NaN compares equal to the same NaN)"""
    if isinstance(x, dict):
        for k, v in x.items():
            _flat(v, f"{name}.{k}", out)
    elif isinstance(x, (tuple, list)):
        for i, v in enumerate(x):
            _flat(v, f"{name}[{i}]", out)
    elif x is None:
        out[name] = b""
    else:
        out[name] = np.asarray(x).tobytes()


def _round(dev, model, reverse=False):
    reqs = _requests(model)
    raw = {name: call(dev) for name, call in (reversed(reqs) if reverse else reqs)}
    # the round holds numbers, so that equality is not NaN against NaN
    value, counts = raw["evidence"]
    assert np.isfinite(value) and counts["undefined"] == 0 and counts["not_positive_definite"] == 0, (value, counts)
    assert all(np.isfinite(a).all() for a in raw["beliefs"])
    for name in ("statistics by parameter set", "statistics by the caller's groups"):
        stats, c = raw[name]
        assert c["factors"] > 0 and c["undefined"] == 0 and c["not_positive_definite"] == 0 and np.isfinite(stats["S_rr"]).all(), (name, c)
    for name in ("predictive loo", "predictive loo, no rows", "predictive causal", "predictive causal, no rows"):
        assert raw[name]["counts"]["scored"] > 0 and np.isfinite(raw[name]["total"]), (name, raw[name]["counts"])
    for name in ("causal predicted", "causal filtered", "causal filtered lag 2"):
        assert raw[name]["counts"]["finite"] > 0 and np.isfinite(raw[name]["mean"]).any(), (name, raw[name]["counts"])
    flat = {}
    for name, _ in reqs:
        _flat(raw[name], name, flat)
    return raw, flat


def _fresh(model, psets, blob):
    dev = cx.DeviceGraph(dim=model.dim, schedule=L.SCHED_TREE)
    cx.synth.load_into_device(dataclasses.replace(model, psets=psets), dev)
    dev.import_state(blob)
    return dev


def _same_as_fresh(dev, model, psets, flat, what):
    fresh = _fresh(model, psets, dev.export_state())
    _, want = _round(fresh, model)
    fresh.close()
    assert flat.keys() == want.keys()
    differ = [k for k in flat if flat[k] != want[k]]
    assert not differ, (what, differ)


@pytest.mark.parametrize("d", [8, 33])      # one tile, embedded; 4 x 4 tiles, embedded: the tightest kernels
def test_a_reused_handle_answers_what_a_fresh_one_answers(hip_lib, d):
    model = cx.synth.lgssm_chain(T, d=d, seed=60 + d)
    psets = dict(model.psets)
    dev = cx.DeviceGraph(dim=d, schedule=L.SCHED_TREE)
    cx.synth.load_into_device(model, dev)
    dev.sweep(1)
    raw0, flat = _round(dev, model)
    _same_as_fresh(dev, model, psets, flat, "the first round")

    # 1. a state that was free becomes observed
    i = 2
    x = model.x_ids[i]
    facs = np.asarray(model.edge_fac)[np.asarray(model.edge_var) == x]
    value = np.random.default_rng(61 + d).standard_normal(d)
    dev.set_messages(np.full(len(facs), x), facs, L.TO_FACTOR, L.FORM_POINT, np.tile(value, (len(facs), 1)))
    dev.sweep(1)
    raw1, flat = _round(dev, model)
    _same_as_fresh(dev, model, psets, flat, "after a state became observed")
    row = list(np.sort(np.unique(model.edge_var))).index(x)      # (causal rows: every variable in ascending id)
    for name in ("causal predicted", "causal filtered", "causal filtered lag 2"):
        assert np.array_equal(raw1[name]["mean"][row], value) and not raw1[name]["cov"][row].any(), name
    assert raw1["evidence"][0] != raw0["evidence"][0]

    # 2. other rule parameters
    A, Q = psets[0]
    psets[0] = (A, 2.0 * Q)
    dev.set_factor_matrices(0, *psets[0])
    dev.sweep(1)
    raw2, flat = _round(dev, model)
    _same_as_fresh(dev, model, psets, flat, "after set_factor_matrices")
    assert raw2["evidence"][0] != raw1["evidence"][0]

    # 3. the same requests in the reverse order
    _, flat = _round(dev, model, reverse=True)
    _same_as_fresh(dev, model, psets, flat, "the requests in reverse order")
    dev.close()
