"""The oracles of the causal-marginal tests (tests/causal_support.py), pinned against each other on the CPU: the Kalman filter of
tests/missing_data.py, the dense solve of the model without the data a mode leaves out, and the definition of cx_causal_marginals
 restated on the messages of a numpy belief propagation.  The GPU tests compare the device with these.

The error floor, oracle against oracle (Kalman filter against the dense solve, both f64, printed by test_chain_oracles_agree): below
3.2e-14 on every chain here (1e-14 on the trees), scaled as predictive_support.scaled_err scales.  FLOOR is asserted at 1e-11; tests/test_gpu_predictive.py's
tolerance against exact solves, 1e-9, is what the GPU tests use for this arithmetic class, well above 100 x the floor."""
import numpy as np
import pytest

from tests import anisotropic as AN
from tests import causal_support as CS
from tests import evidence_support as E
from tests import missing_data as MD
from tests import predictive_support as P

FLOOR = 1e-11
T = 12


def chain_of(d, n=T):
    """anisotropic.chain has no scalar form (its graphs name parameter sets): at d = 1 the general chain is synth.ssm_chain_linear, with
    per-factor a, b != 0 and q"""
    import cortex.jl_amd as cx

    return cx.synth.ssm_chain_linear(n, seed=42) if d == 1 else AN.chain(n, d)


def tree_of(shape, d):
    """comb(5, d, teeth=2) / branching(15, d, 2); at d = 1 the same shapes as causal_support.scalar_tree"""
    if d == 1:
        return CS.scalar_tree(CS.comb_parents(5, 2) if shape == "comb" else CS.branching_parents(15, 2))
    return AN.comb(5, d, teeth=2) if shape == "comb" else AN.branching(15, d, 2)


def _kalman(model):
    s = MD.chain_spec(model)
    return MD.kalman_filter(s["A"], s["b"], s["Q"], s["H"], s["R"], s["y"], s["keep"])


def _states(gm, model):
    return np.searchsorted(gm.var_ids, model.x_ids)


@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_chain_oracles_agree(d):
    model = chain_of(d)
    gm = E.gmodel(model)
    xs = _states(gm, model)
    f = _kalman(model)
    f2v = E.numpy_bp(gm)
    for mode, mk, Pk in ((CS.PREDICTED, "mp", "Pp"), (CS.FILTERED, "mf", "Pf")):
        dense = CS.dense_causal_all(gm, mode)
        msgs = CS.causal_from_messages(gm, f2v, None, mode)
        want = {"variable_ids": model.x_ids, "mean": f[mk].copy(), "cov": f[Pk].copy()}
        improper = int(mode == CS.PREDICTED)
        if improper:                                 # the first state has no prediction: no prior
            want["mean"][0], want["cov"][0] = np.nan, np.nan
        assert dense["counts"]["improper"] == improper and msgs["counts"] == dense["counts"], (d, mode, dense["counts"], msgs["counts"])
        got = {k: dense[k][xs] for k in ("variable_ids", "mean", "cov")}
        print(d, mode, "kalman vs dense", CS.assert_close(want, got, FLOOR, f"d {d} mode {mode} kalman vs dense"))
        print(d, mode, "messages vs dense", CS.assert_close(msgs, dense, FLOOR, f"d {d} mode {mode} messages vs dense"))
    for lag in (1, 3, T):
        dense = CS.dense_causal_all(gm, CS.FILTERED, lag)
        msgs = CS.causal_from_messages(gm, f2v, None, CS.FILTERED, lag)
        assert msgs["counts"] == dense["counts"] and dense["counts"]["finite"] == dense["counts"]["rows"]
        print(d, "lag", lag, CS.assert_close(msgs, dense, FLOOR, f"d {d} lag {lag}"))
    smooth = MD.kalman_missing(model)
    mean, cov = smooth["mean"], smooth["cov"]
    full = CS.causal_from_messages(gm, f2v, None, CS.FILTERED, T)
    assert P.scaled_err(full["mean"][xs], mean) <= FLOOR and P.scaled_err(full["cov"][xs], cov) <= FLOOR
    # a lag moves the estimate: lag 3 is neither the filter nor the smoother
    l3 = CS.causal_from_messages(gm, f2v, None, CS.FILTERED, 3)
    assert P.scaled_err(l3["mean"][xs[:4]], f["mf"][:4]) > 1e-6 and P.scaled_err(l3["mean"][xs[:4]], mean[:4]) > 1e-9


@pytest.mark.parametrize("d", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", ["comb", "branching"])
def test_tree_oracles_agree(shape, d):
    model = tree_of(shape, d)
    gm = E.gmodel(model)
    f2v = E.numpy_bp(gm)
    for mode, lag in ((CS.PREDICTED, 0), (CS.FILTERED, 0), (CS.FILTERED, 1), (CS.FILTERED, 3), (CS.FILTERED, 15)):
        dense = CS.dense_causal_all(gm, mode, lag)
        msgs = CS.causal_from_messages(gm, f2v, None, mode, lag)
        assert msgs["counts"] == dense["counts"], (shape, d, mode, lag, msgs["counts"], dense["counts"])
        print(shape, d, mode, lag, CS.assert_close(msgs, dense, FLOOR, f"{shape} d {d} mode {mode} lag {lag}"))
    if d > 1:
        xs = _states(gm, model)
        mean, cov = AN.dense_posterior(model)
        full = CS.causal_from_messages(gm, f2v, None, CS.FILTERED, 15)
        assert P.scaled_err(full["mean"][xs], mean) <= FLOOR and P.scaled_err(full["cov"][xs], cov) <= FLOOR


def test_reverse_time_on_additive_chains():
    """CX_FACTOR_GAUSS_ADDITIVE has no roles: the lower id is `out`, so on synth.ssm_chain the causal order runs backwards in time"""
    import cortex.jl_amd as cx

    model = cx.synth.ssm_chain(T, seed=5, random_variances=True)
    gm = E.gmodel(model)
    xs = _states(gm, model)
    s = MD.chain_spec(model)
    r = MD.kalman_filter(s["A"][::-1], s["b"][::-1], s["Q"][::-1], s["H"], s["R"][::-1], s["y"][::-1], s["keep"][::-1])
    f2v = E.numpy_bp(gm)
    flt = CS.causal_from_messages(gm, f2v, None, CS.FILTERED)
    assert P.scaled_err(flt["mean"][xs], r["mf"][::-1]) <= FLOOR and P.scaled_err(flt["cov"][xs], r["Pf"][::-1]) <= FLOOR
    pre = CS.causal_from_messages(gm, f2v, None, CS.PREDICTED)
    assert pre["counts"]["improper"] == 1 and np.isnan(pre["mean"][xs[-1]]).all()
    assert P.scaled_err(pre["mean"][xs[:-1]], r["mp"][::-1][:-1]) <= FLOOR
    for mode, lag in ((CS.PREDICTED, 0), (CS.FILTERED, 0), (CS.FILTERED, 2)):
        CS.assert_close(CS.causal_from_messages(gm, f2v, None, mode, lag), CS.dense_causal_all(gm, mode, lag), FLOOR, f"ssm_chain {mode} {lag}")
