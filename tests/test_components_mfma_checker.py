"""CPU: the inputs of tests/test_gpu_evidence_components_mfma.py are what those tests take them for (tests/components_mfma_support.py), so
that the GPU tests cannot pass on a degenerate input: the joined graphs have the components they are built from, by two independent
labellings; the dense value of a component cut out of the joined model is that of the part alone; no value is near zero, where a relative
tolerance says nothing; the long chain of the tile-border graph is longer than a tile of the segmented sum."""
import math

import numpy as np
import pytest

from tests import components_mfma_support as M
from tests import components_support as CS
from tests import evidence_support as E


@pytest.mark.parametrize("d", M.DIMS)
def test_three_chains_are_three_components_with_the_values_of_the_parts(d):
    parts, model, wants = M.chains(d)
    ids, lab, n = CS.labels(model)
    gm = E.gmodel(model)
    glab, gn = CS.gm_labels(gm)
    assert n == 3 and gn == 3 and (glab == lab).all()
    for k, (part, want) in enumerate(zip(parts, wants)):
        cut = E.dense_log_z(CS.restrict(gm, k, glab))
        assert math.isfinite(want) and abs(want) >= 1, (d, k, want)
        assert abs(cut - want) <= 1e-12 * abs(want), (d, k, cut, want)
        assert int((lab == k).sum()) == 2 * len(part.x_ids)      # the states and their data


@pytest.mark.parametrize("d", [5, 17])
def test_forest_has_a_comb_and_two_chains(d):
    model = M.forest(d)
    gm = E.gmodel(model)
    glab, gn = CS.gm_labels(gm)
    assert gn == 3 and (glab == CS.labels(model)[1]).all()
    rng = np.random.default_rng(31)
    again = CS.relabel(model, rng)
    assert CS.labels(again)[2] == 3
    for k in range(3):
        want = E.dense_log_z(CS.restrict(gm, k, glab))
        assert math.isfinite(want) and abs(want) >= 1, (d, k, want)


def test_tile_border_graph():
    model, opq, comp_of_part, wants, n = M.borders()
    assert n == M.N_SHORT + 2 and sorted(comp_of_part) == list(range(n))
    assert 3 * M.LONG - 1 > 1024      # the long chain's terms (2 T - 1 factors, T variables): more than one tile
    assert all(math.isfinite(w) for w in wants) and min(abs(w) for w in wants[:-1]) >= 1 and abs(wants[-1]) <= 1e-12
    assert np.linalg.eigvalsh(opq[3][0])[0] > 0


def test_two_rings_are_two_loopy_components():
    d = 16
    model = M.rings(d)
    gm = E.gmodel(model)
    glab, gn = CS.gm_labels(gm)
    assert gn == 2 and (glab == CS.labels(model)[1]).all()
    for k in range(2):
        cut = CS.restrict(gm, k, glab)
        assert sum(len(g["fid"]) for g in cut.groups.values()) == len(cut.var_ids)      # T likelihoods and T transitions on T states and T data: one loop
        assert abs(E.dense_log_z(cut)) >= 1
