"""The partner-run table of the packed fused sweep (cortex.jl_amd/csrc/cx_partner_runs.h) on the CPU build of the host logic: every
lane the sweep pushes from decodes to exactly partner[slot]; an entry falls back only where its wave really has three pieces; on a
wide grid at least 0.90 of the wave-rows of pairwise factors are covered."""
import ctypes as C

import numpy as np
import pytest

import cortex.jl_amd as cx
from tests.hostlogic import FlatGraph, lib
from tests.sweep_graphs import PARTNER_RUN_GRAPHS

NONE = -2 ** 31


def table(model):
    g = FlatGraph(model.edge_var, model.edge_fac, model.factor_ids, model.factor_kind, model.factor_var, edge_role=model.edge_role)
    assert g.status == 0, g.error
    L = lib()
    L.cxh_flat_partner_runs.restype = C.c_int64
    L.cxh_flat_partner_runs.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    fb = C.c_int64(0)
    n = int(L.cxh_flat_partner_runs(g.p, None, C.byref(fb)))
    ent = np.zeros((max(n, 1), 4), dtype=np.int32)
    if n:
        L.cxh_flat_partner_runs(g.p, ent.ctypes.data, C.byref(fb))
    return g, ent[:n], int(fb.value)


def check_decode(g, ent, fallback):
    """returns (wave-rows with k >= 1, covered ones among them)"""
    partner, slice_off, vinfo, nv = g.arr("partner"), g.arr("slice_off"), g.arr("vinfo"), g.scalar("nv")
    assert len(ent) == slice_off[-1] // 256 * 4
    assert int((ent[:, 2] < 0).sum()) == fallback
    lanes = np.arange(64)
    rows_k1 = covered_k1 = 0
    for s in range(len(slice_off) - 1):
        off, W = int(slice_off[s]), int(slice_off[s + 1] - slice_off[s]) // 256
        for k in range(W):
            for w in range(4):
                v = s * 256 + w * 64 + lanes
                ok = v < nv
                deg = np.where(ok, vinfo[np.minimum(v, nv - 1)] & 15, 0)
                care = ok & (deg != 15) & (k < deg)
                slot = off + k * 256 + w * 64 + lanes
                p = partner[slot]
                want = np.where(p < 0, NONE, p - slot)[care]
                d0, d1, split, _ = (int(x) for x in ent[(off // 256 + k) * 4 + w])
                pieces = 0 if len(want) == 0 else 1 + int((want[1:] != want[:-1]).sum())
                if k >= 1 and care.any():
                    rows_k1 += 1
                    covered_k1 += split >= 0
                if split < 0:
                    assert pieces >= 3, f"slice {s} row {k} wave {w}: falls back with {pieces} piece(s)"
                    continue
                assert pieces <= 2
                got = np.where(lanes < split, d0, d1)[care]
                assert np.array_equal(got, want), f"slice {s} row {k} wave {w}: decoded differences != partner - slot"
    return rows_k1, covered_k1


@pytest.mark.parametrize("name", sorted(PARTNER_RUN_GRAPHS))
def test_every_pushing_lane_decodes_to_its_partner(name):
    g, ent, fb = table(PARTNER_RUN_GRAPHS[name][0]())
    rows, cov = check_decode(g, ent, fb)
    if name == "random600":
        assert cov < 0.5 * rows, (rows, cov)


def test_a_wide_grid_is_covered():
    """24 x 1415: only waves that hold a row end have three pieces — about 64 / 1415 of them; the condition is 0.90"""
    g, ent, fb = table(cx.synth.gaussian_grid(24, 1415, seed=1))
    rows, cov = check_decode(g, ent, fb)
    assert cov >= 0.90 * rows, f"{cov} of {rows} wave-rows of pairwise factors covered ({cov / rows:.3f})"
    k0 = ent[:, 2] >= 0
    assert k0.any()
