"""-m gpu: five and six fused sweeps per launch on grids (cortex.jl_amd/csrc/cx_sweep_deep.hip: k_sweep_deep<5>, <6>; two waves per SIMD), in
calls of at least 16 sweeps under CX_SWEEP_DEPTH=5 and 6.  The kernel body is the one of depths 3 and 4, so are the properties: every level
is the plain sweep's arithmetic term by term, and every comparison here is bit for bit on the float64 read-backs of all factor→variable
messages and all marginals, NaN pattern included, against the same number of sweep(1) calls or the same calls under CX_SWEEP_PAIRS=0.  With
c = 64 - 2 (K - 1) owned columns per strip (54 and 52) the widths lie below the number of levels, around one strip and around a workgroup
column of four; the heights below, at and above the K - 1 halo rows; CX_DEEP_ROWS below the halo and with a short last segment."""
import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from tests.sweep_graphs import assert_same, clean_env, fused_device, model_of, read_back, undefined_midcall_grid
from tests.test_lattice_deep_classes import COLUMN_EDGE, GENERAL, INTERIOR, classes

pytestmark = pytest.mark.gpu

DEPTHS = (5, 6)
DEFAULT_DEPTH = 5          # cx_api_sweep.hip: kDeepDefault (profiles/deep_sweep_56.md: what the measurement chose)
N = 17
ROWS_CASES = (1, 3, 7)     # 7: a short last segment at every height below (2 = 2, 4 = 4, 5 = 5, 9 = 7 + 2, 11 = 7 + 4, 20 = 7 + 7 + 6)
REMAINDER_NS = range(16, 23)


def widths(K):
    c = 64 - 2 * (K - 1)
    return (2, K, 2 * K - 1, c - 1, c, c + 1, 4 * c - 1, 4 * c, 4 * c + 1)


def heights(K):
    return (2, K - 1, 2 * (K - 1) + 1, 20)


def greedy(n, depth):
    """the launches of one call of n sweeps at `depth`, as cx_sweep_deep_launches counts them: [d] launches of d sweeps"""
    count = [0] * 7
    rem = n - 1
    if n < 16:
        depth = 2
    while rem >= 2:
        d = min(depth, rem)
        count[d] += 1
        rem -= d
    return tuple(count)


def test_the_decomposition_this_file_expects():
    assert [greedy(n, 5)[2:] for n in REMAINDER_NS] == [(0, 0, 0, 3, 0), (0, 0, 0, 3, 0), (1, 0, 0, 3, 0), (0, 1, 0, 3, 0), (0, 0, 1, 3, 0), (0, 0, 0, 4, 0), (0, 0, 0, 4, 0)]
    assert [greedy(n, 6)[2:] for n in REMAINDER_NS] == [(0, 1, 0, 0, 2), (0, 0, 1, 0, 2), (0, 0, 0, 1, 2), (0, 0, 0, 0, 3), (0, 0, 0, 0, 3), (1, 0, 0, 0, 3), (0, 1, 0, 0, 3)]
    assert greedy(8, 6) == (0, 0, 3, 0, 0, 0, 0) and all(g[0] == g[1] == 0 for g in (greedy(n, d) for n in REMAINDER_NS for d in DEPTHS))


_plain, _singles = {}, {}


def plain(monkeypatch, shape, calls=(N,)):
    """(messages to variables, marginals) after the calls under CX_SWEEP_PAIRS=0: computed once per grid, shared by both depths and every rows case"""
    if (shape, calls) not in _plain:
        monkeypatch.setenv("CX_SWEEP_PAIRS", "0")
        c = fused_device(model_of(shape))
        for n in calls:
            c.sweep(n)
        monkeypatch.delenv("CX_SWEEP_PAIRS")
        assert c.sweep_deep_launches() == (0,) * 7, shape
        _plain[(shape, calls)] = read_back(c, model_of(shape))
        c.close()
    return _plain[(shape, calls)]


def singles(shape):
    """the read-backs after n = 16 .. 22 calls of sweep(1), computed once"""
    if shape not in _singles:
        b = fused_device(model_of(shape))
        out = {}
        for n in range(1, max(REMAINDER_NS) + 1):
            b.sweep(1)
            if n in REMAINDER_NS:
                out[n] = read_back(b, model_of(shape))
        assert b.sweep_deep_launches() == (0,) * 7
        b.close()
        _singles[shape] = out
    return _singles[shape]


def _run(env, shape, depth, rows, want, calls=(N,)):
    """the calls at `depth` and `rows` rows per segment (None: chosen) on a fresh handle, compared with `want`; returns the handle's launch counts"""
    what = f"{shape}, depth {depth}, {rows or 'chosen'} rows per segment: sweep{calls}"
    env.setenv("CX_SWEEP_DEPTH", str(depth))
    if rows:
        env.setenv("CX_DEEP_ROWS", str(rows))
    a = fused_device(model_of(shape))
    for n in calls:
        a.sweep(n)
    ran = a.sweep_deep_launches()
    d = a.sweep_deep_stats()
    assert d["depth"] == depth and (d["rows"] == rows if rows else d["rows"] >= 4 * (depth - 1)), (what, d)
    assert a.stats()["sweeps_done"] == sum(calls), what
    got = read_back(a, model_of(shape))
    a.close()
    assert np.all(np.isfinite(got[0])), f"{what}: a seeded grid, every message defined"
    assert_same(got, want, what)
    return ran


@pytest.mark.parametrize("height", range(4), ids=("2", "K-1", "2K-1", "20"))
@pytest.mark.parametrize("depth", DEPTHS)
def test_widths_heights_and_rows_per_segment(hip_lib, clean_env, depth, height):
    H = heights(depth)[height]
    for W in widths(depth):
        want = plain(clean_env, (H, W))
        for rows in ROWS_CASES:
            assert _run(clean_env, (H, W), depth, rows, want) == greedy(N, depth)


@pytest.mark.parametrize("depth", DEPTHS)
def test_all_three_instances_in_one_launch(hip_lib, clean_env, depth):
    """24 x 130 at 4 rows per segment: three strips, six segments, of which segments 2 and 3 touch rows 1 .. 22 only (tests/test_lattice_deep_56.py)"""
    cls = classes(depth, 130, 24, 4)[0]
    assert all((cls == k).any() for k in (GENERAL, INTERIOR, COLUMN_EDGE))
    assert _run(clean_env, (24, 130), depth, 4, plain(clean_env, (24, 130))) == greedy(N, depth)


@pytest.mark.parametrize("depth", DEPTHS)
def test_every_remainder(hip_lib, clean_env, depth):
    """20 x 37, sweep(n) for n = 16 .. 22: the n - 1 sweeps before the last leave every remainder 0 .. 5 of the depth, which runs as one launch
    of that depth (5 .. 2) or a plain sweep (1)"""
    ref = singles((20, 37))
    for n in REMAINDER_NS:
        ran = _run(clean_env, (20, 37), depth, None, ref[n], calls=(n,))
        assert ran == greedy(n, depth), (n, depth, ran)
        assert sum(d * k for d, k in enumerate(ran)) == (n - 1 if (n - 1) % depth != 1 else n - 2), (n, depth, ran)


@pytest.mark.parametrize("depth", DEPTHS)
def test_two_consecutive_calls(hip_lib, clean_env, depth):
    ran = _run(clean_env, (20, 37), depth, None, plain(clean_env, (20, 37), (17, 16)), calls=(17, 16))
    assert ran == tuple(x + y for x, y in zip(greedy(17, depth), greedy(16, depth)))


def test_the_default_depth(hip_lib, clean_env):
    """no variable set: a long call runs at kDeepDefault, at the rows per segment chosen by occupancy; 40 x 180 has interior waves there"""
    shape = (40, 180)
    want = plain(clean_env, shape)
    a = fused_device(model_of(shape))
    a.sweep(N)
    assert a.sweep_deep_stats()["depth"] == DEFAULT_DEPTH and a.sweep_deep_launches() == greedy(N, DEFAULT_DEPTH)
    assert_same(read_back(a, model_of(shape)), want, f"{shape} at the default depth")
    a.close()


@pytest.mark.parametrize("depth", DEPTHS)
def test_a_launch_that_meets_an_undefined_message_is_reported_once(hip_lib, clean_env, depth):
    """tests/sweep_graphs.py: undefined_midcall_grid — sweep 3, level 3 of the first launch, reads an undefined message: the NaN path, no fault"""
    clean_env.setenv("CX_SWEEP_DEPTH", str(depth))
    model, sv, sf, payload = undefined_midcall_grid()
    a = fused_device(model)
    a.set_messages(sv, sf, L.TO_VARIABLE, L.FORM_NATURAL, payload)
    errors = []
    for call in (lambda: a.sweep(N), a.sync, a.sync, lambda: a.get_marginals(model.x_ids), a.sync):
        try:
            call()
        except cx.CortexHipError as e:
            errors.append(e)
    assert len(errors) == 1, [str(e) for e in errors]
    assert errors[0].code == L.ERR_DEVICE and "CX_SWEEP_PAIRS=0" in str(errors[0]) and "undefined" in str(errors[0])
    assert a.stats()["sweeps_done"] == N
    ran = a.sweep_deep_launches()
    assert ran == greedy(N, depth)
    a.sweep(N)
    a.sync()
    assert a.sweep_deep_launches() == ran, "the handle sweeps plain from then on"
    assert a.stats()["sweeps_done"] == 2 * N
    a.close()
