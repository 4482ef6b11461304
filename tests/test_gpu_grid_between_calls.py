"""-m gpu: a grid handle across what a caller does BETWEEN two cx_sweep calls, now that a call of three sweeps or more runs two sweeps per
launch (cortex.jl_amd/csrc/cx_sweep_pair.hip).  The handle keeps a verdict on its inputs (cx_api_sweep.hip: pairs_allowed) that cxh::changed
(cx_derived.h) makes due again; a forgotten flag shows as the old model's answer, a flag raised for nothing as pairs that never come back.

Every scenario drives three things through the same steps: `a` (calls of n sweeps, pairs on), `b` (the same with sweep(1) n times) and `g`,
the moment-form CPU checker (oracle/bp_flood.c), which shares no code with the device.  After every phase: a == b bit for bit on messages
to variables, marginals and messages to factors; a against g within RTOL of tests/test_gpu_scalar_parity.py on the messages, and on the
marginals against g one sweep earlier (the marginals a sweep writes are those of the messages it read); and a's count of paired launches
equals what pairs_allowed gives for that history, worked out from the code and written next to each call.

Then: the readers after a paired call, the refusal path (a launch that meets an undefined variable→factor message), and CX_PAIR_NT=1."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cortex.jl_amd as cx
from cortex.jl_amd import _lib as L
from tests.helpers import assert_close, flood_oracle_from_model
from tests.sweep_graphs import GridIds, assert_same, everything, fused_device, load_undefined_midcall, natural_form_sweeps, paired_launches, read_back, undefined_midcall_grid
from tests.test_gpu_damping import _numpy_damped_sweeps
from tests.test_gpu_scalar_parity import RTOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED_VARIANCE = 1e6
# 9 x 125: three strips, their boundaries at columns 61 | 62 and 123 | 124 (halo lanes); 20 x 37: one strip, three slices, five segments
GRID, SMALL = (9, 125), (20, 37)
# (0, 0) a corner, (3, 61) | (3, 62) and (8, 124) either side of a strip boundary, (4, 30) inside a strip; the same roles on 20 x 37, where
# the variables 256 and 257 = (6, 33) and (6, 34) lie either side of a slice boundary
PRIOR_AT = {GRID: [(0, 0), (3, 61), (3, 62), (8, 124), (4, 30)], SMALL: [(0, 0), (6, 33), (6, 34), (19, 36), (4, 30)]}


class Trio:
    """`a`, `b` and `g` on one model, and the paired launches `a` must have run so far"""

    def __init__(self, shape, seed=7):
        self.model = cx.synth.gaussian_grid(*shape, seed=seed)
        self.ids = GridIds(*shape)
        self.a, self.b = fused_device(self.model), fused_device(self.model)
        self.g = flood_oracle_from_model(self.model, seed_variance=SEED_VARIANCE)
        self.g_marginals = None
        self.pairs = 0
        self.damping = 0.0

    def close(self):
        self.a.close(); self.b.close()

    def both(self, call):
        for d in (self.a, self.b):
            call(d)

    def g_sweep(self, n):
        if self.damping:
            _numpy_damped_sweeps(self.g, self.damping, n)
        else:
            self.g.sweep(n)

    def sweep(self, n, pairs, what, oracle=True):
        """one call of n sweeps on `a`, which must run `pairs` paired launches in it, and everything compared afterwards"""
        self.a.sweep(n)
        for _ in range(n):
            self.b.sweep(1)
        self.g_sweep(n - 1)
        self.g_marginals = self.g.marginals()
        self.g_sweep(1)
        self.pairs += pairs
        self.check(what, oracle)

    def check(self, what, oracle=True):
        assert paired_launches(self.a) == self.pairs, f"{what}: paired launches of a"
        assert paired_launches(self.b) == 0
        assert self.a.stats()["sweeps_done"] == self.b.stats()["sweeps_done"]
        ra = everything(self.a, self.model)
        assert_same(ra, everything(self.b, self.model), what)
        if not oracle:
            return
        g = self.g
        got = self.a.get_messages(g.edge_var, g.edge_fac, L.TO_VARIABLE)
        for col, want, name in ((0, g.f2v_m, "mean"), (1, g.f2v_v, "variance")):
            err = assert_close(got[:, col], want, RTOL, f"{what}: message {name} against the CPU checker")
            print(f"{what}: message {name}: max rel err {err:.3e}")
        for col, want, name in ((0, self.g_marginals[0], "mean"), (1, self.g_marginals[1], "variance")):
            err = assert_close(ra[1][:, col], want, RTOL, f"{what}: marginal {name} against the CPU checker one sweep earlier")
            print(f"{what}: marginal {name}: max rel err {err:.3e}")


@pytest.fixture
def pairs_on(monkeypatch):
    for name in ("CX_SWEEP_PAIRS", "CX_PAIR_ROWS", "CX_MARG_EVERY_SWEEP"):
        monkeypatch.delenv(name, raising=False)


# ---- 2. one change between two calls, three ways ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [GRID, SMALL], ids=lambda s: "%dx%d" % s)
def test_new_priors_between_two_calls(hip_lib, pairs_on, shape):
    t = Trio(shape)
    t.sweep(5, 2, "before")                     # the first call of >= 3 sweeps checks (due since the graph was made), finds a seeded grid: (5 - 1) // 2
    rng = np.random.default_rng(11)
    at = PRIOR_AT[shape]
    v = np.array([t.ids.var(r, c) for r, c in at], dtype=np.int64)
    f = np.array([t.ids.unary(r, c) for r, c in at], dtype=np.int64)
    mean, var = rng.standard_normal(len(at)) * 3.0, rng.uniform(0.3, 3.0, len(at))
    t.both(lambda d: d.set_messages(v, f, L.TO_VARIABLE, L.FORM_MOMENT, np.stack([mean, var], axis=1)))
    t.g.set_message_to_variable(v, f, mean, var)
    # StoredToVariable makes the check due; cx_set_messages wrote both Jacobi buffers, so the unary messages agree and every message is defined: 2 more
    t.sweep(5, 2, "after new priors")
    t.sweep(4, 1, "and a call of four")          # nothing changed: no check, (4 - 1) // 2
    t.close()


def test_a_cut_message_between_two_calls(hip_lib, pairs_on):
    t = Trio(GRID)
    t.sweep(5, 2, "before")
    v, f = t.ids.var(4, 62), t.ids.factor(4, 62, "left")      # the left neighbour's message into (4, 62): across the strip boundary 61 | 62
    t.both(lambda d: d.set_messages([v], [f], L.TO_VARIABLE, L.FORM_MOMENT, np.array([[0.7, 1.3]])))
    t.g.set_message_to_variable([v], [f], [0.7], [1.3])
    t.sweep(5, 2, "after a cut message")        # the check is due and passes (a defined value, in both buffers)
    t.close()


def test_seed_again_between_two_calls(hip_lib, pairs_on):
    """a seed fills undefined messages only: one message is made undefined, then seeded with another variance"""
    t = Trio(GRID)
    t.sweep(5, 2, "before")
    v, f = t.ids.var(3, 60), t.ids.factor(3, 60, "up")
    t.both(lambda d: d.set_messages([v], [f], L.TO_VARIABLE, L.FORM_NATURAL, np.array([[np.nan, np.nan]])))
    t.both(lambda d: d.seed_messages(L.TO_VARIABLE, 0.0, 25.0))
    t.g.set_message_to_variable([v], [f], [0.0], [25.0])
    t.sweep(5, 2, "after a second seed")        # due (a store, a seed); the seed has filled the hole in both buffers: the check passes
    t.close()


def test_seed_after_a_failed_check_brings_pairs_back_at_once(hip_lib, pairs_on):
    """an undefined message fails the check and the handle would look again 16 sweeps on; a seed makes the check due in the very next call"""
    t = Trio(GRID)
    t.sweep(5, 2, "before", oracle=False)
    v, f = t.ids.var(3, 60), t.ids.factor(3, 60, "up")
    t.both(lambda d: d.set_messages([v], [f], L.TO_VARIABLE, L.FORM_NATURAL, np.array([[np.nan, np.nan]])))
    t.sweep(3, 0, "an undefined input", oracle=False)       # the check fails: plain, and not looked at before sweep 5 + 16
    t.both(lambda d: d.seed_messages(L.TO_VARIABLE, 0.0, 25.0))
    t.sweep(5, 2, "seeded", oracle=False)        # 8 < 21 sweeps done, but Seeded made the check due; three plain sweeps have defined every message
    t.close()


def test_update_batch_between_two_calls(hip_lib, pairs_on):
    """messages to and from (4, 62) recomputed and the marginals of its row refreshed by cx_update_batch: the messages to the variable come
    out of the stored variable→factor messages, which are those the last sweep formed, so they are the last sweep's own; the marginals come
    out of the current messages, so the row's marginals move ON by one sweep"""
    t = Trio(GRID)
    t.sweep(5, 2, "before")
    pv, pf = t.ids.pairwise_edges(4, 62)
    row = np.array([t.ids.var(4, c) for c in range(GRID[1])], dtype=np.int64)
    # (three batches: the items of one batch run side by side, and these read what the others write)
    t.both(lambda d: d.update_batch([L.ITEM_MESSAGE_TO_FACTOR] * 4, pv, pf))
    t.both(lambda d: d.update_batch([L.ITEM_MESSAGE_TO_VARIABLE] * 4, pv, pf))
    t.both(lambda d: d.update_batch([L.ITEM_INDIVIDUAL_MARGINAL] * len(row), row, np.zeros(len(row), dtype=np.int64)))
    t.g_marginals = t.g.marginals()              # of the CURRENT messages, for the row; the other rows keep the last sweep's
    ma, mb = t.a.get_marginals(row), t.b.get_marginals(row)
    assert np.array_equal(ma, mb)
    assert_close(ma[:, 0], t.g_marginals[0][row - 1], RTOL, "batch: marginal means of the row")
    assert_close(ma[:, 1], t.g_marginals[1][row - 1], RTOL, "batch: marginal variances of the row")
    assert_same(everything(t.a, t.model), everything(t.b, t.model), "after the batch")
    got = t.a.get_messages(t.g.edge_var, t.g.edge_fac, L.TO_VARIABLE)
    assert_close(got[:, 0], t.g.f2v_m, RTOL, "batch: message means")
    assert_close(got[:, 1], t.g.f2v_v, RTOL, "batch: message variances")
    t.sweep(5, 2, "after a batch")              # BatchWrote makes the check due; everything is defined and no unary message was touched
    t.close()


@pytest.mark.parametrize("shape", [GRID, SMALL], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("at", [5, 6])
def test_state_import_continues_the_exporter(hip_lib, pairs_on, shape, at):
    """exported after 5 and after 6 sweeps (d_f2v is either buffer), imported into a handle with other messages and another sweep count"""
    t = Trio(shape)
    t.sweep(5, 2, "before")
    if at == 6:
        t.sweep(1, 0, "one more")                # a call of fewer than three sweeps runs none
    blob = t.a.export_state()
    imp = fused_device(t.model, 50.0)
    imp.sweep(2)
    assert paired_launches(imp) == 0
    imp.import_state(blob)
    assert_same(everything(imp, t.model), everything(t.a, t.model), "right after the import")
    t.sweep(5, 2, "the exporter goes on")
    imp.sweep(5)
    assert paired_launches(imp) == 2                      # the importer's first call of >= 3 sweeps: checks the imported buffers, which a paired exporter left consistent
    assert imp.stats()["sweeps_done"] == at + 5
    assert_same(everything(imp, t.model), everything(t.a, t.model), "the importer against the exporter continuing")
    imp.close(); t.close()


def test_state_import_after_a_failed_check_brings_pairs_at_once(hip_lib, pairs_on):
    """the importer was never seeded: its own check failed and it would look again once 16 sweeps are done; the imported state is defined"""
    t = Trio(GRID)
    t.sweep(5, 2, "before", oracle=False)
    imp = fused_device(t.model, None)
    imp.sweep(3)
    assert paired_launches(imp) == 0 and np.isnan(read_back(imp, t.model)[0]).any()
    imp.import_state(t.a.export_state())
    t.sweep(5, 2, "the exporter goes on", oracle=False)
    imp.sweep(5)
    assert paired_launches(imp) == 2                      # StateImported made the check due: 5 < 16 sweeps done does not matter
    assert_same(everything(imp, t.model), everything(t.a, t.model), "the importer against the exporter continuing")
    imp.close(); t.close()


def test_damping_on_and_off_again(hip_lib, pairs_on):
    """(the oracle leg: tests/test_gpu_damping.py's definition, natural parameters mixed, on the moment-form checker)"""
    t = Trio(GRID)
    t.sweep(5, 2, "before")
    t.both(lambda d: d.set_damping(0.25))
    t.damping = 0.25
    t.sweep(5, 0, "damped")                     # h->damping != 0: no pair, whatever the verdict
    t.both(lambda d: d.set_damping(0.0))
    t.damping = 0.0
    t.sweep(5, 2, "damping off again")          # the verdict of the first call still holds (damped sweeps define what they write): 2, without a check
    t.close()


def test_profiling_on_and_off_again(hip_lib, pairs_on):
    t = Trio(GRID)
    t.sweep(5, 2, "before")
    t.both(lambda d: d.profile_enable(1))
    t.sweep(5, 0, "profiled")                   # h->profiling: events around every launch, so every sweep is a launch of its own
    for d in (t.a, t.b):
        launches = sum(d.profile_read(k)[1] for k in range(L.KERNEL_COUNT))
        assert launches >= 5, "five profiled sweeps leave at least five records"
    t.both(lambda d: d.profile_enable(0))
    t.sweep(5, 2, "profiling off again")
    t.close()


def test_a_new_stream_between_two_calls(hip_lib, pairs_on):
    import torch

    t = Trio(GRID)
    t.sweep(5, 2, "before")
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    t.a.set_stream(sa.cuda_stream); t.b.set_stream(sb.cuda_stream)
    t.sweep(5, 2, "on a stream of the caller's")   # the stream is no input of the verdict: no check, 2
    t.both(lambda d: d.set_stream(None))
    t.sweep(5, 2, "back on the null stream")
    t.close()


def test_sweep_until_with_and_without_pairs(hip_lib, monkeypatch, pairs_on):
    """the CPU checker's largest change of a message over five sweeps on this grid: 2.3e-3 after 20 sweeps, 3.2e-4 after 25"""
    model = cx.synth.gaussian_grid(*GRID, seed=7)
    a = fused_device(model)
    na, ra = a.sweep_until(1e-3, 60, check_every=5)
    monkeypatch.setenv("CX_SWEEP_PAIRS", "0")
    c = fused_device(model)
    nc, rc = c.sweep_until(1e-3, 60, check_every=5)
    monkeypatch.delenv("CX_SWEEP_PAIRS")
    assert na == nc == 25
    assert ra == rc and 1e-4 < ra <= 1e-3
    assert paired_launches(a) == 2 * na // 5 and paired_launches(c) == 0        # every round is a call of five sweeps: 2 each; cx_residual changes nothing
    assert_same(everything(a, model), everything(c, model), "sweep_until")
    g = flood_oracle_from_model(model, seed_variance=SEED_VARIANCE)
    g.sweep(na)
    got = a.get_messages(g.edge_var, g.edge_fac, L.TO_VARIABLE)
    assert_close(got[:, 0], g.f2v_m, RTOL, "sweep_until: message means")
    assert_close(got[:, 1], g.f2v_v, RTOL, "sweep_until: message variances")
    a.close(); c.close()


# ---- 3. readers after a paired call ---------------------------------------------------------------------------------------------------------
def _outcome(call):
    """what a reader returns, or the error it refuses with"""
    try:
        return ("ok", call())
    except cx.CortexHipError as e:
        return ("refused", e.code, e.message)


def _flat(x):
    """every array and number of a reader's result, in order"""
    if x is None:
        return []
    if isinstance(x, dict):
        return [y for k in sorted(x) for y in _flat(x[k])]
    if isinstance(x, (tuple, list)):
        return [y for e in x for y in _flat(e)]
    return [np.asarray(x)]


def test_readers_after_a_paired_call(hip_lib, monkeypatch, pairs_on):
    """after a paired call d_f2v_alt is "the last sweep's input" as after plain sweeps (the last sweep of a call is plain): every reader that
    takes a loopy scalar fused handle returns the same bits from a handle that ran pairs and from one that did not"""
    model = cx.synth.gaussian_grid(*GRID, seed=7)
    ids = GridIds(*GRID)
    pairwise = model.factor_ids[model.factor_kind == L.FACTOR_GAUSS_ADDITIVE]
    groups = (pairwise % 3).astype(np.int64)
    row = np.array([ids.var(4, c) for c in range(GRID[1])], dtype=np.int64)
    joint = np.array([ids.factor(4, c, "right") for c in range(60, 64)] + [ids.factor(r, 62, "down") for r in range(3, 6)], dtype=np.int64)

    def run(dev):
        dev.sweep(6)
        out = {}
        out["log_evidence"] = _outcome(dev.log_evidence)
        out["factor_beliefs"] = _outcome(lambda: dev.factor_beliefs(pairwise))
        out["factor_statistics"] = _outcome(lambda: dev.factor_statistics(pairwise, groups))
        out["message_health"] = _outcome(dev.message_health)
        out["residual_1"] = _outcome(dev.residual)
        out["residual_2"] = _outcome(dev.residual)
        # the stored JointMarginal / ProductOfMessages values are what a batch computed: from the stored variable→factor messages, formed on demand
        kinds = [L.ITEM_JOINT_MARGINAL] * len(joint) + [L.ITEM_PRODUCT_OF_MESSAGES] * len(row)
        vs = np.concatenate([np.zeros(len(joint), dtype=np.int64), row])
        fs = np.concatenate([joint, np.full(len(row), L.item_range(2, 4), dtype=np.int64)])
        out["update_batch"] = _outcome(lambda: dev.update_batch(kinds, vs, fs))
        out["joint_marginals"] = _outcome(lambda: dev.get_joint_marginals(joint))
        out["products"] = _outcome(lambda: dev.get_products(row, np.full(len(row), 2), np.full(len(row), 4)))
        out["linear_moments"] = _outcome(lambda: dev.linear_moments([([int(row[0])], np.ones((1, 1)))]))
        out["everything"] = ("ok", everything(dev, model))
        return out

    a = fused_device(model)
    ra = run(a)
    assert paired_launches(a) == 2
    monkeypatch.setenv("CX_SWEEP_PAIRS", "0")
    c = fused_device(model)
    rc = run(c)
    assert paired_launches(c) == 0
    for name in ra:
        assert ra[name][0] == rc[name][0], f"{name}: {ra[name]} against {rc[name]}"
        if ra[name][0] == "refused":
            assert ra[name] == rc[name], name
            continue
        xa, xc = _flat(ra[name][1]), _flat(rc[name][1])
        assert len(xa) == len(xc)
        for x, y in zip(xa, xc):
            assert np.array_equal(x, y, equal_nan=True), f"{name} differs after a paired call"
    # the readers this test is about took the handle, and read something
    for name in ("log_evidence", "factor_beliefs", "factor_statistics", "message_health", "residual_1", "residual_2", "update_batch", "joint_marginals", "products"):
        assert ra[name][0] == "ok", (name, ra[name])
    assert np.isfinite(ra["log_evidence"][1][0]) and ra["log_evidence"][1][1]["undefined"] == 0
    assert np.all(np.isfinite(ra["factor_beliefs"][1][0])) and np.all(np.isfinite(ra["joint_marginals"][1][1])) and np.all(np.isfinite(ra["products"][1]))
    assert ra["message_health"][1]["undefined"] == 0 and ra["message_health"][1]["defined"] > 0
    assert ra["residual_1"][1] == np.inf and ra["residual_2"][1] == 0.0       # the first call takes the snapshot, the second finds nothing changed
    assert ra["linear_moments"][0] == "refused"                               # exact moments need a forest
    a.close(); c.close()


# ---- 4. the refusal path ----------------------------------------------------------------------------------------------------------------------
def test_a_launch_that_meets_an_undefined_message_is_reported_once(hip_lib, monkeypatch, pairs_on):
    """tests/sweep_graphs.py: undefined_midcall_grid — every input defined, so the check lets pairs start; sweep 1 divides by 1 + q w = 0, sweep 2
    stores undefined messages, and the second launch of sweep(7) (sweeps 3 and 4) reads them, as does the third.  The word a launch raises is
    found by whichever checked call comes first once the launch has run — cx_sweep's own last check, or the cx_sync behind it."""
    model, sv, sf, payload = undefined_midcall_grid()
    assert natural_form_sweeps(model, SEED_VARIANCE, sv, sf, payload, 3) == [(1, 0, 0), (0, 3, 0), (0, 0, 8)]
    model, a = load_undefined_midcall()
    errors = []
    for call in (lambda: a.sweep(7), a.sync, a.sync, lambda: a.get_marginals(model.x_ids), a.sync):
        try:
            call()
        except cx.CortexHipError as e:
            errors.append(e)
    assert len(errors) == 1, [str(e) for e in errors]
    assert errors[0].code == L.ERR_DEVICE and "CX_SWEEP_PAIRS=0" in str(errors[0]) and "undefined" in str(errors[0])
    assert a.stats()["sweeps_done"] == 7
    ran = paired_launches(a)
    assert ran == 3
    a.sweep(5)
    a.sync()
    assert paired_launches(a) == ran, "the handle sweeps plain from then on"
    assert a.stats()["sweeps_done"] == 12
    a.close()
    # plain sweeps keep the older value of a slot whose input is undefined: the same inputs run to completion, one call or seven
    monkeypatch.setenv("CX_SWEEP_PAIRS", "0")
    _, c = load_undefined_midcall()
    _, b = load_undefined_midcall()
    c.sweep(7)
    c.sync()
    for _ in range(7):
        b.sweep(1)
    assert paired_launches(c) == 0 and paired_launches(b) == 0
    assert_same(everything(c, model), everything(b, model), "CX_SWEEP_PAIRS=0: sweep(7) against 7 x sweep(1)")
    c.close(); b.close()


# ---- 5. CX_PAIR_NT=1 ----------------------------------------------------------------------------------------------------------------------------
def test_nontemporal_stores_in_a_process_of_their_own(hip_lib, tmp_path, pairs_on):
    """CX_PAIR_NT is read once per process: a fresh child (tests/_pair_nt_worker.py) sweeps the 9 x 125 grid eight times and dumps its read-backs"""
    out = str(tmp_path / "nt.npz")
    env = dict(os.environ, CX_PAIR_NT="1")
    for name in ("CX_SWEEP_PAIRS", "CX_PAIR_ROWS", "CX_MARG_EVERY_SWEEP"):
        env.pop(name, None)
    p = subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_pair_nt_worker.py"), str(GRID[0]), str(GRID[1]), "8", out], env=env, cwd=ROOT)
    try:
        assert p.wait(timeout=120) == 0
    finally:
        if p.poll() is None:
            p.kill()
    got = np.load(out)
    assert json.loads(str(got["info"])) == {"nt": "1", "paired_launches": 3, "sweeps_done": 8}
    model = cx.synth.gaussian_grid(*GRID, seed=7)
    b = fused_device(model)
    for _ in range(8):
        b.sweep(1)
    assert_same((got["f2v"], got["marg"], got["v2f"]), everything(b, model), "CX_PAIR_NT=1 against plain sweeps")
    b.close()
