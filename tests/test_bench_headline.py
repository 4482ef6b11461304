"""bench.py's last stdout line is what the driver parses: ONE compact, strict JSON object under 4 KB with the contract's keys,
`roofline` and `cpu_baseline`; everything else goes to a side file.  (Round 5's line had grown to 20.5 KB and the driver's record
came back `parsed: null`.)  The emitter is run here on canned numbers — no GPU."""
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _canned(n_other=14, long_text=400):
    pad = "x" * long_text
    other = [{"config": f"cfg{i}", "ms_per_sweep": 0.1 * i, "workload": pad, "roofline": {"bound": "hbm", "frac": 0.5, "frac_note": pad, "achieved": 1.0},
              "parity": {"ok": True, "max_rel_err": 1e-15, "checker": pad}, "plan": {"stages": 100001, "note": pad}} for i in range(n_other)]
    other.append({"config": "broken", "error": "RuntimeError: " + pad})
    return {
        "metric": "edge-message updates/sec per sweep, 10M-edge Gaussian grid", "value": 2.8634e11, "unit": "edge-message updates/s", "n_gpus": 1,
        "steps": 20, "warmup": 5, "ms_per_step": 0.0559, "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64",
        "data": "synthetic",
        "config": {"workload": "C4: ONE 1415x1415 2-D Gaussian grid loopy BP; " + pad, "schedule": "fused " + pad, "partition": "1 row blocks", "seed": 1234},
        "timed_regions": {"count": 5, "ms_per_step_each": [0.05] * 5, "device_ms_per_step_each": [0.05] * 5},
        "roofline": {"bound": "hbm", "kernel": "void cx::k_sweep<0, false, true, 3, 5, false>(cx::SweepArgs)", "achieved": 6790.123456789, "peak": 8000.0,
                     "unit": "GB/s", "frac": 0.848765432, "traffic": 3.762e8, "basis": "counter bytes / avg launch duration " + pad, "avg_kernel_ms": 0.05544,
                     "payload_bytes_per_launch": 320174880.0, "frac_payload": 0.72, "survey_convention_bytes_per_launch": 512207360.0,
                     "frac_survey_convention": 1.15, "bound_detail": pad, "all_kernels_sampled_ms": {"a": 1.0}},
        "marginals_per_s": 3.6e10, "max_message_change_over_run": float("nan"),
        "cpu_baseline": {"value": 8.8e6, "unit": "edge-message updates/s", "cores": 1, "kind": "port", "sample": "12 sweeps " + pad,
                         "reference_julia": "not on this box", "flooding_all_cores": {"value": 1.3e8, "unit": "edge-message updates/s", "cores": 16, "kind": "port", "sample": pad}},
        "parity": {"max_rel_err_marginals": 1e-13, "max_rel_err_messages": float("inf"), "tolerance": 1e-6, "ok": False, "sweeps": 8, "sample": pad, "checker": pad},
        "other_configs": other,
    }


@pytest.mark.parametrize("n_other,long_text", [(0, 10), (14, 400), (60, 3000)])
def test_the_headline_is_one_compact_strict_json_line(n_other, long_text):
    full = _canned(n_other, long_text)
    line = bench.headline_line(full, "gpurun_out/bench_details_n1.json")
    assert "\n" not in line
    assert len(line.encode()) < 4096
    assert "NaN" not in line and "Infinity" not in line

    def no_constants(tok):
        raise AssertionError(f"non-finite token {tok} in the headline")
    d = json.loads(line, parse_constant=no_constants)
    assert set(d) <= set(bench.HEADLINE_KEYS) | {"other_configs_digest", "weak_scaling", "halo_check"}
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "cpu_baseline", "parity", "details"):
        assert k in d, k
    assert d["config"]["workload"].startswith("C4")
    assert "model" not in d["config"]
    ro = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "payload_bytes_per_launch", "frac_survey_convention"):
        assert k in ro, k
    assert not any(k.startswith("frac_algorithmic") for k in ro)
    assert abs(ro["frac"] - ro["achieved"] / ro["peak"]) < 1e-3
    cb = d["cpu_baseline"]
    assert set(("value", "unit", "cores", "kind", "sample")) <= set(cb) and cb["kind"] in ("port", "reference")
    assert d["parity"]["ok"] is False and d["parity"]["max_rel_err_messages"] is None      # inf -> null, the verdict stays
    assert d["value"] == pytest.approx(2.8634e11) and d["steps"] == 20 and d["warmup"] == 5


def test_a_multi_gpu_line_without_cpu_baseline_is_still_valid():
    full = _canned(0, 10)
    for k in ("cpu_baseline", "parity", "other_configs"):
        del full[k]
    full["n_gpus"] = 8
    full["weak_scaling"] = {"value": 1e12, "unit": "edge-message updates/s", "ms_per_step": 0.06, "workload": "w" * 500, "schedule": "s" * 500}
    full["halo_check"] = "ok: last imported halo == neighbours' packed messages, bit for bit"
    d = json.loads(bench.headline_line(full, None))
    assert d["n_gpus"] == 8 and "cpu_baseline" not in d and d["details"] is None
    assert d["weak_scaling"]["value"] == 1e12 and "workload" not in d["weak_scaling"]


def test_the_side_file_holds_everything_and_is_strict_json(tmp_path, monkeypatch, capsys):
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    rel = bench.write_details(_canned(3, 50), 1)
    assert rel == os.path.join("gpurun_out", "bench_details_n1.json")
    text = open(tmp_path / rel).read()
    assert "NaN" not in text and "Infinity" not in text
    d = json.loads(text)
    assert len(d["other_configs"]) == 4 and "timed_regions" in d
    err = capsys.readouterr()
    assert err.out == "" and "[bench] details:" in err.err        # stdout stays clean for the one line


def test_bench_prints_the_headline_last_and_only_once():
    src = open(os.path.join(ROOT, "bench.py")).read()
    body = src[src.index("def run_rank"):src.index("def main")]
    assert body.count("print(headline_line(") == 1
    assert "print(json.dumps(out)" not in body


def test_a_plain_run_line_holds_the_contract_keys_and_no_roofline():
    full = _canned(0, 10)
    for k in ("roofline", "cpu_baseline", "parity", "other_configs"):
        del full[k]
    d = json.loads(bench.headline_line(full, None))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"):
        assert k in d, k
    assert d["details"] is None and not {"roofline", "cpu_baseline", "parity", "other_configs_digest"} & set(d)


def test_the_extras_are_behind_full_and_steps_is_one_region():
    a = bench.parse(["--gpus", "1", "--steps", "30", "--warmup", "4"])
    assert a.full is False and a.repeats is None and a.dump_outputs is None and a.steps == 30
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"
    body = open(os.path.join(ROOT, "bench.py")).read()
    body = body[body.index("def run_rank"):body.index("def main")]
    assert "(5 if args.full else 1)" in body
    lines = body.splitlines()
    for call in ("cpu_baseline(", "parity_check(", "other_configs(", "write_details(", "roofline(", "dev.profile_enable(", "timed_regions(w2"):
        n = next(i for i, l in enumerate(lines) if call in l and not l.lstrip().startswith("#"))
        guard = next(l for l in reversed(lines[:n + 1]) if re.match(r"\s*(el)?if ", l) or " if args.full else " in l)
        assert "args.full" in guard, (call, guard)


class _FakeDev:
    """what dump_outputs reads: marginals and messages as functions of the ids, so that a sample is recognisable"""
    def get_marginals(self, ids):
        ids = np.asarray(ids, dtype=np.float64)
        return np.stack([ids, -ids], axis=1)

    def get_messages(self, v, f, direction):
        return np.stack([np.asarray(v, dtype=np.float64), np.asarray(f, dtype=np.float64)], axis=1)


def test_dump_outputs_writes_float64_and_samples_the_same_entries_every_time(tmp_path, monkeypatch):
    import types

    import cortex.jl_amd as cx

    model = cx.synth.gaussian_grid(20, 20, seed=3)
    w = types.SimpleNamespace(model=model, part=None, dev=_FakeDev())
    budget = (bench.DUMP_MAX_MARGINALS + bench.DUMP_MAX_MESSAGES) * 2 * 8     # (mean, variance) pairs of float64
    assert budget <= 64 * 2**20
    shapes = bench.dump_outputs(str(tmp_path / "all"), w)
    assert shapes == {"marginals": [400, 2], "messages_to_variable": [len(model.edge_var), 2]}
    m = np.load(tmp_path / "all" / "marginals.npy")
    assert m.dtype == np.float64 and np.array_equal(m[:, 0], model.x_ids)
    monkeypatch.setattr(bench, "DUMP_MAX_MARGINALS", 50)
    monkeypatch.setattr(bench, "DUMP_MAX_MESSAGES", 70)
    for d in ("s1", "s2"):
        assert bench.dump_outputs(str(tmp_path / d), w) == {"marginals": [50, 2], "messages_to_variable": [70, 2]}
    for name in ("marginals", "messages_to_variable"):
        a, b = np.load(tmp_path / "s1" / f"{name}.npy"), np.load(tmp_path / "s2" / f"{name}.npy")
        assert a.dtype == np.float64 and np.array_equal(a, b)
    s = np.load(tmp_path / "s1" / "marginals.npy")[:, 0]
    assert np.all(np.diff(s) > 0) and np.all(np.isin(s, model.x_ids))
