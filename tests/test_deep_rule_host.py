"""The deep sweep's additive rule with one division (cortex.jl_amd/csrc/cx_sweep_deep.hip: deep_rule) against the rule of the plain
kernels with one division per branch (cx_scalar_core.h: factor_rule<kRuleAdditive>), both restated for the host in
tests/deep_rule_host.cpp: the same bits on every triple of 22 special values (+-0, +-inf, NaN, denormals, the least and the largest
normal numbers, ...) and on 1e6 random inputs (any bit pattern; the magnitudes of a model; a fifth of them at a point mass), a NaN equal
to a NaN.  No GPU.  Built without contraction and, where the CPU has a fused multiply-add, with it, as the device code is.  The GPU side
of the same statement: tests/test_gpu_sweep_deep_rule.py and the bit-for-bit comparisons of tests/test_gpu_sweep_deep*.py."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "deep_rule_host.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "cortex.jl_amd", "csrc")
N = 1_000_000


def _cpu_has_fma():
    try:
        return " fma " in open("/proc/cpuinfo").read().replace("\n", " ")
    except OSError:
        return False


def _code(text):
    return re.sub(r"\s+", " ", re.sub(r"//[^\n]*", "", text))


def test_the_restatement_is_the_code():
    """the two forms in tests/deep_rule_host.cpp say what the sources say: the same expressions for the denominator and the two products"""
    host = _code(open(SRC).read())
    deep = _code(open(os.path.join(CSRC, "cx_sweep_deep.hip")).read())
    core = _code(open(os.path.join(CSRC, "cx_scalar_core.h")).read())
    for part in ("const double s = 1.0 / ((pm ? -0.0 : 1.0) + q * t);", "m.x * s, t * s"):
        assert part in host and part in deep, part
    assert "pm ? 0x3ff00000 : __double2hiint(m.y), __double2loint(m.y)" in deep
    assert "o.y = 1.0 / q;" in host and "o.y = 1.0 / q;" in core and "o.y = m.y * s;" in host and "o.y = m.y * s;" in core
    assert "factor_rule<kRuleAdditive>(o[" not in deep and deep.count("deep_rule(") == 9, "every rule of the deep sweep is deep_rule: its definition and eight calls"


@pytest.mark.parametrize("contract", ("off", "fast"))
def test_one_division_gives_the_bits_of_two(tmp_path, contract):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    flags = ["-O2", "-std=c++17", "-ffp-contract=" + contract]
    if contract == "fast":
        if not _cpu_has_fma():
            pytest.skip("no fused multiply-add on this CPU: the build without contraction is the whole check")
        flags.append("-mfma")
    exe = str(tmp_path / "deep_rule_host")
    subprocess.check_call([cxx] + flags + [SRC, "-o", exe])
    out = subprocess.run([exe, str(N)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.search(r"checked (\d+) point_masses (\d+) mismatches (\d+)", out.stdout)
    assert m and int(m.group(1)) == N + 22 ** 3 and int(m.group(2)) >= N // 5 and int(m.group(3)) == 0, out.stdout[-2000:]
