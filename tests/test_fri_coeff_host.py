"""The host form of the coefficient-form FRI combination (csrc/plonky2_fri_combine.cuh: p2_fri_coeff_lane, the body of
p2_fri_coeff_combine_kernel, and p2_fri_finish_lane) against a plain Horner sum over the extension field, in a stand-alone program
(tests/fri_coeff_host/fri_coeff_host.cpp) built once plain and once with -fsanitize=address,undefined and run directly: nothing is
loaded into Python.  Total widths 1, 15, 16, 17, 383, 384, 385 and 400 (the sixteen-wide load batch, the fold of the limb columns
every 384 terms), each as one matrix and spread over four, at n = 2^3 and 2^9."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "fri_coeff_host", "fri_coeff_host.cpp")
CXX = os.environ.get("CXX", "g++")
WIDTHS = [1, 15, 16, 17, 383, 384, 385, 400]


def _build_and_run(tmp_path, flags, name):
    exe = str(tmp_path / name)
    if shutil.which(CXX) is None:
        pytest.fail("no host C++ compiler (%s)" % CXX)
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"] + flags + [SRC, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    cases = [ln for ln in lines if ln.startswith("width ")]
    assert len(cases) == len(WIDTHS) * 2 * 2 and all(ln.endswith(": 0 differ") for ln in cases), cases
    assert sorted({int(ln.split()[1]) for ln in cases}) == WIDTHS and {int(ln.split()[-3][:-1]) for ln in cases} == {8, 512}
    assert lines[-1] == "finish: 16 points, 0 differ"


def test_host_form_equals_the_horner_sum(tmp_path):
    _build_and_run(tmp_path, ["-O2"], "fri_coeff_host")


def test_host_form_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    _build_and_run(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "fri_coeff_host_san")
