"""The host form of p2_eval_poseidon_stmt (csrc/plonky2_gates.cuh: the evaluator of ZKLC_P2_POSEIDON_GATE=stmt with its steps in
plain C++) against the plain evaluator and the oracle, in a stand-alone program (tests/poseidon_gate_host/poseidon_gate_host.cpp),
built once plain and once with -fsanitize=address,undefined and run directly: nothing is loaded into Python."""
import os
import shutil
import struct
import subprocess

import pytest

import poseidon_gate_vectors as PV
from oracle import plonky2_gates as OG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "poseidon_gate_host", "poseidon_gate_host.cpp")
CXX = os.environ.get("CXX", "g++")


@pytest.fixture(scope="module")
def rows_file(tmp_path_factory):
    rows, alphas = PV.rows(), PV.alphas()
    path = tmp_path_factory.mktemp("poseidon_gate_host") / "rows.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(rows)))
        for expect, r in rows:
            f.write(struct.pack("<136Q", expect, *r))
        f.write(struct.pack("<Q", len(alphas)))
        for a in alphas:
            f.write(struct.pack("<2Q", *a))
    return path, rows, alphas


def _build_and_run(rows_file, flags, name):
    path = rows_file[0]
    exe = str(path.parent / name)
    if shutil.which(CXX) is None:
        pytest.fail("no host C++ compiler (%s)" % CXX)
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"] + flags + [SRC, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return [[int(x) for x in ln.split()] for ln in r.stdout.splitlines()]


def test_host_form_equals_the_plain_evaluator_and_the_oracle(rows_file):
    _, rows, alphas = rows_file
    assert len(rows) == 144 and sorted({65 + (k if k < 22 else 21 * (k - 22)) for k in range(24)}) == list(range(65, 87))
    got = _build_and_run(rows_file, ["-O2"], "poseidon_gate_host")
    assert len(got) == len(rows) * len(alphas)
    from zklc_amd.plonky2 import gates as G
    og = OG.gate_from_id(G.PoseidonGate().id())
    res = {(i, p): (a0, a1) for i, p, a0, a1 in got}
    for i, (expect, r) in enumerate(rows):
        cs = og.eval(OG.BaseK, [], r, [0] * 4)
        assert len(cs) == 123
        for p, al in enumerate(alphas):
            assert list(res[(i, p)]) == [OG.reduce_with_powers(OG.BaseK, cs, a) for a in al], (i, p)
        if expect:
            assert all(c == 0 for c in cs) == (expect == 1), i


def test_host_form_under_address_and_undefined_behaviour_sanitizers(rows_file):
    _, rows, alphas = rows_file
    got = _build_and_run(rows_file, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "poseidon_gate_host_san")
    assert len(got) == len(rows) * len(alphas)
