"""The host forms of poseidon_gl_permute_keep<0/4/8> (the permutation with a four-row last MDS layer), of the sponge that uses them
and of two_to_one (csrc/poseidon_gl.cuh) against oracle/poseidon_gl.py, in a stand-alone program
(tests/poseidon_tail_host/poseidon_tail_host.cpp) built once plain and once with -fsanitize=address,undefined and run directly:
nothing is loaded into Python.  Widths 5, 8, 9, 15, 16, 17, 24, 135, 234 are the smallest that take each branch of the sponge's
rule (final permutation only; exactly one chunk; full then one element; partial then final; ...) plus the two a block uses."""
import os
import random
import shutil
import struct
import subprocess

import pytest

from oracle import poseidon_gl as PG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "poseidon_tail_host", "poseidon_tail_host.cpp")
CXX = os.environ.get("CXX", "g++")
P = PG.P
WIDTHS = [5, 8, 9, 15, 16, 17, 24, 135, 234]


def _fill(kind, n, rng):
    if kind == "random":
        return [rng.randrange(P) for _ in range(n)]
    return [0] * n if kind == "zero" else [P - 1] * n


@pytest.fixture(scope="module")
def vectors(tmp_path_factory):
    """the inputs, the file the program reads and what the oracle says, computed once"""
    rng = random.Random(77)
    states = [_fill("random", 12, rng) for _ in range(6)] + [_fill("zero", 12, rng), _fill("p-1", 12, rng)]
    states += [[rng.choice([0, 1, P - 1, 2**32 - 1, 2**32]) for _ in range(12)] for _ in range(4)]
    inputs = [_fill(kind, w, rng) for w in WIDTHS for kind in ("random", "zero", "p-1")]
    inputs += [_fill("random", w, rng) for w in (0, 1, 4)]            # hash_or_noop's no-op branch
    pairs = [_fill(kind, 8, rng) for kind in ("random", "random", "zero", "p-1")]
    path = tmp_path_factory.mktemp("poseidon_tail_host") / "vectors.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(states)))
        for s in states:
            f.write(struct.pack("<12Q", *s))
        f.write(struct.pack("<Q", len(inputs)))
        for x in inputs:
            f.write(struct.pack("<%dQ" % (1 + len(x)), len(x), *x))
        f.write(struct.pack("<Q", len(pairs)))
        for x in pairs:
            f.write(struct.pack("<8Q", *x))
    want = {"K": [PG.permute(s) for s in states], "H": [PG.hash_or_noop(x) for x in inputs], "T": [PG.two_to_one(x[:4], x[4:]) for x in pairs]}
    return path, want


def _build_and_run(path, flags, name):
    exe = str(path.parent / name)
    if shutil.which(CXX) is None:
        pytest.fail("no host C++ compiler (%s)" % CXX)
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"] + flags + [SRC, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return [ln.split() for ln in r.stdout.splitlines()]


def _check(lines, want):
    seen = {"K": 0, "H": 0, "T": 0}
    for ln in lines:
        tag, i, got = ln[0], int(ln[1]), [int(x) for x in ln[-4:]]
        seen[tag] += 1
        if tag == "K":
            first = int(ln[2])
            assert got == want["K"][i][first:first + 4], ("keep", i, first, "loose" if ln[3] == "1" else "canonical")
        else:
            assert got == want[tag][i], (tag, i, "tail" if ln[2] == "1" else "full")
    assert seen == {"K": 6 * len(want["K"]), "H": 2 * len(want["H"]), "T": 2 * len(want["T"])}


def test_host_forms_equal_the_oracle(vectors):
    path, want = vectors
    _check(_build_and_run(path, ["-O2"], "poseidon_tail_host"), want)


def test_host_forms_under_address_and_undefined_behaviour_sanitizers(vectors):
    path, want = vectors
    _check(_build_and_run(path, ["-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "poseidon_tail_host_san"), want)
