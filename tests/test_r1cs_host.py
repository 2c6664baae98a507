"""zklc_r1cs_create / zklc_r1cs_abc_host (no GPU): the validation of the caller's CSR and the host twin of the evaluation kernels --
the lane functions of csrc/r1cs_eval.cuh compiled for the host -- against Python integers (tests/r1cs_cases.py), byte for byte."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import r1cs_cases as C
from conftest import ROOT
from oracle import groth16 as G
from zklc_amd import _lib
from zklc_amd.groth16 import fr_to_mont_words
from zklc_amd.r1cs import BIN_LIMITS, R, R1CS

INVALID = -1          # ZKLC_ERR_INVALID_ARG


def _equal(got, want, what):
    for name, g, w in zip("abc", got[:3], want[:3]):
        bad = np.nonzero((np.asarray(g) != w).any(axis=1))[0]
        assert len(bad) == 0, "%s: row %d of %s is %s, expected %s" % (what, bad[0], name, g[bad[0]], w[bad[0]])
        assert np.asarray(g).tobytes() == w.tobytes()
    assert got[3] == want[3], what + ": summary"


def test_bin_limits_are_the_kernels():
    src = open(os.path.join(ROOT, "zk-light-client-implementation_amd", "csrc", "r1cs_eval.cuh")).read()
    assert "#define R1CS_BIN0_MAX %du" % BIN_LIMITS[0] in src and "#define R1CS_BIN1_MAX %du" % BIN_LIMITS[1] in src
    assert 1 <= BIN_LIMITS[0] < BIN_LIMITS[1]


def test_edge_system_has_every_case():
    s = C.edge_system()
    lens = [len(r) for r in s.rows]
    for want in [0, 1, 64, 65, 129] + [b + d for b in BIN_LIMITS for d in (0, 1)]:
        assert want in lens
    assert max(lens) >= 1000
    assert any(len({w for w, _ in r}) < len(r) for r in s.rows)                      # a wire repeated inside a row
    used = {s.values[c] for r in s.rows for _, c in r}
    assert {0, 1, R - 1, 2, R - 2} <= used and len(used) > 8
    assert {0, 1, R - 1} <= set(s.witness)
    assert len(set(s.values)) < len(s.values)                                        # two ids, one value
    v = s.row_values(s.witness)
    nc = s.n_constraints
    assert all((v[j] * v[nc + j] - v[2 * nc + j]) % R == 0 for j in range(nc))       # satisfied by construction
    assert 0 in v[:nc] and (R - 1) * (R - 1) % R in v[:nc]


@pytest.mark.parametrize("nthreads", [1, 3, 0])
def test_host_twin_equals_python_on_the_edge_system(nthreads):
    s = C.edge_system()
    n = 2 * C.domain_size(s.n_constraints)                                           # n > n_constraints: the padding is written
    _, w, *want = C.expected_cached("edge", 0, n)
    sys_ = R1CS.from_csr(*s.csr())
    _equal(sys_.abc_host(C.witness_words(w), n, check=True, nthreads=nthreads), want, "edge system")
    a, b, c, summary = sys_.abc_host(C.witness_words(w), n, nthreads=nthreads)       # without the check: the same words, no summary
    _equal((a, b, c, want[3]), want, "edge system, unchecked")
    assert summary is None
    sys_.close()


@pytest.mark.parametrize("nthreads", [1, 3, 0])
@pytest.mark.parametrize("nc", [1, 2, 300])
def test_host_twin_equals_python_on_random_systems(nc, nthreads):
    s = C.random_system(nc)
    n = C.domain_size(nc) + 3                                                        # the library does not ask for a power of two
    _, w, *want = C.expected_cached("random", nc, n)
    sys_ = R1CS.from_csr(*s.csr())
    _equal(sys_.abc_host(C.witness_words(w), n, check=True, nthreads=nthreads), want, "nc = %d" % nc)
    # n = n_constraints: no padding at all
    _, _, *want0 = C.expected_cached("random", nc, nc)
    _equal(sys_.abc_host(C.witness_words(w), nc, check=True, nthreads=nthreads), want0, "nc = %d, n = nc" % nc)


def test_outputs_are_written_in_full():
    """the caller's buffers are not assumed clear: 0xFF everywhere before the call, through the raw ABI"""
    s = C.edge_system()
    n = s.n_constraints + 5
    _, w, ea, eb, ec, _ = C.expected_cached("edge", 0, n)
    sys_ = R1CS.from_csr(*s.csr())
    a, b, c = (np.full((n, 4), (1 << 64) - 1, dtype=np.uint64) for _ in range(3))
    ww = C.witness_words(w)
    rc = sys_._lib.zklc_r1cs_abc_host(sys_._s, ww.ctypes.data, n, a.ctypes.data, b.ctypes.data, c.ctypes.data, 0, 3, None)
    assert rc == 0
    assert a.tobytes() == ea.tobytes() and b.tobytes() == eb.tobytes() and c.tobytes() == ec.tobytes()


def test_unreduced_witness_words_are_reduced():
    s = C.random_system(300)
    n = 512
    _, w, *want = C.expected_cached("random", 300, n)
    big = [x + R if i % 3 == 0 else x for i, x in enumerate(w)]                       # < 2 r < 2^256: still four words
    words = np.array([[(x >> (64 * i)) & ((1 << 64) - 1) for i in range(4)] for x in big], dtype=np.uint64)
    _equal(R1CS.from_csr(*s.csr()).abc_host(words, n, check=True), want, "witness + r")


def test_from_rows_equals_the_oracle():
    r1cs, wit = G.square_chain_r1cs(20)
    w = wit([5, 6], 9)
    n_wires = len(w)
    sys_ = R1CS.from_rows(*r1cs, n_wires)
    assert sys_.n_coeff == 3                                                         # 1, r - 1, r - 3: the dictionary has no duplicates
    n = G.domain_size(20)
    want = G.abc_evaluations(r1cs, w, n)
    a, b, c, summary = sys_.abc_host(C.witness_words(w), n, check=True)
    for got, exp in zip((a, b, c), want):
        assert got.tolist() == [fr_to_mont_words(x) for x in exp]
    assert summary == (0, None)
    w[-1] = (w[-1] + 1) % R
    assert sys_.abc_host(C.witness_words(w), n, check=True)[3] == (1, 19)


@pytest.mark.parametrize("kind,arg", [("edge", 0), ("random", 300)])
def test_summaries_of_broken_witnesses(kind, arg):
    s = C.edge_system() if kind == "edge" else C.random_system(arg)
    nc = s.n_constraints
    n = C.domain_size(nc)
    sys_ = R1CS.from_csr(*s.csr())
    fresh = [j for j in range(nc) if any(w == s.fresh_wire(j) for w, _ in s.rows[2 * nc + j])]
    assert fresh[0] == 0 and fresh[-1] == nc - 1
    for broken in [(), (0,), (nc - 1,), (0, nc - 1), tuple(fresh[1:-1:3]), tuple(fresh)]:
        _, w, *want = C.expected_cached(kind, arg, n, broken)
        assert want[3] == (len(broken), broken[0] if broken else None)               # the expectation is the construction's
        _equal(sys_.abc_host(C.witness_words(w), n, check=True, nthreads=3), want, "broken at %s" % (broken,))


# ---- validation: one case per condition of include/zklc.h, through the raw ABI (the Python wrapper compares lengths itself)
def _create(nc, n_wires, row_ptr, wire, coeff, nnz, coeffs, n_coeff):
    lib = _lib.load()
    row_ptr, coeffs = np.array(row_ptr, dtype=np.uint64), np.array(coeffs, dtype=np.uint64)
    wire, coeff = np.array(wire, dtype=np.uint32), np.array(coeff, dtype=np.uint32)
    h = ctypes.c_void_p(1)
    rc = lib.zklc_r1cs_create(None, nc, n_wires, row_ptr.ctypes.data, wire.ctypes.data, coeff.ctypes.data, nnz, coeffs.ctypes.data,
                              n_coeff, ctypes.byref(h))
    if rc == 0:
        lib.zklc_r1cs_destroy(h)
    else:
        assert not h.value, "a failed create leaves no handle"
    return rc


ONE = fr_to_mont_words(1)
R_WORDS = [(R >> (64 * i)) & ((1 << 64) - 1) for i in range(4)]
TINY = dict(nc=2, n_wires=2, row_ptr=[0, 1, 2, 3, 3, 4, 4], wire=[0, 1, 0, 0], coeff=[0, 0, 0, 0], nnz=4, coeffs=ONE, n_coeff=1)
MALFORMED = {
    "n_constraints = 2^62, four-entry arrays": dict(nc=1 << 62),
    "3 n_constraints + 1 wraps to 3": dict(nc=((1 << 64) + 2) // 3),
    "nnz = 2^62": dict(nnz=1 << 62),
    "n_coeff above 2^30": dict(n_coeff=(1 << 30) + 1),
    "n_wires = 0": dict(n_wires=0),
    "n_wires above 2^32": dict(n_wires=(1 << 32) + 1),
    "row_ptr[0] != 0": dict(row_ptr=[1, 1, 2, 3, 3, 4, 4]),
    "row_ptr decreasing in the middle": dict(row_ptr=[0, 1, 2, 1, 3, 4, 4]),
    "row_ptr beyond nnz in the middle": dict(row_ptr=[0, 1, 2, 1 << 63, 3, 4, 4]),
    "last entry below nnz": dict(row_ptr=[0, 1, 2, 3, 3, 3, 3]),
    "last entry above nnz": dict(row_ptr=[0, 1, 2, 3, 3, 4, 5]),
    "wire = n_wires": dict(wire=[0, 1, 0, 2]),
    "coefficient id = n_coeff": dict(coeff=[0, 1, 0, 0]),
    "coefficient = r": dict(coeffs=R_WORDS),
    "coefficient = 2^256 - 1": dict(coeffs=[(1 << 64) - 1] * 4),
}


def test_the_well_formed_tiny_system_is_accepted():
    assert _create(**TINY) == 0
    assert _create(**dict(TINY, coeffs=[R_WORDS[0] - 1] + R_WORDS[1:])) == 0         # r - 1 is a coefficient
    assert _create(**dict(TINY, nc=0, row_ptr=[0], wire=[], coeff=[], nnz=0)) == 0   # no constraint at all


@pytest.mark.parametrize("what", sorted(MALFORMED))
def test_malformed_systems_are_rejected(what):
    assert (3 * (((1 << 64) + 2) // 3) + 1) % (1 << 64) == 3
    assert _create(**dict(TINY, **MALFORMED[what])) == INVALID


def test_malformed_calls_are_rejected():
    s = C.random_system(2)
    sys_ = R1CS.from_csr(*s.csr())
    lib, h = sys_._lib, sys_._s
    w = C.witness_words(s.witness)
    n = 4
    buf = np.zeros((3, n + 1, 4), dtype=np.uint64)
    a, b, c = (buf[i].ctypes.data for i in range(3))
    summary = np.zeros(2, dtype=np.uint64)
    call = lambda *args: lib.zklc_r1cs_abc_host(h, *args)
    assert call(w.ctypes.data, n, a, b, c, 1, 1, summary.ctypes.data) == 0
    assert call(w.ctypes.data, 1, a, b, c, 0, 1, None) == INVALID                    # n < n_constraints
    assert call(w.ctypes.data, n, a, b, c, 2, 1, summary.ctypes.data) == INVALID     # unknown flag bits
    assert call(w.ctypes.data, n, a, b, c, 1, 1, None) == INVALID                    # check without a summary
    assert call(None, n, a, b, c, 0, 1, None) == INVALID                             # missing pointers
    assert call(w.ctypes.data, n, a, None, c, 0, 1, None) == INVALID
    assert call(w.ctypes.data + 8, n, a, b, c, 0, 1, None) == INVALID                # misaligned pointers
    assert call(w.ctypes.data, n, a, b, c + 8, 0, 1, None) == INVALID
    assert lib.zklc_r1cs_abc_host(None, w.ctypes.data, n, a, b, c, 0, 1, None) == INVALID
    assert sys_.workspace_bytes() == 32 * s.n_wires
    with pytest.raises(ValueError):
        R1CS.from_csr(2, 2, [0, 1], [0], [0], [ONE])                                 # lengths that contradict the sizes: Python's check
    sys_.close()
    with pytest.raises(ValueError):
        sys_.abc_host(w, n)


# ---- the host file on its own, under the sanitizers
def _write_case_file(path, s, n, brokens):
    with open(path, "wb") as f:
        f.write(np.array([s.n_constraints, s.n_wires, s.nnz, s.coeffs.shape[0], n, len(brokens) - 1], dtype=np.uint64).tobytes())
        f.write(s.row_ptr.tobytes())
        for arr in (s.term_wire, s.term_coeff):
            f.write(arr.tobytes() + b"\0" * (4 * (s.nnz % 2)))
        f.write(s.coeffs.tobytes())
        for broken in brokens:
            _, w, a, b, c, (count, first) = C.expected_cached("edge", 0, n, broken)
            f.write(C.witness_words(w).tobytes() + a.tobytes() + b.tobytes() + c.tobytes())
            f.write(np.array([count, (1 << 64) - 1 if first is None else first], dtype=np.uint64).tobytes())


def test_the_host_file_links_alone_and_is_clean_under_the_sanitizers(tmp_path):
    """csrc/r1cs_eval_host.cpp + tests/r1cs_host/r1cs_host_main.cpp and nothing else, g++ -fsanitize=address,undefined, as a child
    process: every malformed input (arrays exactly as long as they claim) and the edge system, satisfied and broken"""
    s = C.edge_system()
    n = C.domain_size(s.n_constraints)
    case = str(tmp_path / "edge.bin")
    _write_case_file(case, s, n, [(), (0,), (s.n_constraints - 1,), (0, 7, s.n_constraints - 1)])
    exe = str(tmp_path / "r1cs_host_main")
    src = [os.path.join(ROOT, "tests", "r1cs_host", "r1cs_host_main.cpp"),
           os.path.join(ROOT, "zk-light-client-implementation_amd", "csrc", "r1cs_eval_host.cpp")]
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                         "-pthread", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"] + src + ["-o", exe],
                        capture_output=True, text=True, timeout=600)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe, case], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "r1cs host: ok" in run.stdout, (run.stdout + run.stderr)[-3000:]
