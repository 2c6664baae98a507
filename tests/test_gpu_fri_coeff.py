"""The FRI opening combination formed on coefficients (csrc/plonky2_fri_combine.cuh; the default whenever the lean arithmetic is on).
Part 1: p2_fri_coeff_combine_kernel alone (tests/fri_coeff_dev) over the cases of tests/fri_coeff_host/fri_coeff_cases.h -- total
widths 1, 15, 16, 17, 383, 384, 385, 400, as one matrix and spread over the four batches, n = 2^3 and 2^9 -- against a plain Horner
sum over the extension field.  Part 2: proof bytes -- one child process per setting (the switches are read once per process) proves
the 2^13 x 234 slice of the Ed25519 shape, the Poseidon-heavy 2^12 x 135, the 2^5 circuit with 77 routed wires (n below one
workgroup), the smallest size the matrix accepts (2^2) and one Poseidon-BN128-capped case; every setting must give the C prover's
bytes (the first FRI cap inside them commits to every element of the combination), and every child reports which form it ran.

The library keeps every batch's coefficients in natural order; ZKLC_P2_COEFF_ORDER is not read by it, so the two settings that
name it run the default order -- they are listed so that the matrix of settings is the one the combination has to hold under."""
import ctypes
import hashlib
import importlib
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = [1, 15, 16, 17, 383, 384, 385, 400]


@pytest.fixture(scope="module")
def dev():
    import zklc_amd  # noqa: F401  (first: the package's hardware-queue setting applies to this process)
    b = importlib.import_module("zk-light-client-implementation_amd.build")
    if os.path.exists(b.HIPCC) and not b.fri_coeff_dev_is_current():
        b.build_fri_coeff_dev(verbose=False)
    if not os.path.exists(b.FCD_LIB):
        pytest.fail("tests/fri_coeff_dev/libfri_coeff_dev.so is missing and there is no hipcc to build it: run __graft_entry__.build()")
    lib = ctypes.CDLL(b.FCD_LIB)
    lib.fcd_run_case.restype = ctypes.c_int
    lib.fcd_run_case.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int]
    return lib


@pytest.mark.parametrize("log_n", [3, 9])
@pytest.mark.parametrize("spread", [0, 1], ids=["single", "spread"])
def test_kernel_equals_the_horner_sum(dev, log_n, spread):
    for w in WIDTHS:
        assert dev.fcd_run_case(w, log_n, spread) == 0, (w, log_n, spread)


# ------------------------------------------------------------------------------------------------ proof bytes
SETTINGS = [({}, "coefficients"),
            ({"ZKLC_P2_FRI_COMBINE": "points"}, "points"),
            ({"ZKLC_P2_COEFF_ORDER": "natural"}, "coefficients"),
            ({"ZKLC_P2_FRI_COMBINE": "points", "ZKLC_P2_COEFF_ORDER": "natural"}, "points"),
            ({"ZKLC_LEAN_ARITH": "0"}, "points, as it was")]


def circuits():
    """-> [(name, (data, wires, public inputs), hasher)]"""
    from zklc_amd.plonky2 import HASH_GL, HASH_BN128
    from test_gpu_poseidon_gate_stmt import circuits as two
    from test_gpu_lean_arith import partial_chunk_circuit
    import p2_matrix_cases as M
    ed, rec = two()
    smallest = min(M.CASES, key=lambda c: c.degree_bits)
    assert smallest.degree_bits == 2
    return [(ed[0], ed[1], HASH_GL), (rec[0], rec[1], HASH_GL), ("partial_2p5x77", partial_chunk_circuit(), HASH_GL),
            (smallest.name, M.make(smallest), HASH_GL), ("cap-0-bn128", M.make(M.BY_NAME["cap-0"]), HASH_BN128)]


_CHILD = r'''
import hashlib, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import zklc_amd
from test_gpu_fri_coeff import circuits
with zklc_amd.Context(0) as ctx:
    for name, (data, wires, pis), hasher in circuits():
        prover = data.prover(ctx, hasher)
        print("DIGEST " + name + " " + hashlib.sha256(prover.prove_bytes(wires, pis)).hexdigest())
        prover.close()
'''


def test_every_setting_gives_the_c_provers_bytes(zctx):
    from oracle import cport
    code = _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    keys = sorted({k for s, _ in SETTINGS for k in s} | {"ZKLC_P2_DEBUG"})
    procs = []
    for s, form in SETTINGS:     # five children: with this process six of the processes that may have the GPU open at once
        env = {k: v for k, v in os.environ.items() if k not in keys}
        env.update(s)
        env["ZKLC_P2_DEBUG"] = "1"      # the library names the form of the combination once per circuit
        procs.append((s, form, subprocess.Popen([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                                                env=env, cwd=ROOT)))
    try:
        want = {}                # the C prover's bytes, computed on the host while the children prove
        for name, (data, wires, pis), hasher in circuits():
            want[name] = hashlib.sha256(cport.plonky2_prove(data, wires, pis, hasher=hasher)[0]).hexdigest()
        assert len(want) == 5
        for s, form, p in procs:
            so, se = p.communicate(timeout=600)
            assert p.returncode == 0, (s, se[-2000:])
            got = dict(ln.split()[1:3] for ln in so.splitlines() if ln.startswith("DIGEST "))
            assert got == want, "proof bytes under %r differ from the C prover's" % (s,)
            forms = [ln.split(": ", 1)[1] for ln in se.splitlines() if ln.startswith("[zklc] fri combine: ")]
            assert forms == [form] * len(want), (s, forms)
    finally:
        for _, _, p in procs:    # nothing is left running when an assertion or the host prover fails
            if p.poll() is None:
                p.kill()
                p.wait()
