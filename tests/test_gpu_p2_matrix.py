"""The parameter matrix of tests/p2_matrix_cases.py on the GPU: for every case the GPU prover's bytes and verifier data equal the
oracle's C prover's, and the GPU verifier gives the C prover's proof and its tampered copies the statuses of the host path
(which tests/test_p2_matrix_host.py pins to the verifier restatement).  The same under Poseidon-BN128 for every case of at most
2^11 rows and for 2^12 and 2^13 rows (the wrap's size, and one above it), four cases again under Poseidon-BN128 against the Python
prover restatement, the configuration with three challenges at the library's edges, and four cases with ZKLC_LEAN_ARITH=0."""
import hashlib
import os
import subprocess
import sys

import pytest

import zklc_amd
from zklc_amd.plonky2 import serialization as S, HASH_GL, HASH_BN128
from zklc_amd.plonky2.verifier import Verifier, PROOF_OK
from oracle import plonky2_prover as OP, plonky2_verifier as V
import p2_matrix_cases as M

pytestmark = pytest.mark.gpu


def _verifier_half(v, batch):
    """the good proof and its tampered copies, then the same batch repeated to 65 entries (more than one wave of lanes)"""
    for proofs in (batch, (batch * (65 // len(batch) + 1))[:65]):
        got, want = v.verify_batch(proofs), v.verify_batch_host(proofs)
        assert got == want, (got, want)
        for i, st in enumerate(got):
            assert (st == PROOF_OK) == (i % len(batch) == 0), (i, got)


def _prover_and_verifier(zctx, case, hasher):
    data, wires, pis = M.make(case)
    want, vd = M.reference(case, hasher)
    prover = data.prover(zctx, hasher)
    problems = []
    try:
        try:
            got = prover.prove_bytes(wires, pis)
            if got != want:
                problems.append("proof bytes differ from the C prover's")
            if prover.prove_bytes(wires, pis) != got:
                problems.append("a second prove_bytes gives other bytes")
        except zklc_amd.ZklcError as e:
            problems.append("prove_bytes: %s" % e)
        if prover.verifier_data() != vd:
            problems.append("verifier data differs from the C prover's")
        # the verifier half takes its proofs from the C prover: it says something even where the prover half has failed
        with Verifier.from_prover(prover) as v:
            _verifier_half(v, M.batch(case, hasher))
    finally:
        prover.close()
    assert not problems, (case.name, data.fri_arity_bits, problems)


@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c.name)
def test_prover_and_verifier_match_the_references(zctx, case):
    _prover_and_verifier(zctx, case, HASH_GL)


@pytest.mark.parametrize("case", M.BN128_C_CASES, ids=lambda c: c.name)
def test_poseidon_bn128_prover_and_verifier_match_the_c_prover(zctx, case):
    """PoseidonBN128GoldilocksConfig: the Merkle caps, and with them every challenge, differ from the Goldilocks configuration's, so
    every stage upstream of the hash runs on other data here.  Proof bytes, a second prove_bytes, the verifier data, and the
    verifier's statuses for the C prover's proof and its tampered copies."""
    _prover_and_verifier(zctx, case, HASH_BN128)


@pytest.mark.parametrize("case", M.BN128_CASES, ids=lambda c: c.name)
def test_poseidon_bn128_matches_the_python_restatement(zctx, case):
    """no C prover under Poseidon-BN128: the Python prover restatement, as test_all_gate_types_match_oracle_bit_for_bit"""
    data, wires, pis = M.make(case)
    common = data.common_data()
    oproof, ovd = OP.prove(common, data.constants, data.sigmas, wires, pis, V.HasherBN128)
    want = S.proof_to_bytes(oproof, common, HASH_BN128)
    prover = data.prover(zctx, HASH_BN128)
    try:
        assert prover.verifier_data() == ovd
        got = prover.prove_bytes(wires, pis)
        assert got == want
        assert prover.prove_bytes(wires, pis) == got
        with Verifier.from_prover(prover) as v:
            _verifier_half(v, [want] + [M.tampered(want, common, ovd, k, HASH_BN128) for k in M.kinds(case)])
    finally:
        prover.close()


def test_three_challenges(zctx):
    """P2_MAX_CH is 2: the prover refuses a configuration with three challenges when the circuit is created; the verifier, whose
    host stage and kernels take the number from the circuit, gives the C prover's proofs the host path's statuses"""
    case = M.THREE_CHALLENGES
    data = M.make(case)[0]
    with pytest.raises(zklc_amd.ZklcError):
        data.prover(zctx, HASH_GL)
    with Verifier(zctx, data.common_data(), M.reference(case)[1]) as v:
        _verifier_half(v, M.batch(case))


_CHILD = r'''
import hashlib, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import zklc_amd
from zklc_amd.plonky2 import HASH_GL
import p2_matrix_cases as M
with zklc_amd.Context(0) as ctx:
    for case in M.LEAN_OFF_CASES:
        data, wires, pis = M.make(case)
        prover = data.prover(ctx, HASH_GL)
        print("DIGEST %%s %%s" %% (case.name, hashlib.sha256(prover.prove_bytes(wires, pis)).hexdigest()))
        prover.close()
'''


def test_proof_bytes_with_the_lean_arithmetic_switched_off():
    """The library reads ZKLC_LEAN_ARITH once per process: one fresh child with ZKLC_LEAN_ARITH=0 proves the [2,2,2] arities, the
    cap of height 0, 73 routed wires and the combined case; every digest must be the C prover's."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    want = {case.name: hashlib.sha256(M.reference(case)[0]).hexdigest() for case in M.LEAN_OFF_CASES}
    code = _CHILD % {"root": root, "tests": os.path.join(root, "tests")}
    env = dict(os.environ, ZKLC_LEAN_ARITH="0")
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=root, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    got = dict(ln.split()[1:3] for ln in run.stdout.splitlines() if ln.startswith("DIGEST "))
    assert got == want, "proof bytes under ZKLC_LEAN_ARITH=0 differ from the C prover's"
