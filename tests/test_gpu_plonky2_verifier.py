"""Native plonky2 verifier on the GPU (zklc_plonky2_verify_batch): the status vector of a batch equals the host path's element for
element -- golden proofs, the tampering matrix, batches of GPU-proved proofs with tampered copies -- and a mainnet Ed25519 proof
passes Prover.verify."""
import json
import os
import random

import pytest

import zklc_amd  # noqa: F401
from zklc_amd.plonky2 import serialization as S, HASH_GL, HASH_BN128
from zklc_amd.plonky2.verifier import Verifier, ProofRejected, PROOF_OK, PROOF_BAD_VANISHING
from conftest import GOLDEN
from test_plonky2_verifier_host import TAMPERS, golden, tamper, _synthetic, vanishing_case

pytestmark = pytest.mark.gpu


def test_gpu_equals_host_on_golden_and_tampering_matrix(zctx):
    cases = golden()
    c0 = cases[0]
    with Verifier(zctx, c0["common_data"], c0["verifier_data"]) as v:
        batch = [S.proof_to_bytes(c0["proof"], c0["common_data"], HASH_BN128)]
        for what in TAMPERS:
            batch.append(S.proof_to_bytes(tamper(c0["proof"], c0["common_data"], c0["verifier_data"], what), c0["common_data"],
                                          HASH_BN128))
        got, want = v.verify_batch(batch), v.verify_batch_host(batch)
        assert got == want and got[0] == PROOF_OK and all(s != PROOF_OK for s in got[1:]), (got, want)
        # a second call of the same size reuses the verifier's buffers and gives the same answer
        assert v.verify_batch(batch) == got
    for c in cases[1:]:
        with Verifier(zctx, c["common_data"], c["verifier_data"]) as v:
            assert v.verify_batch([c["proof"]]) == [PROOF_OK], c["source"]


def _tampered_bytes(raw, common, vd, hasher, what):
    return S.proof_to_bytes(tamper(S.proof_from_bytes(raw, common, hasher), common, vd, what), common, hasher)


@pytest.mark.parametrize("shape,degree_bits,hasher", [("recursion", 12, HASH_GL), ("recursion", 12, HASH_BN128), ("ed25519", 13, HASH_GL)])
def test_gpu_proved_batches(zctx, shape, degree_bits, hasher):
    """batches of 1, 65 and 128 proofs of one GPU-proved circuit: byte copies of a proof, tampered copies at seeded random
    positions; GPU statuses == host statuses, the untampered ones 0"""
    data, wires, pis = _synthetic(shape, degree_bits, seed=5, npi=16)
    common = data.common_data()
    prover = data.prover(zctx, hasher)
    good = [prover.prove_bytes(wires, pis)]
    vd = prover.verifier_data()
    kinds = ["initial_leaf", "step_eval_within", "step_eval_other", "initial_sibling", "pow_witness", "non_canonical"]
    bad = {k: _tampered_bytes(good[0], common, vd, hasher, k) for k in kinds}
    rng = random.Random(11)
    with Verifier.from_prover(prover) as v:
        for n in (1, 65, 128):
            batch, valid = [], []
            for i in range(n):
                if n > 1 and rng.random() < 0.3:
                    batch.append(bad[rng.choice(kinds)])
                    valid.append(False)
                else:
                    batch.append(good[0])
                    valid.append(True)
            got = v.verify_batch(batch)
            assert got == v.verify_batch_host(batch), n
            assert all((s == PROOF_OK) == ok for s, ok in zip(got, valid)), (n, got)
    prover.close()


def test_gpu_vanishing_proof_in_a_batch(zctx):
    """the CPU tests' VANISHING case re-made by the GPU prover, in a batch with valid and tampered proofs of its circuit: the
    proofs the host stage rejects (VANISHING, POW, FORMAT) sit beside proofs that go through the kernels"""
    provers = []

    def prove(d, w, p):
        pr = d.prover(zctx, HASH_GL)
        provers.append(pr)
        return pr.prove_bytes(w, p), pr.verifier_data()
    data, vd, raw = vanishing_case(prove)
    wires, pis = _synthetic("recursion", 6, seed=4)[1:]
    good = provers[-1].prove_bytes(wires, pis)
    common = data.common_data()
    kinds = ["pow_witness", "non_canonical", "initial_leaf", "step_eval_within"]
    batch = [good, raw] + [_tampered_bytes(good, common, vd, HASH_GL, k) for k in kinds] + [raw, good]
    with Verifier(zctx, common, vd) as v:
        got = v.verify_batch(batch)
        assert got == v.verify_batch_host(batch)
        assert got[0] == got[-1] == PROOF_OK and got[1] == got[-2] == PROOF_BAD_VANISHING
        assert all(st != PROOF_OK for st in got[2:-2]), got
    for pr in provers:
        pr.close()


@pytest.mark.parametrize("hasher", [HASH_GL, HASH_BN128])
def test_verifier_from_circuit_equals_explicit_arguments(zctx, hasher):
    """zklc_plonky2_verifier_create_from_circuit (cap and digest from the circuit's commitment) and zklc_plonky2_verifier_create
    from the common data and verifier_only JSON give the same verdicts"""
    data, wires, pis = _synthetic("recursion", 6, seed=9)
    prover = data.prover(zctx, hasher)
    raw = prover.prove_bytes(wires, pis)
    common, vd = data.common_data(), prover.verifier_data()
    batch = [raw] + [_tampered_bytes(raw, common, vd, hasher, k) for k in ("initial_leaf", "step_eval_within", "public_input")]
    with Verifier.from_prover(prover) as a, Verifier(None, json.loads(json.dumps(common)), json.loads(json.dumps(vd))) as b:
        assert a.proof_bytes == b.proof_bytes == prover.proof_bytes
        got = a.verify_batch(batch)
        assert got == a.verify_batch_host(batch) == b.verify_batch(batch) and got[0] == PROOF_OK
        assert all(st != PROOF_OK for st in got[1:])
    prover.close()


def test_primitive_prover_verify_flag(zctx):
    """PrimitiveProver(ctx, verify=True) checks its proofs where the reference calls data.verify (primitives.rs:110,160) and
    returns the same proof as without the flag"""
    from zklc_amd.primitives import PrimitiveProver
    h1, h2 = (105971807).to_bytes(8, "little"), (105971806).to_bytes(8, "little")
    plain = PrimitiveProver(zctx)
    checked = PrimitiveProver(zctx, verify=True)
    a = plain.prove_consecutive_heights(h1, h2)
    b = checked.prove_consecutive_heights(h1, h2)
    assert a == b
    prover = checked._cache["heights"][2]
    assert prover._verifier is not None        # the flag did run the verifier
    plain.close()
    checked.close()


def test_mainnet_ed25519_proof(zctx, approval_prover):
    """one Ed25519-circuit proof (2^18 x 234) of a NEAR mainnet signature passes Prover.verify; one byte changed in its wires
    opening is rejected"""
    j = json.load(open(os.path.join(GOLDEN, "ed25519_near_c1_small.json")))
    msg = bytes.fromhex(j["msg"])
    e = j["entries"][0]
    pk, sig = bytes.fromhex(e["validator_tail"])[1:33], bytes.fromhex(e["approval"])[2:]
    (common, vd, raw), = approval_prover.ed25519_proofs(msg, [sig], [pk])
    prover = approval_prover.ed25519_circuit(len(msg))[2]
    prover.verify(raw)
    sh = S.shapes(common)
    off = 3 * sh["cap"] * 32 + 16 * (common["num_constants"] + common["config"]["num_routed_wires"]) + 16 * 5
    bad = bytearray(raw)
    bad[off] ^= 1
    with pytest.raises(ProofRejected) as ei:
        prover.verify(bytes(bad))
    assert ei.value.status != PROOF_OK


def test_block_hash_prover_verify_flag(zctx):
    """BlockHashProver(ctx, verify=True).prove_header_hash checks its proof where the reference calls data.verify
    (header_bphash.rs:94); the native verifier ran and accepts the proof it returned"""
    import hashlib
    from zklc_amd.header_bphash import BlockHashProver
    bp = BlockHashProver(zctx, verify=True)
    prev_hash = hashlib.sha256(b"prev").digest()
    inner_lite = bytes((5 * i + 1) & 0xFF for i in range(208))
    inner_rest = bytes((3 * i + 2) & 0xFF for i in range(330))
    inner = hashlib.sha256(hashlib.sha256(inner_lite).digest() + hashlib.sha256(inner_rest).digest()).digest()
    header_hash = hashlib.sha256(inner + prev_hash).digest()
    common, vd, proof = bp.prove_header_hash(header_hash, prev_hash, inner_lite, inner_rest)
    assert len(bp._verifiers) == 1
    with Verifier(zctx, common, vd) as v:
        assert v.verify_batch([proof]) == [PROOF_OK]
    bp.close()
