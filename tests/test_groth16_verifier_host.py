"""The native batched Groth16 verifier (zklc_groth16_verify_batch_host, include/zklc.h; zklc_amd.groth16.NativeGroth16Verifier) on
its host path -- the lane functions of csrc/groth16_verify.cuh compiled for the host, the same ones the kernels run.  Every
expected status is the independent classification of tests/groth16_cases.py (oracle.bn254 + oracle.groth16.verify)."""
import random

import pytest

import groth16_cases as C
from oracle import bn254 as B
from zklc_amd import formats as F
from zklc_amd.groth16 import NativeGroth16Verifier, ProofRejected, G16_STATUS_NAMES


@pytest.fixture(scope="module")
def keys():
    return C.fixture_keys()


@pytest.fixture(scope="module")
def verifiers(keys):
    vs = [NativeGroth16Verifier(None, vk) for vk, _ in keys]
    yield vs
    for v in vs:
        v.close()


def _check(ver, vk, cases, compressed=False):
    """host statuses of `cases` == their classification, one by one; returns the statuses"""
    want = C.classify_many(vk, cases)
    got = ver.verify_batch_host([p for p, _ in cases], [x for _, x in cases])
    assert got == want, [(i, G16_STATUS_NAMES[g], G16_STATUS_NAMES[w]) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    return got


def test_reference_kat():
    vk, proof, inputs, bad_inputs, bad_proof = C.kat()
    assert len(inputs) == 4
    ver = NativeGroth16Verifier(None, vk)
    got = _check(ver, vk, [(proof, inputs), (proof, bad_inputs), (bad_proof, inputs)])
    assert got[0] == C.OK and got[1] != C.OK and got[2] != C.OK
    assert ver.verify(proof, inputs) is True
    assert ver.verify(F.proof_to_raw_bytes(proof), inputs) is True
    with pytest.raises(ProofRejected) as e:
        ver.verify(proof, bad_inputs)
    assert e.value.status == got[1]
    ver.close()


def test_both_fixture_keys_base_and_rerandomised_proofs(keys, verifiers):
    rng = random.Random(20241)
    for (vk, proofs), ver in zip(keys, verifiers):
        cases = list(proofs)
        for i in range(21):
            proof, pubs = proofs[i % 3]
            cases.append((C.rerandomise(proof, rng.randrange(2, C.R)), pubs))
        assert len(cases) >= 23
        assert _check(ver, vk, cases) == [C.OK] * len(cases)
        # compressed form of every valid proof: the same status; formats.decompress_proof is the yardstick of the encoding
        comp = [F.compress_proof(p) for p, _ in cases]
        assert all(F.decompress_proof(c) == list(p) for c, (p, _) in zip(comp, cases))
        assert ver.verify_batch_host(comp, [x for _, x in cases], compressed=True) == [C.OK] * len(cases)
        # the public inputs of two proofs swapped; [t] A without [1 / t] B
        swapped = [(proofs[0][0], proofs[1][1]), (proofs[1][0], proofs[0][1])]
        a, b, c = C.points(proofs[2][0])
        half = C.G.proof_to_uint256x8((B.mul(5, a), b, c))
        bad = swapped + [(half, proofs[2][1])]
        assert _check(ver, vk, bad) == [C.PAIRING] * 3
        assert ver.verify_batch_host([F.compress_proof(p) for p, _ in bad], [x for _, x in bad], compressed=True) == [C.PAIRING] * 3


def test_one_proof_per_failure_class_and_their_order(keys, verifiers):
    outside = C.twist_point_outside_g2()
    for (vk, proofs), ver in zip(keys, verifiers):
        proof, pubs = proofs[0]
        cases, want = [], []

        def add(p, w):
            cases.append((p, pubs))
            want.append(w)
        for i in range(8):                                   # a coordinate equal to p
            p = list(proof)
            p[i] = C.P
            add(p, C.BAD_ENCODING)
        for lo, hi in ((0, 2), (2, 6), (6, 8)):              # A, B, C zeroed
            p = list(proof)
            p[lo:hi] = [0] * (hi - lo)
            add(p, C.INFINITY)
        for i in (1, 7, 5, 4):                               # A, C, B off their curves
            p = list(proof)
            p[i] = (p[i] + 1) % C.P
            add(p, C.NOT_ON_CURVE)
        add(C.set_b(proof, outside), C.NOT_IN_SUBGROUP)
        two = list(proof)
        two[0], two[1] = B.mul(2, B.G1)
        add(two, C.PAIRING)
        # two defects: the earlier class wins
        p = C.set_b(proof, outside)
        p[1] = (p[1] + 1) % C.P
        add(p, C.NOT_ON_CURVE)                               # A off the curve + B outside G2
        p = list(proof)
        p[6] = p[7] = 0
        p[1] = (p[1] + 1) % C.P
        add(p, C.INFINITY)                                   # C zero + A off the curve
        p = list(proof)
        p[0] = p[1] = 0
        p[4] = C.P + 5
        add(p, C.BAD_ENCODING)                               # A zero + a B coordinate >= p
        p = C.set_b(two, outside)
        add(p, C.NOT_IN_SUBGROUP)                            # wrong A (pairing) + B outside G2
        assert _check(ver, vk, cases) == want


def test_seeded_sweep_of_mutated_proofs(keys, verifiers):
    items = C.sweep(keys, 72, seed=0x6716)
    seen = set()
    for k, ((vk, _), ver) in enumerate(zip(keys, verifiers)):
        cases = [(p, x) for kk, p, x in items if kk == k]
        assert len(cases) >= 32
        seen |= set(_check(ver, vk, cases))
    assert seen == {C.OK, C.BAD_ENCODING, C.INFINITY, C.NOT_ON_CURVE, C.NOT_IN_SUBGROUP, C.PAIRING}


def test_public_input_edges(keys, verifiers):
    for (vk, proofs), ver in zip(keys, verifiers):
        n = len(vk["K"]) - 1
        proof, pubs = proofs[0]
        plus_r = [x + C.R for x in pubs]
        assert all(x < 1 << 256 for x in plus_r)
        cases = [(proof, [0] * n), (proof, [C.R - 1] * n), (proof, pubs), (proof, plus_r), (proofs[1][0], proofs[1][1])]
        got = _check(ver, vk, cases)
        assert got[2] == got[3] == C.OK and got[4] == C.OK and got[0] == got[1] == C.PAIRING
        if n == 40:
            assert all(x % C.R for x in proofs[1][1])        # every input nonzero
    # all-zero inputs: kSum = K[0].  A key whose other K points are wrong still accepts exactly when K[0] alone is right
    vk, proofs = keys[0]
    l = vk["K"][0]
    for x, pt in zip(proofs[0][1], vk["K"][1:]):
        l = B.add(l, B.mul(x, pt))
    vk0 = dict(vk)
    vk0["K"] = [l] + [B.mul(7 + i, B.G1) for i in range(len(vk["K"]) - 1)]
    ver = NativeGroth16Verifier(None, vk0)
    assert _check(ver, vk0, [(proofs[0][0], [0] * (len(vk["K"]) - 1)), (proofs[0][0], [1] + [0] * (len(vk["K"]) - 2))]) == [C.OK, C.PAIRING]
    ver.close()


def _x_without_y():
    x = 1
    while F._is_square((x * x * x + 3) % C.P):
        x += 1
    return x


def test_compressed_form_defects(keys, verifiers):
    (vk, proofs), ver = keys[0], verifiers[0]
    proof, pubs = proofs[0]
    good = F.compress_proof(proof)
    run = lambda c4: ver.verify_batch_host([c4], [pubs], compressed=True)[0]
    assert run(good) == C.OK and run(b"".join(x.to_bytes(32, "big") for x in good)) == C.OK

    def rejected(c4):
        with pytest.raises(F.ProofInvalid):
            F.decompress_proof(c4)
    # an x without a square root: A, C, and a B whose x^3 + b' has a non-square norm
    for i in (0, 3):
        c = list(good)
        c[i] = _x_without_y() << 1
        rejected(c)
        assert run(c) == C.NOT_ON_CURVE
    c = list(good)
    x1 = c[1]
    while True:
        r0, r1 = F._g2_rhs(c[2] >> 2, x1)
        if not F._is_square((r0 * r0 + r1 * r1) % C.P):
            break
        x1 += 1
    c[1] = x1
    rejected(c)
    assert run(c) == C.NOT_ON_CURVE
    # x >= p; a hint bit that selects a root which does not exist: malformed words
    for i, val in ((0, C.P << 1), (3, (C.P << 1) | 1), (2, C.P << 2), (1, C.P), (2, good[2] ^ 2)):
        c = list(good)
        c[i] = val
        rejected(c)
        assert run(c) == C.BAD_ENCODING, i
    # zero words are the point at infinity
    for idx in ((0,), (3,), (1, 2)):
        c = list(good)
        for i in idx:
            c[i] = 0
        assert F.decompress_proof(c).count(0) >= 2 and run(c) == C.INFINITY
    # the sign bit flipped: a valid point, the other one -- the pairing fails; equals the status of its decompression
    c = list(good)
    c[0] ^= 1
    assert run(c) == C.classify(vk, F.decompress_proof(c), pubs) == C.PAIRING
    # order across points: an unreduced C before an A without y
    c = list(good)
    c[0] = _x_without_y() << 1
    c[3] = C.P << 1
    assert run(c) == C.BAD_ENCODING
    # B on the twist but outside G2, compressed
    c = F.compress_proof(C.set_b(proof, C.twist_point_outside_g2()))
    assert run(c) == C.NOT_IN_SUBGROUP


def test_invalid_keys_are_refused_and_empty_batches_are_a_no_op(keys, verifiers):
    from zklc_amd import ZklcError
    vk, proofs = keys[0]
    bad = dict(vk)
    bad["gamma2"] = C.twist_point_outside_g2()
    with pytest.raises(ZklcError) as e:
        NativeGroth16Verifier(None, bad)
    assert e.value.code == -1
    bad = dict(vk)
    bad["K"] = list(vk["K"])
    bad["K"][2] = (vk["K"][2][0], (vk["K"][2][1] + 1) % C.P)
    with pytest.raises(ZklcError) as e:
        NativeGroth16Verifier(None, bad)
    assert e.value.code == -1
    bad = dict(vk)
    bad["alpha1"] = None                  # the point at infinity: a degenerate key
    with pytest.raises(ZklcError):
        NativeGroth16Verifier(None, bad)
    assert verifiers[0].verify_batch_host([], []) == []
    with pytest.raises(ValueError):       # no context: the GPU path is not available, and nothing falls back
        verifiers[0].verify_batch([proofs[0][0]], [proofs[0][1]])


def test_sizes_are_checked_before_the_call(keys, verifiers):
    (vk, proofs), ver = keys[0], verifiers[0]
    proof, pubs = proofs[0]
    raw = F.proof_to_raw_bytes(proof)
    for bad in (raw[:-1], raw + b"\0", raw[:128], proof[:7], proof + [1]):
        with pytest.raises(ValueError):
            ver.verify_batch_host([bad], [pubs])
    with pytest.raises(ValueError):
        ver.verify_batch_host([raw], [pubs], compressed=True)
    with pytest.raises(ValueError):
        ver.verify_batch_host([F.compress_proof(proof)], [pubs])
    with pytest.raises(ValueError):
        ver.verify_batch_host([proof], [pubs[:-1]])
    with pytest.raises(ValueError):
        ver.verify_batch_host([proof, proof], [pubs])
    with pytest.raises(ValueError):
        ver.verify_batch_host([[1 << 256] + proof[1:]], [pubs])
    assert ver.verify_batch_host([raw], [pubs]) == [C.OK]
    assert ver.verify_batch_host([raw, raw], [pubs, pubs], nthreads=1) == [C.OK, C.OK]


def test_subgroup_test_agrees_with_the_oracle_on_twist_points(keys, verifiers):
    """the endomorphism criterion of csrc/groth16_verify.cuh against [r] Q == O of the oracle, on twist points outside G2 (found by
    solving the twist equation), on their multiples by the cofactor 2p - r (inside G2) and on multiples of the generator"""
    (vk, proofs), ver = keys[0], verifiers[0]
    proof, pubs = proofs[0]
    pts = []
    for x0 in range(1, 200):
        if len(pts) >= 10:
            break
        r0, r1 = F._g2_rhs(x0, 3)
        try:
            pts.append(((x0, 3), F._sqrt_fp2(r0, r1, x0 % 2 == 1)))
        except F.ProofInvalid:
            continue
    assert len(pts) == 10
    cof = 2 * C.P - C.R
    inside = []
    # g2_mul reduces its scalar modulo r, so the cofactor multiple is built from two multiplications: cof = q r + s
    q, s = divmod(cof, C.R)
    for pt in pts[:3]:
        rp = B.g2_add(B.g2_mul(C.R - 1, pt), pt)                       # [r] pt, not O
        assert rp is not None
        inside.append(B.g2_add(B.g2_mul(q, rp), B.g2_mul(s, pt)))
    inside += [B.g2_mul(k, B.G2) for k in (1, 2, C.R - 1, 0x1234567890abcdef)]
    cases = [(C.set_b(proof, pt), pubs) for pt in pts + inside]
    got = _check(ver, vk, cases)
    assert got == [C.NOT_IN_SUBGROUP] * len(pts) + [C.PAIRING] * len(inside)
