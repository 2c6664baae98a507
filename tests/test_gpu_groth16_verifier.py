"""zklc_groth16_verify_batch on the GPU (csrc/groth16_verify.hip: the validation / kSum kernel + the pairing kernels) against the
host path and against the independent classification of tests/groth16_cases.py, on the matrices of
tests/test_groth16_verifier_host.py; batch sizes that mix valid and invalid proofs inside a wave and reach the throughput form of
the pairing kernel (> 2048); no state between calls; agreement with zklc_amd.groth16.Groth16Verifier.  Expected statuses of the
large batches come from repeating classified proofs."""
import random

import pytest

import groth16_cases as C
from oracle import bn254 as B
from zklc_amd import formats as F
from zklc_amd.groth16 import Groth16Verifier, NativeGroth16Verifier, G16_STATUS_NAMES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def keys():
    return C.fixture_keys()


@pytest.fixture(scope="module")
def verifiers(zctx, keys):
    vs = [NativeGroth16Verifier(zctx, vk) for vk, _ in keys]
    yield vs
    for v in vs:
        v.close()


def _failure_cases(proof, pubs):
    """one proof per failure class (tests/test_groth16_verifier_host.py has the full list)"""
    out = []
    rng = random.Random(5)
    for kind in ("p", "zero", "curve", "subgroup", "two_g1"):
        out.append((C.mutate(proof, kind, rng), pubs))
    p = C.set_b(proof, C.twist_point_outside_g2())
    p[1] = (p[1] + 1) % C.P
    out.append((p, pubs))                      # two defects
    return out


@pytest.fixture(scope="module")
def matrix(keys):
    """per key: [(proof8, public_inputs)] -- base, re-randomised, swapped inputs, the failure classes and a seeded sweep -- and
    the classification of each"""
    rng = random.Random(20242)
    items = C.sweep(keys, 72, seed=0x6716)
    out = []
    for k, (vk, proofs) in enumerate(keys):
        cases = list(proofs)
        for i in range(20):
            proof, pubs = proofs[i % 3]
            cases.append((C.rerandomise(proof, rng.randrange(2, C.R)), pubs))
        cases += [(proofs[0][0], proofs[1][1]), (proofs[1][0], proofs[0][1])]
        cases += _failure_cases(*proofs[0])
        cases += [(p, x) for kk, p, x in items if kk == k]
        n = len(vk["K"]) - 1
        cases += [(proofs[0][0], [0] * n), (proofs[0][0], [C.R - 1] * n), (proofs[0][0], [x + C.R for x in proofs[0][1]])]
        out.append((cases, C.classify_many(vk, cases)))
    return out


def _names(xs):
    return [G16_STATUS_NAMES[x] for x in xs]


def test_gpu_equals_host_equals_classification(verifiers, matrix):
    seen = set()
    for ver, (cases, want) in zip(verifiers, matrix):
        ps, xs = [p for p, _ in cases], [x for _, x in cases]
        gpu, host = ver.verify_batch(ps, xs), ver.verify_batch_host(ps, xs)
        assert _names(gpu) == _names(host) == _names(want)
        t = ver.last_timings()
        print("groth16 verify_batch n = %d, n_public = %d: ms %s" % (len(cases), ver.n_public, t))
        assert t["total"] > 0 and t["pairing_kernel"] > 0 and t["validate_ksum_kernel"] > 0
        seen |= set(gpu)
    assert seen == set(range(6))


def test_reference_kat_and_agreement_with_the_python_verifier(zctx, keys):
    vk, proof, inputs, bad_inputs, bad_proof = C.kat()
    cases = [(proof, inputs), (proof, bad_inputs), (bad_proof, inputs)] + _failure_cases(proof, inputs)
    want = C.classify_many(vk, cases)
    ver, old = NativeGroth16Verifier(zctx, vk), Groth16Verifier(zctx, vk)
    got = ver.verify_batch([p for p, _ in cases], [x for _, x in cases])
    assert _names(got) == _names(want) and got[0] == C.OK
    assert set(got) == set(range(6))
    for (p, x), st in zip(cases, got):
        try:
            verdict = old.verify(p, x)
        except F.ProofInvalid:
            verdict = None
        assert verdict == {C.OK: True, C.PAIRING: False}.get(st), (G16_STATUS_NAMES[st], verdict)
    ver.close()


@pytest.mark.parametrize("n", [1, 5, 65, 300, 2100])
def test_batch_sizes_with_valid_and_invalid_proofs_in_one_wave(verifiers, matrix, n):
    """2100 > 2048: the throughput form of the pairing kernel"""
    k = 1 if n == 65 else 0                     # n_public = 40 for one size
    ver, (cases, want) = verifiers[k], matrix[k]
    rng = random.Random(n)
    idx = [rng.randrange(len(cases)) for _ in range(n)]
    if n >= 5:
        assert len({want[i] for i in idx}) >= 3
    ps, xs, exp = [cases[i][0] for i in idx], [cases[i][1] for i in idx], [want[i] for i in idx]
    assert ver.verify_batch(ps, xs) == exp
    assert ver.verify_batch_host(ps, xs) == exp


def test_no_state_between_calls(verifiers, matrix):
    ver, (cases, want) = verifiers[0], matrix[0]
    big = [cases[i % len(cases)] for i in range(200)]
    small = cases[3:8]
    run = lambda cs: ver.verify_batch([p for p, _ in cs], [x for _, x in cs])
    first = run(small)
    assert first == want[3:8]
    assert run(big) == [want[i % len(cases)] for i in range(200)]
    assert run(small) == first == run(small)
    assert run(list(reversed(small))) == list(reversed(first))


def test_compressed_form_on_the_gpu(verifiers, matrix):
    for ver, (cases, want) in zip(verifiers, matrix):
        sel = [(c, w) for c, w in zip(cases, want) if w in (C.OK, C.PAIRING, C.NOT_IN_SUBGROUP)]
        comp = [F.compress_proof(p) for (p, _), _ in sel]
        xs = [x for (_, x), _ in sel]
        good = comp[0]
        # defects of the words themselves (expected classes: tests/test_groth16_verifier_host.py::test_compressed_form_defects)
        x = 1
        while F._is_square((x * x * x + 3) % C.P):
            x += 1
        extra = []
        for i, val, st in ((0, x << 1, C.NOT_ON_CURVE), (3, C.P << 1, C.BAD_ENCODING), (2, good[2] ^ 2, C.BAD_ENCODING), (0, 0, C.INFINITY),
                           (1, C.P, C.BAD_ENCODING)):
            c = list(good)
            c[i] = val
            extra.append((c, st))
        allc = comp + [c for c, _ in extra]
        allx = xs + [xs[0]] * len(extra)
        exp = [w for _, w in sel] + [st for _, st in extra]
        assert _names(ver.verify_batch(allc, allx, compressed=True)) == _names(ver.verify_batch_host(allc, allx, compressed=True)) == _names(exp)
