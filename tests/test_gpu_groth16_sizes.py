"""`Groth16Prover` at the domain sizes where its production kernels run -- 2^12 (the first two-pass NTT size, split 6 + 6, 4000
constraints: live padding), 2^13 (odd split 7 + 6, no padding) and 2^15 (split 8 + 7; G1 sums at c = 14) -- on two constraint
systems (uniform wires; mostly bits with points at infinity in the key), against the CLOSED FORM of the proof in the exponent
(oracle.groth16.closed_form_proof: the toxic waste is known in a test, so Ar, Bs, Krs are three scalar multiplications of field
sums -- no transform, no multi-exponentiation, no key point).  The key's points come from the library's batched fixed-base
multiplication over the key's scalars; a fixed sample of them is compared with the oracle's B.mul / B.g2_mul so that a failure
points at the right kernel.  Every comparison is exact equality of integers.  The paths are ASSERTED from the plan functions
(tests/hostsim): every G1 sum splits by the endomorphism (glv = 1) with c = 11 / 11 / 14, the transforms take the two-pass path."""
import numpy as np
import pytest
import torch

import groth16_size_cases as S
from oracle import bn254 as B, groth16 as G
from zklc_amd import fixed_base as FB
from zklc_amd.groth16 import Groth16Prover, Groth16Verifier, UnsatisfiedConstraint
from zklc_amd.r1cs import R1CS

pytestmark = pytest.mark.gpu

R = G.R
RS = [(0, 0), (R - 1, R - 1), (0x2b1f0c3d5e6f708192a3b4c5d6e7f8091a2b3c4d5e6f70819a, 0x1d9e8f7a6b5c4d3e2f1a0b9c8d7e6f5a4b3c2d1e0f9a8b7c6d)]
SPLIT = {12: (6, 6), 13: (7, 6), 15: (8, 7)}
G1_WINDOW = {12: 11, 13: 11, 15: 14}
CASES = [(log_n, kind) for log_n in (12, 13, 15) for kind in ("chain", "bits")]


@pytest.fixture(scope="module")
def generators(zctx):
    """the c = 16 tables of the two generators, built once by the GPU"""
    t = {1: FB.FixedBase(zctx, FB.G1), 2: FB.FixedBase(zctx, FB.G2)}
    yield t
    for x in t.values():
        x.close()


def _points(zctx, table, scalars):
    """scalars * generator on the GPU -> (uint64 [n, 8 | 16] on the host, (infinities, first | None))"""
    dev = torch.device("cuda", zctx.device_id)
    d_s = torch.from_numpy(S.words_from_ints(scalars).view(np.int64)).to(dev)
    words, summary, ws = table.mul_dev(d_s)
    zctx.synchronize()
    return words.cpu().numpy().view(np.uint64).copy(), FB.summary_tuple(summary.cpu().numpy().view(np.uint64))


@pytest.fixture(scope="module", params=CASES, ids=["2p%d-%s" % c for c in CASES])
def case(request, zctx, generators):
    """one (domain, system): the key scalars and the closed-form proofs in Python, the key points on the GPU, the prover with the
    constraint system resident -- built once, shared by the tests below, closed afterwards"""
    log_n, kind = request.param
    sy = dict(S.system(kind, log_n))
    sc = G.key_scalars(sy["r1cs"], sy["n_public"], S.TOXIC)
    assert sc["n"] == 1 << log_n and sc["n_wires"] == len(sy["witness"])
    tau, alpha, beta, gamma, delta = S.TOXIC
    arrays = {"A": (1, sc["a_t"]), "B1": (1, sc["b_t"]), "B2": (2, sc["b_t"]), "K": (1, sc["k_pk"]), "Z": (1, sc["z"])}
    pk = {"n": sc["n"], "n_public": sy["n_public"], "alpha1": B.mul(alpha, B.G1), "beta1": B.mul(beta, B.G1), "delta1": B.mul(delta, B.G1),
          "beta2": B.g2_mul(beta, B.G2), "delta2": B.g2_mul(delta, B.G2)}
    summaries = {}
    for name, (group, scalars) in arrays.items():
        pk[name + "_words"], summaries[name] = _points(zctx, generators[group], scalars)
    sys_ = R1CS.from_rows(*sy["r1cs"], sc["n_wires"], ctx=zctx)
    prover = Groth16Prover(zctx, pk, sys_)
    sy.update(scalars=sc, arrays=arrays, pk=pk, summaries=summaries, prover=prover,
              want=[G.closed_form_proof(sc, S.TOXIC, sy["n_public"], sy["witness"], r, s) for r, s in RS])
    yield sy
    prover.close()
    sys_.close()


def _assert_paths(hostsim, case, pk=None):
    """the plans the library makes for this key's operands: the production ones, not the small case's"""
    log_n = case["log_n"]
    pk = pk or case["pk"]
    assert S.fr_ntt_plan(hostsim, log_n) == SPLIT[log_n] + (True,)
    sizes = {"A": len(pk["A_words"]) + 2, "B1": len(pk["B1_words"]) + 2, "K": len(pk["K_words"]), "Z": len(pk["Z_words"])}
    for name, n in sizes.items():
        plan = S.msm_plan(hostsim, n, True)
        assert plan["glv"] == 1 and plan["c"] == G1_WINDOW[log_n], (name, n, plan)
    assert S.msm_plan(hostsim, len(pk["B2_words"]) + 2, False)["glv"] == 0
    return sizes


def test_the_key_points_are_the_oracles(case):
    """the fixed-base kernel that made the key: per array at least 32 points, the first, the last and every zero scalar (all-zero
    record) against B.mul / B.g2_mul of their scalars; the count of points at infinity against the count of zero scalars"""
    jobs, where = [], []
    for name, (group, scalars) in case["arrays"].items():
        zeros = [i for i, s in enumerate(scalars) if s == 0]
        assert case["summaries"][name] == (len(zeros), zeros[0] if zeros else None), name
        idx = S.sample_indices(scalars, 32, seed=case["log_n"])
        assert {0, len(scalars) - 1} | set(zeros) <= set(idx) and len(set(idx) - set(zeros)) >= 32
        jobs += [(group, scalars[i]) for i in idx]
        where += [(name, i) for i in idx]
    for (name, i), want in zip(where, S.expected_point_words(jobs)):
        assert [int(x) for x in case["pk"][name + "_words"][i]] == want, "%s[%d]" % (name, i)
    if case["kind"] == "bits":
        u = case["layout"]["u"]
        assert len(u) >= 50 and all(case["scalars"]["a_t"][i] == 0 and case["scalars"]["b_t"][i] == 0 for i in u)


def test_prove_equals_the_closed_form(zctx, hostsim, case):
    """two-pass computeH (split t1 + t2 of SPLIT) feeding the Z sum on its own stream, A / B1 / K / Z sums with the endomorphism
    split at c = 11 (2^12, 2^13) or 14 (2^15), B2 without it, the five-point sum at the end: the eight words are the closed form's
    for (r, s) = (0, 0), (r - 1, r - 1) and a random pair"""
    _assert_paths(hostsim, case)
    prover = case["prover"]
    for (r, s), want in zip(RS, case["want"]):
        got = prover.prove(case["witness"], case["abc"], r, s)
        assert got == want, "GPU proof differs from the closed form at (r, s) = (%#x, %#x)" % (r, s)
    print("groth16 prove (n = 2^%d, %s): ms" % (case["log_n"], case["kind"]), prover.last_ms)


def test_prove_witness_equals_the_closed_form(zctx, hostsim, case):
    """the same paths with a, b, c evaluated on the GPU from the resident constraint system (rows in all lanes-per-row bins for
    the 'bits' system), with and without the satisfaction check"""
    _assert_paths(hostsim, case)
    prover = case["prover"]
    r, s = RS[2]
    assert prover.prove_witness(case["witness"], r, s) == case["want"][2]
    assert prover.last_ms["r1cs_check"] is True
    assert prover.prove_witness(case["witness"], r, s, check=False) == case["want"][2]
    assert prover.prove_witness(case["witness"], *RS[1]) == case["want"][1]


def test_a_broken_witness_raises_and_the_next_proof_is_the_closed_form(zctx, hostsim, case):
    """a bit wire set to 2 (chain system: a chain value bumped) raises UnsatisfiedConstraint with the index and count Python finds;
    the three streams are drained, and the next proof of the good witness is the closed form again (two-pass path, glv = 1)"""
    _assert_paths(hostsim, case)
    prover = case["prover"]
    bad = list(case["witness"])
    if case["kind"] == "bits":
        bits = case["layout"]["bits"]
        wire = bits[len(bits) // 2]
        assert bad[wire] in (0, 1)
        bad[wire] = 2
    else:
        wire = len(bad) // 2
        bad[wire] = (bad[wire] + 1) % R
    first, count = S.unsatisfied(case["r1cs"], bad, case["n"])
    assert count == 2
    with pytest.raises(UnsatisfiedConstraint) as e:
        prover.prove_witness(bad, *RS[2])
    assert (e.value.index, e.value.count) == (first, count)
    assert prover.prove_witness(case["witness"], *RS[2]) == case["want"][2]


def test_the_compacted_key_with_masks_gives_the_same_words(zctx, hostsim, case):
    """gnark's key layout (points at infinity removed from A / B1 / B2, positions in infinity_a / infinity_b): the scalar vectors
    are gathered on the device before sums that still split (glv = 1, c as in G1_WINDOW)"""
    sc, pk = case["scalars"], case["pk"]
    inf_a = np.array([x == 0 for x in sc["a_t"]])
    inf_b = np.array([x == 0 for x in sc["b_t"]])
    # the chain system: the public wires and the last chain value; the 'bits' system: every u besides
    assert inf_a.sum() >= 4 and inf_b.sum() >= 4 and (case["kind"] != "bits" or min(inf_a.sum(), inf_b.sum()) >= 50)
    assert not pk["A_words"][inf_a].any() and not pk["B1_words"][inf_b].any() and not pk["B2_words"][inf_b].any()
    compact = dict(pk)
    compact["A_words"], compact["B1_words"], compact["B2_words"] = pk["A_words"][~inf_a], pk["B1_words"][~inf_b], pk["B2_words"][~inf_b]
    compact["infinity_a"], compact["infinity_b"] = inf_a, inf_b
    _assert_paths(hostsim, case, compact)
    prover = Groth16Prover(zctx, compact)
    try:
        for (r, s), want in zip(RS, case["want"]):
            assert prover.prove(case["witness"], case["abc"], r, s) == want
    finally:
        prover.close()


def test_the_verifier_accepts_the_proof_under_the_closed_form_key(zctx, hostsim, case):
    """Groth16Verifier under oracle.groth16.closed_form_vk: a proof no oracle `prove` made (two-pass computeH, split sums) passes the
    pairing equation with its public inputs and fails with one of them changed"""
    _assert_paths(hostsim, case)
    vk = G.closed_form_vk(case["scalars"], S.TOXIC, case["n_public"])
    proof = case["prover"].prove(case["witness"], case["abc"], *RS[2])
    assert proof == case["want"][2]
    ver = Groth16Verifier(zctx, vk)
    pubs = case["publics"]
    assert ver.verify(proof, pubs) is True
    assert ver.verify(proof, [pubs[0], (pubs[1] + 1) % R, pubs[2]]) is False


@pytest.mark.parametrize("kind", ["chain", "bits"])
def test_fixed_base_tables_give_the_closed_form_at_2p12(zctx, hostsim, generators, kind, monkeypatch):
    """ZKLC_GROTH16_FIXED=1 at 2^12: the four big sums over fixed-base tables (no endomorphism split on that form), computeH on
    the two-pass path (6 + 6): the same words"""
    sy = S.system(kind, 12)
    assert S.fr_ntt_plan(hostsim, 12) == (6, 6, True)
    sc = G.key_scalars(sy["r1cs"], sy["n_public"], S.TOXIC)
    tau, alpha, beta, gamma, delta = S.TOXIC
    pk = {"n": sc["n"], "n_public": sy["n_public"], "alpha1": B.mul(alpha, B.G1), "beta1": B.mul(beta, B.G1), "delta1": B.mul(delta, B.G1),
          "beta2": B.g2_mul(beta, B.G2), "delta2": B.g2_mul(delta, B.G2)}
    for name, (group, scalars) in {"A": (1, sc["a_t"]), "B1": (1, sc["b_t"]), "B2": (2, sc["b_t"]), "K": (1, sc["k_pk"]), "Z": (1, sc["z"])}.items():
        pk[name + "_words"] = _points(zctx, generators[group], scalars)[0]
    monkeypatch.setenv("ZKLC_GROTH16_FIXED", "1")
    prover = Groth16Prover(zctx, pk)
    try:
        assert prover.fixed
        for r, s in RS:
            assert prover.prove(sy["witness"], sy["abc"], r, s) == G.closed_form_proof(sc, S.TOXIC, sy["n_public"], sy["witness"], r, s)
    finally:
        prover.close()
