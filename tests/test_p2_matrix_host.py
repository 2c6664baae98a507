"""The parameter matrix of tests/p2_matrix_cases.py on the host (no GPU): the oracle's C prover's proof of every case is accepted by
the verifier restatement and by the native verifier's host path (zklc_plonky2_verify_batch_host), and every tampered copy gets the
status the restatement's failure names.  The GPU tests (tests/test_gpu_p2_matrix.py) compare the GPU prover and the GPU verifier
with the same proofs and statuses."""
import json

import pytest

import zklc_amd  # noqa: F401
from zklc_amd.plonky2 import serialization as S, HASH_GL
from zklc_amd.plonky2.verifier import Verifier, PROOF_OK
from oracle import plonky2_verifier as V, poseidon_gl as pgl
from test_plonky2_verifier_host import expected_status
import p2_matrix_cases as M


@pytest.fixture(scope="module", autouse=True)
def _fast_poseidon():
    pgl.use_c_port()        # the restatement's permutation through the oracle's C port: same values, the matrix in seconds


def host_statuses(case):
    data = M.make(case)[0]
    with Verifier(None, data.common_data(), M.reference(case)[1]) as v:
        return v.verify_batch_host(M.batch(case))


@pytest.mark.parametrize("case", M.CASES + [M.THREE_CHALLENGES], ids=lambda c: c.name)
def test_c_prover_proof_and_tampered_copies(case):
    data = M.make(case)[0]
    raw, vd = M.reference(case)
    common = data.common_data()
    assert len(raw) == S.proof_size(common, HASH_GL)
    if case.degree_bits <= 12:
        V.verify(json.loads(json.dumps(S.proof_from_bytes(raw, common, HASH_GL))), vd, common)
    batch, kinds = M.batch(case), M.kinds(case)
    want = [PROOF_OK] + [expected_status(S.proof_from_bytes(t, common, HASH_GL), vd, common, k) for t, k in zip(batch[1:], kinds)]
    got = host_statuses(case)
    print(case.name, data.fri_arity_bits, kinds, got)
    assert got == want, (kinds, got, want)
    assert got[0] == PROOF_OK and all(s != PROOF_OK for s in got[1:]), got


def test_the_matrix_reaches_the_branches_it_names():
    """the size axis crosses the Merkle plan's thresholds (2^12 .. 2^14 parents: degree_bits 9 .. 11 at rate 3), the parameter axis
    has every arity from 2^1 to 2^5, circuits without a reduction, caps of height 0 and of the tree's own height, and a number of
    routed wires that is no multiple of the chunk size"""
    from zklc_amd.plonky2.builder import fri_reduction_arity_bits
    arities, caps, no_reduction, whole_tree_caps, partial = set(), set(), 0, 0, 0
    for case in M.CASES:
        cfg = M.config(case)
        fri = cfg["fri_config"]
        ab = fri_reduction_arity_bits(cfg, case.degree_bits)
        arities |= set(ab)
        no_reduction += not ab
        caps.add(fri["cap_height"])
        whole_tree_caps += fri["cap_height"] == case.degree_bits + fri["rate_bits"]
        partial += cfg["num_routed_wires"] % cfg["max_quotient_degree_factor"] != 0
    assert arities == {1, 2, 3, 4, 5} and no_reduction >= 6 and whole_tree_caps >= 1 and partial >= 4
    assert caps == {0, 1, 2, 4, 7, 9}
    assert {c.degree_bits for c in M.CASES} == {2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 14}


def test_synthetic_circuit_too_small_is_an_assertion():
    """2^5 rows cannot hold two rows of each of the recursion mix's gate types and the public-input rows: the generator says so"""
    from zklc_amd.plonky2 import synthetic as SY, gates as G, standard_recursion_config
    cfg = standard_recursion_config()
    mix = SY.recursion_shape_mix(cfg) + [(G.ExponentiationGate(20), 3)]
    with pytest.raises(AssertionError, match="circuit too small"):
        SY.synthetic_circuit(5, cfg, mix, num_public_inputs=11, seed=3)


def test_cap_taller_than_the_tree_serialises_clamped():
    """cap_height 12 over a 2^9 LDE: both provers and the native verifier commit to the 2^9 leaves' digests themselves; the
    serialisation follows (caps of 2^9 entries, openings without siblings), so bytes -> proof.json -> bytes is the identity, the
    size is proof_size's and the native verifier accepts the proof and rejects its tampered copies"""
    case = M._case("cap-12", "recursion", 6, cap=12)
    data = M.make(case)[0]
    raw, vd = M.reference(case)
    common = data.common_data()
    assert data.fri_arity_bits == [] and len(vd["constants_sigmas_cap"]) == 1 << 9
    assert len(raw) == S.proof_size(common, HASH_GL)
    pj = S.proof_from_bytes(raw, common, HASH_GL)
    assert len(pj["proof"]["wires_cap"]) == 1 << 9
    assert pj["proof"]["opening_proof"]["query_round_proofs"][0]["initial_trees_proof"]["evals_proofs"][0][1]["siblings"] == []
    assert S.proof_to_bytes(pj, common, HASH_GL) == raw
    assert M.kinds(case)[1] == "wires_cap"
    got = host_statuses(case)
    assert got[0] == PROOF_OK and all(s != PROOF_OK for s in got[1:]), got
