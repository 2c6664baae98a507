"""The reference's golden plonky2 proofs verify through this repo's oracle stack (transcript, PoW, Poseidon-BN254
Merkle paths to the caps, evaluation-domain order, FRI folding): pins oracle/poseidon_gl.py,
oracle/poseidon_bn254.py and the Merkle conventions the GPU kernels are tested against."""
import copy
import gzip
import json
import os

import pytest

from conftest import GOLDEN, load_golden
from oracle import plonky2_verifier as V

FIX = ["plonky2_near_random_CGZP.json", "plonky2_gnark_test_circuit.json"]


@pytest.mark.parametrize("name", FIX)
def test_golden_proof_verifies(name):
    j = load_golden(name)
    ch = V.verify(j["proof"], j["verifier_data"], j["common_data"])
    assert len(ch["query_indices"]) == 28 and len(ch["fri_betas"]) == 2
    assert ch["pow_response"] < 1 << 48


@pytest.mark.parametrize("what", ["pow", "sibling", "leaf", "step_eval", "final_poly", "cap", "opening"])
def test_tampering_is_detected(what):
    j = copy.deepcopy(load_golden(FIX[0]))
    op = j["proof"]["proof"]["opening_proof"]
    q0 = op["query_round_proofs"][0]
    if what == "pow":
        op["pow_witness"] += 1
    elif what == "sibling":
        s = q0["initial_trees_proof"]["evals_proofs"][1][1]["siblings"]
        s[3] = str(int(s[3]) ^ 1)
    elif what == "leaf":
        q0["initial_trees_proof"]["evals_proofs"][1][0][7] ^= 1
    elif what == "step_eval":
        q0["steps"][1]["evals"][5][0] ^= 1
    elif what == "final_poly":
        op["final_poly"]["coeffs"][2][0] ^= 1
    elif what == "cap":
        c = j["proof"]["proof"]["wires_cap"]
        c[0] = str(int(c[0]) ^ 1)
    elif what == "opening":
        j["proof"]["proof"]["openings"]["wires"][3][0] ^= 1
    with pytest.raises(AssertionError):
        V.verify(j["proof"], j["verifier_data"], j["common_data"])


def test_all_reference_proofs_full_28_rounds():
    """the reference's four golden proofs, all 28 FRI query rounds (tests/golden/make_plonky2_fixtures.py: full_proofs)"""
    with gzip.open(os.path.join(GOLDEN, "plonky2_reference_proofs_full.json.gz")) as f:
        cases = json.load(f)
    assert len(cases) == 4
    for c in cases:
        assert len(c["proof"]["proof"]["opening_proof"]["query_round_proofs"]) == 28, c["source"]
        V.verify(c["proof"], c["verifier_data"], c["common_data"])
