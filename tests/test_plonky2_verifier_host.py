"""Native plonky2 verifier, host path (zklc_plonky2_verify_batch_host; no GPU): the reference's golden proofs verify, every kind of
tampering ends at the status the verifier restatement's failure names (oracle/plonky2_verifier.py), proofs of the oracle's
provers over all 22 gate types verify, and a batch reports each proof's own status."""
import copy
import gzip
import json
import os

import numpy as np
import pytest

import zklc_amd  # noqa: F401
from zklc_amd.plonky2 import serialization as S, HASH_GL, HASH_BN128
from zklc_amd.plonky2.verifier import (Verifier, ProofRejected, PROOF_OK, PROOF_BAD_FORMAT, PROOF_BAD_POW, PROOF_BAD_VANISHING,
                                       PROOF_BAD_MERKLE, PROOF_BAD_FRI)
from conftest import GOLDEN
from oracle import plonky2_verifier as V

P = 2**64 - 2**32 + 1
TAMPERS = ["pow_witness", "initial_sibling", "initial_leaf", "step_eval_other", "step_eval_within", "final_poly", "wires_cap",
           "wires_opening", "public_input", "non_canonical"]


def golden():
    with gzip.open(os.path.join(GOLDEN, "plonky2_reference_proofs_full.json.gz")) as f:
        return json.load(f)


def oracle_status(proof, verifier_only, common):
    """the verifier restatement's verdict as a ZKLC_PROOF_* status, from the text of its failure"""
    try:
        V.verify(json.loads(json.dumps(proof)), verifier_only, common)
        return PROOF_OK
    except AssertionError as e:
        msg = str(e)
    for key, st in (("proof of work", PROOF_BAD_POW), ("vanishing", PROOF_BAD_VANISHING), ("initial tree", PROOF_BAD_MERKLE),
                    ("commit-phase tree", PROOF_BAD_MERKLE), ("fri consistency", PROOF_BAD_FRI), ("final polynomial", PROOF_BAD_FRI)):
        if key in msg:
            return st
    raise AssertionError("unmapped oracle failure: %r" % msg)


def _bump_hash(h):
    if isinstance(h, dict):
        return {"elements": [(int(h["elements"][0]) + 1) % P] + [int(x) for x in h["elements"][1:]]}
    return str(int(h) ^ 1)


def tamper(proof, common, verifier_only, what):
    """a copy of the proof.json dict `proof` with one thing changed"""
    j = copy.deepcopy(proof)
    pr = j["proof"]
    op = pr["opening_proof"]
    q0 = op["query_round_proofs"][0]
    fp = common["fri_params"]
    if what.startswith("step_eval"):
        arity = 1 << fp["reduction_arity_bits"][0]     # only circuits with a FRI reduction have step evaluations
        ch = V.challenges(V.parse_proof(json.loads(json.dumps(proof)), verifier_only), common)
        within = (ch["query_indices"][0] % (1 << (fp["degree_bits"] + fp["config"]["rate_bits"]))) & (arity - 1)
        pos = within if what == "step_eval_within" else (within + 1) % arity
        e = q0["steps"][0]["evals"][pos]
        e[0] = (int(e[0]) + 1) % P
    elif what == "pow_witness":
        op["pow_witness"] = (int(op["pow_witness"]) + 1) % P
    elif what == "initial_sibling":
        s = q0["initial_trees_proof"]["evals_proofs"][1][1]["siblings"]
        s[0] = _bump_hash(s[0])
    elif what == "initial_leaf":
        leaf = q0["initial_trees_proof"]["evals_proofs"][1][0]
        leaf[3] = (int(leaf[3]) + 1) % P
    elif what == "final_poly":
        c = op["final_poly"]["coeffs"][0]
        c[0] = (int(c[0]) + 1) % P
    elif what == "wires_cap":
        pr["wires_cap"][0] = _bump_hash(pr["wires_cap"][0])
    elif what == "wires_opening":
        o = pr["openings"]["wires"][3]
        o[0] = (int(o[0]) + 1) % P
    elif what == "public_input":
        j["public_inputs"][0] = (int(j["public_inputs"][0]) + 1) % P
    elif what == "non_canonical":
        leaf = q0["initial_trees_proof"]["evals_proofs"][2][0]
        leaf[0] = int(leaf[0]) + P if int(leaf[0]) + P < 2**64 else P
    else:
        raise ValueError(what)
    return j


def expected_status(tampered, verifier_only, common, what):
    return PROOF_BAD_FORMAT if what == "non_canonical" else oracle_status(tampered, verifier_only, common)


@pytest.fixture(scope="module")
def golden_cases():
    return golden()


def test_golden_proofs_verify(golden_cases):
    """the reference's four golden proofs (Poseidon-BN128 wrap config, 28 rounds, 13 gate types): status 0 from bytes and JSON"""
    assert len(golden_cases) == 4
    for c in golden_cases:
        with Verifier(None, c["common_data"], c["verifier_data"]) as v:
            assert v.hasher == HASH_BN128
            raw = S.proof_to_bytes(c["proof"], c["common_data"], HASH_BN128)
            assert v.proof_bytes == len(raw) == S.proof_size(c["common_data"], HASH_BN128)
            assert v.verify_batch([raw, c["proof"]]) == [PROOF_OK, PROOF_OK], c["source"]
            v.verify(raw)


@pytest.mark.parametrize("what", TAMPERS)
def test_golden_tampering_matrix(golden_cases, what):
    """one change to golden proof 0 -> exactly the status the oracle's failure maps to (an element >= p: FORMAT)"""
    c = golden_cases[0]
    common, vd = c["common_data"], c["verifier_data"]
    t = tamper(c["proof"], common, vd, what)
    want = expected_status(t, vd, common, what)
    assert want != PROOF_OK
    with Verifier(None, common, vd) as v:
        got = v.verify_batch_host([S.proof_to_bytes(t, common, HASH_BN128)])
        assert got == [want], (what, got, want)
        with pytest.raises(ProofRejected) as ei:
            v.verify(t)
        assert ei.value.status == want and isinstance(ei.value, ValueError)


def _synthetic(shape, degree_bits, seed=3, npi=11):
    from zklc_amd.plonky2 import synthetic as SY, gates as G, standard_recursion_config, wide_ecc_config
    if shape == "recursion":
        cfg = standard_recursion_config()
        mix = SY.recursion_shape_mix(cfg) + [(G.ExponentiationGate(20), 3)]
    else:
        cfg = wide_ecc_config()
        mix = SY.ed25519_shape_mix(cfg)
    return SY.synthetic_circuit(degree_bits, cfg, mix, num_public_inputs=npi, seed=seed)


def vanishing_case(prove=None):
    """a synthetic 2^6 circuit whose witness breaks one gate constraint on a wire no copy constraint binds (an S-box input of a
    PoseidonGate row, column 100, not routed): the prover makes a proof with an honest transcript and proof of work whose t(zeta)
    is not vanishing(zeta) / Z_H(zeta).  prove(data, wires, pis) -> (bytes, verifier_only); default: the oracle's C prover."""
    from oracle import cport
    if prove is None:
        def prove(d, w, p):
            raw, _, vd = cport.plonky2_prove(d, w, p, verifier_data=True)
            return raw, vd
    data, wires, pis = _synthetic("recursion", 6, seed=4)
    assert data.degree_bits == 6 and data.config["num_routed_wires"] <= 100
    common = data.common_data()
    for row in np.nonzero(wires[100])[0]:
        bad = wires.copy()
        bad[100, row] = (int(bad[100, row]) + 1) % P
        raw, vd = prove(data, bad, pis)
        if oracle_status(S.proof_from_bytes(raw, common, HASH_GL), vd, common) == PROOF_BAD_VANISHING:
            return data, vd, raw
    raise AssertionError("no PoseidonGate row in the synthetic circuit")


def test_vanishing_is_reached_honestly():
    data, vd, raw = vanishing_case()
    common = data.common_data()
    assert oracle_status(S.proof_from_bytes(raw, common, HASH_GL), vd, common) == PROOF_BAD_VANISHING
    with Verifier(None, common, vd) as v:
        assert v.verify_batch([raw]) == [PROOF_BAD_VANISHING]


def _gate_codes(common):
    from zklc_amd.plonky2 import gates as G
    return {G.gate_from_id(g).code for g in common["gates"]}


def _oracle_prover_cases():
    """(name, common, verifier_only, proof bytes, hasher) over circuits that together hold all 22 gate types"""
    from oracle import cport, plonky2_prover as OP
    from zklc_amd.plonky2 import sha256 as SHA
    out = []
    for shape in ("recursion", "ed25519"):
        data, wires, pis = _synthetic(shape, 6)
        common = data.common_data()
        raw, _, vd = cport.plonky2_prove(data, wires, pis, verifier_data=True)
        out.append((shape + "/gl", common, vd, raw, HASH_GL))
        oproof, ovd = OP.prove(common, data.constants, data.sigmas, wires, pis, V.HasherBN128)
        out.append((shape + "/bn128", common, ovd, S.proof_to_bytes(oproof, common, HASH_BN128), HASH_BN128))
    data, words = SHA.sha256_circuit(1)
    pw = SHA.sha256_witness(words, b"\x60")
    data.witness_program(list(pw))
    wn, pn = data.generate_witness_native([pw])
    raw, _, vd = cport.plonky2_prove(data, wn[0], [int(x) for x in pn[0]], verifier_data=True)
    out.append(("sha256/gl", data.common_data(), vd, raw, HASH_GL))
    return out


@pytest.fixture(scope="module")
def oracle_prover_cases():
    return _oracle_prover_cases()


def test_oracle_prover_proofs_over_all_gate_types(oracle_prover_cases):
    codes = set()
    for name, common, vd, raw, hasher in oracle_prover_cases:
        codes |= _gate_codes(common)
        with Verifier(None, common, vd, hasher) as v:
            assert v.verify_batch([raw]) == [PROOF_OK], name
            pj = S.proof_from_bytes(raw, common, hasher)
            for what in ("initial_leaf", "step_eval_within", "wires_opening"):
                t = tamper(pj, common, vd, what)
                assert v.verify_batch([t]) == [expected_status(t, vd, common, what)], (name, what)
    assert codes == set(range(22)), sorted(set(range(22)) - codes)


def test_mixed_batch_reports_each_proof(golden_cases, oracle_prover_cases):
    """valid and tampered proofs in one batch: each element gets its own status; every status code occurs"""
    c = golden_cases[0]
    common, vd = c["common_data"], c["verifier_data"]
    batch, want = [], []
    for i, what in enumerate([None, "pow_witness", "initial_sibling", None, "step_eval_within", "non_canonical", "initial_leaf", None]):
        t = c["proof"] if what is None else tamper(c["proof"], common, vd, what)
        batch.append(S.proof_to_bytes(t, common, HASH_BN128))
        want.append(PROOF_OK if what is None else expected_status(t, vd, common, what))
    batch.append(batch[0][:-8])          # a proof of the wrong length
    want.append(PROOF_BAD_FORMAT)
    with Verifier(None, common, vd) as v:
        assert v.verify_batch(batch, threads=3) == want
        assert v.verify_batch_host(batch, threads=1) == want
    data, vd2, raw = vanishing_case()
    with Verifier(None, data.common_data(), vd2) as v2:
        want.append(v2.verify_batch([raw])[0])
    assert set(want) == {PROOF_OK, PROOF_BAD_FORMAT, PROOF_BAD_POW, PROOF_BAD_VANISHING, PROOF_BAD_MERKLE, PROOF_BAD_FRI}


def test_same_verifier_two_ways():
    """a verifier from the CircuitData's own common data and one from its common_data() JSON text agree"""
    from oracle import cport
    from zklc_amd.plonky2.container import native_arguments
    from zklc_amd.plonky2.verifier import native_arguments_from_common
    data, wires, pis = _synthetic("recursion", 6, seed=9)
    raw, _, vd = cport.plonky2_prove(data, wires, pis, verifier_data=True)
    a = native_arguments(data, HASH_GL)
    b = native_arguments_from_common(json.loads(json.dumps(data.common_data())), HASH_GL)
    assert bytes(a[0]) == bytes(b[0]) and bytes(a[1]) == bytes(b[1])
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    bad = bytearray(raw)
    bad[-9] ^= 1                          # the last public input
    with Verifier(None, data.common_data(), vd) as v1, Verifier(None, json.loads(json.dumps(data.common_data())), vd) as v2:
        assert v1.verify_batch([raw, bytes(bad)]) == v2.verify_batch([raw, bytes(bad)]) == [PROOF_OK, PROOF_BAD_POW]


def test_unsupported_circuits_are_refused(golden_cases):
    c = golden_cases[0]
    zk = copy.deepcopy(c["common_data"])
    zk["fri_params"]["hiding"] = True
    with pytest.raises(ValueError):
        Verifier(None, zk, c["verifier_data"])
    lk = copy.deepcopy(c["common_data"])
    lk["num_lookup_polys"] = 2
    with pytest.raises(ValueError):
        Verifier(None, lk, c["verifier_data"])


def test_proof_argument_kinds(golden_cases):
    """bytes of the wrong length and a proof.json of another shape are BAD_FORMAT verdicts; an object that is no proof at all is
    the caller's error"""
    c = golden_cases[0]
    with Verifier(None, c["common_data"], c["verifier_data"]) as v:
        short = copy.deepcopy(c["proof"])
        short["proof"]["opening_proof"]["query_round_proofs"].pop()
        huge = copy.deepcopy(c["proof"])
        huge["proof"]["openings"]["wires"][0][0] = 2**64
        assert v.verify_batch([b"\0" * 10, short, huge]) == [PROOF_BAD_FORMAT] * 3
        with pytest.raises(TypeError):
            v.verify_batch([42])
