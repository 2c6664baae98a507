#!/usr/bin/env python3
"""Verifying keys and proofs for the batched Groth16 verifier's tests, from this repository's own oracle
(oracle.groth16.square_chain_r1cs / setup / prove with fixed toxic values and blinding scalars): for n_public in {3, 40} one key
and three proofs, each with its own public inputs.  Written to tests/golden/groth16_batch.json (decimal strings; a G1 point is
[x, y], a G2 point [[x0, x1], [y0, y1]]; a proof is the eight words of gnark's WriteRawTo order).

    python tests/golden/make_groth16_batch_fixture.py            # ~3 minutes: setup and prove are plain Python
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import groth16 as G  # noqa: E402

TOXIC = (0x1234567891, 0xabcdef12345, 0x777766665555, 0x3133731337, 0x42424242)
N_CONSTRAINTS = 60


def public_inputs(n_public, k):
    if k == 0:
        return [5 + i for i in range(n_public)]
    if k == 1:   # large field elements, every one nonzero
        return [(G.R - 1 - 977 * i * i) % G.R for i in range(n_public)]
    return [pow(7, 11 * i + 3, G.R) for i in range(n_public)]


def main():
    out = {"source": "oracle.groth16 (square_chain_r1cs, %d constraints; toxic values and blinding scalars fixed in "
                     "tests/golden/make_groth16_batch_fixture.py)" % N_CONSTRAINTS, "keys": []}
    s = lambda pt: [str(pt[0]), str(pt[1])]
    s2 = lambda pt: [[str(pt[0][0]), str(pt[0][1])], [str(pt[1][0]), str(pt[1][1])]]
    for n_public in (3, 40):
        r1cs, wit = G.square_chain_r1cs(N_CONSTRAINTS, n_public=n_public)
        pk, vk = G.setup(r1cs, n_public, TOXIC)
        entry = {"n_public": n_public,
                 "vk": {"alpha1": s(vk["alpha1"]), "beta2": s2(vk["beta2"]), "gamma2": s2(vk["gamma2"]), "delta2": s2(vk["delta2"]),
                        "K": [s(p) for p in vk["K"]]},
                 "proofs": []}
        for k in range(3):
            pubs = public_inputs(n_public, k)
            w = wit(pubs, 11 + k)
            proof = G.prove(pk, r1cs, w, 0x1234 + 7 * k, 0x5678 + 13 * k)
            assert G.verify(vk, proof, pubs)
            entry["proofs"].append({"public_inputs": [str(x) for x in pubs], "proof": [str(x) for x in G.proof_to_uint256x8(proof)]})
            print("n_public", n_public, "proof", k, "ok", flush=True)
        out["keys"].append(entry)
    json.dump(out, open(os.path.join(HERE, "groth16_batch.json"), "w"), indent=1)
    print("wrote groth16_batch.json")


if __name__ == "__main__":
    main()
