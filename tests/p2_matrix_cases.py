"""The parameter matrix of the plonky2 prover and verifier (tests/test_p2_matrix_host.py, tests/test_gpu_p2_matrix.py): circuit sizes
from 2^2 to 2^14 rows and every FRI parameter that zklc_plonky2_circuit_create / zklc_plonky2_verifier_create accept and the code
branches on -- reduction arities 2^1 .. 2^5, no reduction at all, cap heights from 0 to the LDE's own height, 1 / 2 challenges,
proof-of-work bits, query rounds, routed wires that leave the permutation argument a partial last chunk.

A case is a name, a circuit shape, a size and the entries it changes in a copy of the standard (135 wires) or wide (234 wires)
configuration.  make(case) builds the circuit with a satisfying witness; reference(case) is the oracle's C prover's proof of it and
its verifier data, computed once per case, hasher and process; batch(case) is that proof followed by its tampered copies."""
import collections

from oracle import cport
from zklc_amd.plonky2 import CircuitBuilder, serialization as S, HASH_GL, HASH_BN128
from zklc_amd.plonky2 import synthetic as SY, gates as G, standard_recursion_config, wide_ecc_config
from test_plonky2_verifier_host import tamper

Case = collections.namedtuple("Case", "name shape degree_bits over")
C_PROVER_THREADS = 8
# tampered copies, in this order after the good proof: circuits with a FRI reduction / without one (no step evaluations there)
KINDS = ["initial_leaf", "step_eval_within", "step_eval_other", "initial_sibling", "pow_witness", "non_canonical", "public_input"]
KINDS_NO_REDUCTION = ["initial_leaf", "initial_sibling", "pow_witness", "non_canonical", "public_input", "final_poly", "wires_opening"]
TINY_CHAIN = {2: 0, 3: 40, 4: 200, 5: 500}     # degree_bits -> mul_add operations (20 to a row) after the one public input


def _case(name, shape, degree_bits, **over):
    return Case(name, shape, degree_bits, tuple(sorted(over.items())))


SIZE_CASES = ([_case("tiny-2^%d" % d, "tiny", d) for d in (2, 3, 4, 5)] +
              [_case("ed25519-2^%d" % d, "ed25519", d) for d in (5, 8, 10, 11, 14)] +
              [_case("recursion-2^%d" % d, "recursion", d) for d in (7, 8, 9, 10, 11, 14)])
# ConstantArityBits [a, f] at 2^7: [1,0] -> [1]*6, [1,2] -> [1]*5, [1,5] -> [1,1], [2,0] / [2,2] -> [2,2,2], [2,5] -> [2],
# [3,0] / [3,2] -> [3,3], [3,5] -> [3], [5,*] -> [5]
ARITIES_AT_2P7 = {(1, 0): [1] * 6, (1, 2): [1] * 5, (1, 5): [1, 1], (2, 0): [2, 2, 2], (2, 2): [2, 2, 2], (2, 5): [2],
                  (3, 0): [3, 3], (3, 2): [3, 3], (3, 5): [3], (5, 0): [5], (5, 2): [5], (5, 5): [5]}
PARAMETER_CASES = ([_case("arity-%d-%d" % af, "recursion", 7, arity=af) for af in ARITIES_AT_2P7] +
                   [_case("cap-%d" % h, "recursion", 6, cap=h) for h in (0, 1, 2, 7, 9)] +
                   # 5 / 6: the last value whose search range is smaller than one workgroup of the prover's kernel, and the first full one
                   [_case("pow-%d" % b, "recursion", 6, pow=b) for b in (1, 5, 6, 8, 20)] +
                   [_case("rounds-%d" % q, "recursion", 6, rounds=q) for q in (1, 3, 84)] +
                   [_case("challenges-1", "recursion", 6, nch=1)] +
                   [_case("routed-%d" % w, "recursion", 6, routed=w) for w in (73, 79, 81)] +
                   [_case("combined-2^9", "recursion", 9, arity=(3, 5), cap=1, nch=1, pow=5, rounds=3, routed=73)])
CASES = SIZE_CASES + PARAMETER_CASES
THREE_CHALLENGES = _case("challenges-3", "recursion", 6, nch=3)     # the host verifier takes it; the GPU prover holds two (P2_MAX_CH)
BY_NAME = {c.name: c for c in CASES + [THREE_CHALLENGES]}
BN128_CASES = [BY_NAME[k] for k in ("arity-2-2", "cap-0", "cap-7", "routed-73")]      # against the Python restatement
LEAN_OFF_CASES = [BY_NAME[k] for k in ("arity-2-2", "cap-0", "routed-73", "combined-2^9")]
assert len(CASES) == 45 and len(BY_NAME) == 46
# Poseidon-BN128 against the C prover: every case of at most 2^11 rows, and two sizes of its own -- 2^12 rows (trees of 2^15 leaves:
# the wrap's size, leaf digests from the one-lane kernel) and 2^13 rows (2^16 leaves: a one-lane tree level inside a proof)
BN128_SIZE_CASES = [_case("recursion-2^%d" % d, "recursion", d) for d in (12, 13)]
BN128_C_CASES = [c for c in CASES if c.degree_bits <= 11] + BN128_SIZE_CASES
BY_NAME.update({c.name: c for c in BN128_SIZE_CASES})
assert len(BN128_C_CASES) == 43 + 2 and len(BY_NAME) == 48


def config(case):
    cfg = wide_ecc_config() if case.shape == "ed25519" else standard_recursion_config()
    fri = cfg["fri_config"]
    for key, val in case.over:
        if key == "arity":
            fri["reduction_strategy"] = {"ConstantArityBits": list(val)}
        elif key == "cap":
            fri["cap_height"] = val
        elif key == "pow":
            fri["proof_of_work_bits"] = val
        elif key == "rounds":
            fri["num_query_rounds"] = val
        elif key == "nch":
            cfg["num_challenges"] = val
        elif key == "routed":
            cfg["num_routed_wires"] = val
        else:
            raise KeyError(key)
    return cfg


_MADE, _REFERENCE, _BATCH = {}, {}, {}


def make(case):
    """-> (CircuitData, wires uint64 [num_wires, n], public inputs)"""
    if case.name not in _MADE:
        cfg = config(case)
        if case.shape == "tiny":
            b = CircuitBuilder(cfg)
            x = b.add_virtual_public_input()
            acc = x
            for _ in range(TINY_CHAIN[case.degree_bits]):
                acc = b.mul_add(acc, x, x)
            data = b.build()
            wires, pis = data.generate_witness({x: 0xFFFFFFFF00000000})       # p - 1
        else:
            if case.shape == "recursion":
                mix = SY.recursion_shape_mix(cfg) + [(G.ExponentiationGate(20), 3)]
            else:
                mix = SY.ed25519_shape_mix(cfg)
            data, wires, pis = SY.synthetic_circuit(case.degree_bits, cfg, mix, num_public_inputs=11, seed=3)
        assert data.degree_bits == case.degree_bits, (case.name, data.degree_bits)
        if "arity" in dict(case.over) and case.degree_bits == 7:
            assert data.fri_arity_bits == ARITIES_AT_2P7[dict(case.over)["arity"]], (case.name, data.fri_arity_bits)
        _MADE[case.name] = (data, wires, pis)
    return _MADE[case.name]


def reference(case, hasher=HASH_GL):
    """-> (proof bytes, verifier data) of the oracle's C prover"""
    if (case.name, hasher) not in _REFERENCE:
        data, wires, pis = make(case)
        raw, _, vd = cport.plonky2_prove(data, wires, pis, nthreads=C_PROVER_THREADS, verifier_data=True, hasher=hasher)
        _REFERENCE[case.name, hasher] = (raw, vd)
    return _REFERENCE[case.name, hasher]


def kinds(case):
    """the tampered copies of the case's proof: the kinds that exist in it (a cap as tall as the tree leaves no sibling: the cap
    entry the opening ends at is changed instead)"""
    data = make(case)[0]
    fri = data.config["fri_config"]
    out = list(KINDS if data.fri_arity_bits else KINDS_NO_REDUCTION)
    if fri["cap_height"] >= data.degree_bits + fri["rate_bits"]:
        out[out.index("initial_sibling")] = "wires_cap"
    return out


def tampered(raw, common, vd, what, hasher=HASH_GL):
    return S.proof_to_bytes(tamper(S.proof_from_bytes(raw, common, hasher), common, vd, what), common, hasher)


def batch(case, hasher=HASH_GL):
    """-> [the C prover's proof] + one tampered copy per kind of kinds(case), as bytes"""
    if (case.name, hasher) not in _BATCH:
        raw, vd = reference(case, hasher)
        common = make(case)[0].common_data()
        _BATCH[case.name, hasher] = [raw] + [tampered(raw, common, vd, k, hasher) for k in kinds(case)]
    return _BATCH[case.name, hasher]
