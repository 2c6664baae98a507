"""The oracle's C Poseidon-BN254 (oracle/c/poseidon_bn254_oracle.c) against its definition (oracle/poseidon_bn254.py) and the
reference's golden proofs: the permutation, the plonky2 hasher on it, the tree builder, and every Merkle path of the four golden
wrap proofs.  The C is what tests/test_gpu_bn254_merkle.py and the Poseidon-BN128 proof parity tests compare the library with."""
import gzip
import itertools
import json
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import cport, poseidon_bn254 as pbn, plonky2_verifier as V
import bn254_merkle_cases as MC
import devsim_vectors as DV

EDGE_FR = [0, 1, pbn.R - 1, pbn.R - 2, 2**192 - 1, 2**253]


def test_permutation_kats():
    """crypto/plonky2_bn128/src/poseidon_bn128.rs:133-180"""
    assert len(pbn.KATS) == 4
    for k in pbn.KATS:
        assert cport.pbn_permute(k["in"]) == k["out"]


def test_permutation_random_and_edge_states():
    rng = random.Random(11)
    states = [[rng.randrange(pbn.R) for _ in range(4)] for _ in range(2000)]
    states += [list(s) for s in itertools.product(EDGE_FR, repeat=4)]
    assert len(states) == 2000 + 6**4
    got = cport.pbn_permute_many(states)
    for s, g in zip(states, got):
        assert g == pbn.permute(s), s


def _leaves(width, rng):
    """a random leaf, a leaf of edge values only, and a mixed one"""
    out = [[rng.randrange(MC.P) for _ in range(width)], [rng.choice(DV.CANON) for _ in range(width)],
           [rng.choice(DV.CANON) if rng.random() < 0.5 else rng.randrange(MC.P) for _ in range(width)]]
    for v in (MC.P - 1, 0):
        out.append([v] * width)
    return out


@pytest.mark.parametrize("width", list(range(29)) + [36, 85, 135])
def test_hash_or_noop(width):
    rng = random.Random(100 + width)
    for leaf in _leaves(width, rng):
        assert cport.pbn_hash_or_noop(leaf) == pbn.hash_or_noop(leaf), leaf
        assert cport.pbn_hash_no_pad(leaf) == pbn.hash_no_pad(leaf), leaf


def test_two_to_one():
    rng = random.Random(5)
    pairs = [(rng.randrange(pbn.R), rng.randrange(pbn.R)) for _ in range(200)] + list(itertools.product(EDGE_FR, repeat=2))
    for l, r in pairs:
        assert cport.pbn_two_to_one(l, r) == pbn.two_to_one(l, r), (l, r)


@pytest.mark.parametrize("case", [MC.Case(10, 6, 2, "random"), MC.Case(3, 4, 0, "random")], ids=MC.name)
def test_tree_every_level(case):
    mat = MC.matrix(case)
    layer = [pbn.hash_or_noop([int(mat[c, i]) for c in range(case.width)]) for i in range(1 << case.log_leaves)]
    one, four = MC.reference(case, 1), MC.reference(case, 4)
    assert MC.first_difference(case, four, one) is None
    assert [lv.shape[0] for lv in one] == MC.level_sizes(case)
    for lv in one:
        assert cport.fr_ints(lv) == layer
        layer = [pbn.two_to_one(layer[2 * i], layer[2 * i + 1]) for i in range(len(layer) // 2)]


def test_tree_of_every_case_of_the_gpu_sweep():
    """the oracle alone handles every small case the GPU tests hand it, with the same levels for 1 and 8 threads, and
    first_difference names the level and index of a changed digest"""
    for case in MC.CHILD_CASES + MC.STRIDED_CASES[:1]:
        one, many = MC.reference(case, 1), MC.reference(case)
        assert MC.first_difference(case, many, one) is None
        assert [lv.shape for lv in one] == [(m, 4) for m in MC.level_sizes(case)]
        flat = np.concatenate([lv.reshape(-1) for lv in one])
        assert MC.first_difference(case, MC.split_levels(case, flat), one) is None
    case = MC.Case(10, 6, 2, "random")
    one = MC.reference(case, 1)
    bad = [lv.copy() for lv in one]
    bad[2][5, 1] ^= np.uint64(1)
    assert "level 2 (16 digests) differs first at index 5 " in MC.first_difference(case, bad, one)


def test_dispatch_rule_of_the_threshold_cases():
    """which kernels the cases of tests/test_gpu_bn254_merkle.py reach, from the rule restated in bn254_merkle_cases.py"""
    for case, leaf, lane_levels in MC.THRESHOLD_CASES:
        got_leaf, levels = MC.dispatch(case)
        assert got_leaf == leaf and levels.count("lane") == lane_levels, MC.name(case)
        assert levels == ["lane"] * lane_levels + ["coop"] * (len(levels) - lane_levels)
    c = MC.Case(4, 5, 0, "random")
    assert MC.dispatch(c, "0") == ("lane", ["lane"] * 5)
    assert MC.dispatch(c, "3") == ("lane", ["lane", "coop", "coop", "coop", "coop"])      # 16 parents, then 8, 4, 2, 1
    assert MC.dispatch(MC.Case(4, 3, 0, "random"), "3") == ("coop", ["coop"] * 3)


def test_every_merkle_path_of_the_golden_wrap_proofs():
    """all 28 query rounds of the reference's four golden proofs: the four initial-tree paths and every FRI path, walked with the
    C hasher, end in the proof's own cap entry"""
    with gzip.open(os.path.join(GOLDEN, "plonky2_reference_proofs_full.json.gz")) as f:
        cases = json.load(f)
    assert len(cases) == 4

    def walk(leaf, index, siblings):
        cur = cport.pbn_hash_or_noop(leaf)
        for s in siblings:
            cur = cport.pbn_two_to_one(s, cur) if index & 1 else cport.pbn_two_to_one(cur, s)
            index >>= 1
        return cur, index

    for c in cases:
        pf = V.parse_proof(c["proof"], c["verifier_data"])
        assert pf["hasher"] is V.HasherBN128 and len(pf["rounds"]) == 28, c["source"]
        fp = c["common_data"]["fri_params"]
        n_log = fp["degree_bits"] + fp["config"]["rate_bits"]
        idx = V.challenges(pf, c["common_data"])["query_indices"]
        caps = [pf["constants_sigmas_cap"], pf["wires_cap"], pf["zs_pp_cap"], pf["quotient_cap"]]
        walked = 0
        for rnd, (init, steps) in enumerate(pf["rounds"]):
            x_index = idx[rnd] % (1 << n_log)
            for k in range(4):
                cur, top = walk(init[k][0], x_index, init[k][1])
                assert cur == caps[k][top], (c["source"], rnd, k)
                walked += 1
            i = x_index
            assert len(steps) == len(fp["reduction_arity_bits"])
            for a, ((evals, sib), arity_bits) in enumerate(zip(steps, fp["reduction_arity_bits"])):
                i >>= arity_bits
                cur, top = walk([x for e in evals for x in e], i, sib)
                assert cur == pf["commit_caps"][a][top], (c["source"], rnd, a)
                walked += 1
        assert walked == 28 * (4 + len(fp["reduction_arity_bits"]))


def test_trees_of_the_threshold_cases_on_sampled_paths():
    """the full trees the GPU tests compare with (up to 2^16 leaves): the oracle builds each, and on sampled leaves the digest and
    the whole path to the cap are the Python definition's"""
    rng = random.Random(3)
    for case in [c for c, _, _ in MC.THRESHOLD_CASES] + MC.STRIDED_CASES[1:]:
        mat, levels = MC.matrix(case), MC.reference(case)
        assert [lv.shape for lv in levels] == [(m, 4) for m in MC.level_sizes(case)]
        n = 1 << case.log_leaves
        for i in [0, n - 1, n // 2 - 1, n // 2] + [rng.randrange(n) for _ in range(2)]:
            assert cport.fr_ints(levels[0][i])[0] == pbn.hash_or_noop([int(x) for x in mat[:, i]]), (MC.name(case), i)
            for l in range(1, len(levels)):
                i >>= 1
                left, right = cport.fr_ints(levels[l - 1][2 * i:2 * i + 2])
                assert cport.fr_ints(levels[l][i])[0] == pbn.two_to_one(left, right), (MC.name(case), l, i)
