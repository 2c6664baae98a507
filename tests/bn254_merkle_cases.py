"""The Poseidon-BN254 Merkle tree cases of tests/test_gpu_bn254_merkle.py and tests/test_oracle_c_bn254.py: the trees at the
dispatch thresholds of csrc/poseidon_bn254.hip, the width and dispatch sweep that runs once per ZKLC_BN254_COOP setting in a
child process, the edge-valued leaves, and the oracle's C tree builder (oracle/c/poseidon_bn254_oracle.c) as the reference of
all of them.

A case is (width, log_leaves, cap_height, fill).  matrix(case) is its poly-major leaf matrix uint64 [width, 2^log_leaves], the
same in every process; every value is canonical (< P), which is what the prover feeds the tree kernels."""
import collections
import zlib

import numpy as np

from oracle import cport
import devsim_vectors as DV

P = 2**64 - 2**32 + 1
ORACLE_THREADS = 8           # as C_PROVER_THREADS of p2_matrix_cases.py
Case = collections.namedtuple("Case", "width log_leaves cap fill")

# ---- the dispatch rule of zklc_bn254_merkle_commit_strided, restated: a launch of at most coop_max items (leaves, or parents of
# a level) takes the kernel with four lanes per permutation, a larger one the kernel with one lane per permutation.
# ZKLC_BN254_COOP=<k> sets coop_max = 2^k, 0 switches the four-lane kernels off; the library reads it once per process.
COOP_MAX_DEFAULT = 1 << 14
SETTINGS = [None, "0", "3"]                                  # the values of ZKLC_BN254_COOP the sweep runs under


def coop_max(setting):
    if setting is None:
        return COOP_MAX_DEFAULT
    k = int(setting)
    return 0 if k <= 0 else 1 << min(k, 30)


def dispatch(case, setting=None):
    """-> ("coop" | "lane" for the leaf kernel, the same for every level kernel, leaves' parents first)"""
    cm = coop_max(setting)
    kind = lambda items: "coop" if cm and items <= cm else "lane"
    n = 1 << case.log_leaves
    return kind(n), [kind(n >> (l + 1)) for l in range(case.log_leaves - case.cap)]


# ---- (a) full trees at the thresholds, default dispatch: case -> (leaf kernel, number of one-lane levels)
THRESHOLD_CASES = [
    (Case(9, 14, 4, "random"), "coop", 0),       # the largest tree hashed entirely four lanes per permutation
    (Case(4, 15, 4, "random"), "lane", 0),       # the smallest with one-lane leaves
    (Case(85, 15, 4, "random"), "lane", 0),      # the four trees of the wrap circuit: constants + sigmas,
    (Case(135, 15, 4, "random"), "lane", 0),     # wires,
    (Case(20, 15, 4, "random"), "lane", 0),      # Z + partial products,
    (Case(16, 15, 4, "random"), "lane", 0),      # quotient chunks
    (Case(4, 16, 4, "random"), "lane", 1),       # the smallest whose first level (2^15 parents) is hashed one lane per permutation
    (Case(32, 11, 4, "random"), "coop", 0),      # a FRI tree of the wrap
]
STRIDED_CASES = [Case(10, 6, 2, "random"), Case(4, 15, 4, "random")]
STRIDE_PAD = 24

# ---- (b) + (c): the sweep of every child
SWEEP_WIDTHS = list(range(1, 29)) + [32, 36, 85, 135]
SWEEP_CASES = list(dict.fromkeys([Case(w, 5, 0, "random") for w in SWEEP_WIDTHS] +
                                 [Case(w, l, c, "random") for w in (4, 10) for l in range(7) for c in sorted({0, l})]))
EDGE_CASES = ([Case(w, 5, 0, fill) for fill in ("pm1", "zero", "canon") for w in (9, 10, 135)] +
              # the leaf digests are the packed 192-bit values themselves: near-maximal children in two_to_one
              [Case(3, 6, 0, "pm1")])
CHILD_CASES = SWEEP_CASES + EDGE_CASES
assert len(SWEEP_CASES) == 32 + 2 * 13 - 2 and len(CHILD_CASES) == 66 and len(set(CHILD_CASES)) == 66      # (4 | 10, 5, 0) are in both


def name(case):
    return "w%d-l%d-c%d-%s" % case


def operands(rng, shape):
    """uniform canonical field elements with the canonical edge operands of tests/devsim_vectors.py in a quarter of the positions
    (as _operands of test_gpu_lean_arith.py)"""
    a = rng.integers(0, 2**64, size=shape, dtype=np.uint64)
    a = np.where(a >= np.uint64(P), a - np.uint64(P), a)
    edge = np.array(DV.CANON, dtype=np.uint64)
    pick = rng.integers(0, 4 * len(edge), size=shape)
    return np.where(pick < len(edge), edge[pick % len(edge)], a)


def matrix(case):
    shape = (case.width, 1 << case.log_leaves)
    if case.fill == "random":
        m = operands(np.random.default_rng(zlib.crc32(name(case).encode())), shape)
    elif case.fill == "pm1":
        m = np.full(shape, P - 1, dtype=np.uint64)
    elif case.fill == "zero":
        m = np.zeros(shape, dtype=np.uint64)
    elif case.fill == "canon":
        # leaf i holds CANON[(c + i) mod 13] in column c: over 13 consecutive leaves every value meets every column, and with it
        # every position of a 3-pack and of a 9-block
        assert shape[1] >= len(DV.CANON)
        c, i = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
        m = np.array(DV.CANON, dtype=np.uint64)[(c + i) % len(DV.CANON)]
    else:
        raise KeyError(case.fill)
    m = np.ascontiguousarray(m, dtype=np.uint64)
    assert m.shape == shape and int(m.max()) < P
    return m


def reference(case, nthreads=ORACLE_THREADS):
    """-> the levels of the oracle's C tree, leaves first ([m, 4] uint64 arrays)"""
    return cport.bn254_merkle_commit(matrix(case), case.cap, nthreads)


def level_sizes(case):
    return [1 << (case.log_leaves - l) for l in range(case.log_leaves - case.cap + 1)]


def split_levels(case, tree):
    """the flat tree (levels concatenated, 4 words a digest) -> levels"""
    tree = np.asarray(tree, dtype=np.uint64).reshape(-1)
    assert tree.size == 4 * sum(level_sizes(case)), (name(case), tree.size)
    out, off = [], 0
    for m in level_sizes(case):
        out.append(tree[off:off + 4 * m].reshape(m, 4))
        off += 4 * m
    return out


def first_difference(case, got, want):
    """None when every level is equal, else a text that names the first differing level (0: the leaf digests) and index"""
    assert len(got) == len(want) == len(level_sizes(case)), name(case)
    for l, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, (name(case), l, g.shape, w.shape)
        bad = np.nonzero((g != w).any(axis=1))[0]
        if bad.size:
            i = int(bad[0])
            return "%s: level %d (%d digests) differs first at index %d (%d differ): got %s, want %s" % (
                name(case), l, g.shape[0], i, bad.size, [hex(int(x)) for x in g[i]], [hex(int(x)) for x in w[i]])
    return None


# ---- the child of the sweep: every CHILD_CASES tree with the library's kernels, whole trees into one .npz
CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import numpy as np
import zklc_amd
import bn254_merkle_cases as MC
out = {}
with zklc_amd.Context(0) as ctx:
    for case in MC.CHILD_CASES:
        cap, levels = ctx.bn254_merkle_commit(MC.matrix(case), case.cap)
        out[MC.name(case)] = np.concatenate([l.reshape(-1) for l in levels])
np.savez(%(out)r, **out)
print("DONE %%d" %% len(out))
'''
