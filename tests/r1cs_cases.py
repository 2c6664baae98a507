"""Seeded constraint systems for the tests of zklc_amd/r1cs.py (NOT a test module): the CSR the C ABI takes, a satisfying witness,
witnesses broken at chosen constraints, and the expected a = A w, b = B w, c = C w and summary computed with Python integers
(converted with fr_to_mont_words).  Shared by tests/test_r1cs_host.py and tests/test_gpu_r1cs.py; every system and every
expectation is computed once per session.

Construction: the rows of A and B are chosen freely over the `free` wires; row j of C is a free linear combination plus ONE fresh
wire n_free + j (coefficient 1, r - 1 or 2) whose value is solved for, so the system is satisfied by construction, and changing the
value of that wire breaks constraint j and no other.  (A C row without terms needs a_j b_j = 0: its A row is empty as well.)"""
import functools
import random

import numpy as np

from zklc_amd.groth16 import fr_to_mont_words, fr_to_regular_words
from zklc_amd.r1cs import BIN_LIMITS, R

# row lengths of the edge system: empty, one term, both sides of each bin limit, one / two passes of a wave's loop and a row of
# more than a thousand terms (every group size loops more than once)
EDGE_LENGTHS = sorted({0, 1, 2, 3, BIN_LIMITS[0], BIN_LIMITS[0] + 1, 8, 9, BIN_LIMITS[1], BIN_LIMITS[1] + 1, 64, 65, 129, 1037})


class System:
    def __init__(self, n_constraints, n_free, rows, values, witness):
        self.n_constraints, self.n_free = n_constraints, n_free
        self.n_wires = n_free + n_constraints
        self.rows = rows                      # 3 n_constraints lists of (wire, coefficient id): A's rows, then B's, then C's
        self.values = values                  # the dictionary as integers
        self.witness = witness                # satisfying, integers
        self.row_ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
        self.term_wire = np.array([w for r in rows for w, _ in r], dtype=np.uint32)
        self.term_coeff = np.array([c for r in rows for _, c in r], dtype=np.uint32)
        self.coeffs = np.array([fr_to_mont_words(v) for v in values], dtype=np.uint64).reshape(-1, 4)
        self.nnz = int(self.term_wire.size)

    def csr(self):
        return self.n_constraints, self.n_wires, self.row_ptr, self.term_wire, self.term_coeff, self.coeffs

    def fresh_wire(self, j):
        return self.n_free + j

    def broken(self, constraints):
        """the witness with the fresh wire of each listed constraint changed: exactly those constraints are violated"""
        w = list(self.witness)
        for j in constraints:
            assert any(wire == self.fresh_wire(j) for wire, _ in self.rows[2 * self.n_constraints + j]), "constraint %d has no fresh wire" % j
            w[self.fresh_wire(j)] = (w[self.fresh_wire(j)] + 1 + j) % R
        return w

    def row_values(self, witness):
        return [sum(self.values[c] * witness[w] for w, c in row) % R for row in self.rows]


def witness_words(witness):
    return np.array([fr_to_regular_words(x) for x in witness], dtype=np.uint64).reshape(-1, 4)


def expected(system, witness, n):
    """-> (a, b, c) uint64 [n, 4] in gnark's Montgomery layout (rows from n_constraints on are zero) and the summary
    (number of constraints with a_j b_j != c_j, index of the first one | None)"""
    nc = system.n_constraints
    v = system.row_values(witness)
    out = []
    for m in range(3):
        col = v[m * nc:(m + 1) * nc] + [0] * (n - nc)
        out.append(np.array([fr_to_mont_words(x) for x in col], dtype=np.uint64).reshape(-1, 4))
    bad = [j for j in range(nc) if (v[j] * v[nc + j] - v[2 * nc + j]) % R]
    return out[0], out[1], out[2], (len(bad), bad[0] if bad else None)


def _build(rng, n_free, lengths_abc, values, pick_id, free_values, special=()):
    """lengths_abc: per constraint the lengths of its A, B and C rows; special: (A row, B row, C free part) given explicitly"""
    fresh_ids = [i for i, v in enumerate(values) if v in (1, R - 1, 2)]
    plan = [(None, t) for t in lengths_abc] + [(sp, None) for sp in special]
    nc = len(plan)
    A, B, C = [], [], []
    witness = list(free_values) + [0] * nc
    term = lambda: (rng.randrange(n_free), pick_id())
    for j, (sp, lens) in enumerate(plan):
        if sp is not None:
            ra, rb, rc = [list(x) for x in sp]
            with_fresh = True
        else:
            la, lb, lc = lens
            with_fresh = lc > 0
            ra = [term() for _ in range(la if with_fresh else 0)]
            rb = [term() for _ in range(lb)]
            rc = [term() for _ in range(max(lc - 1, 0))]
        val = lambda row: sum(values[c] * witness[w] for w, c in row) % R
        if with_fresh:
            cid = fresh_ids[rng.randrange(len(fresh_ids))]
            witness[n_free + j] = (val(ra) * val(rb) - val(rc)) * pow(values[cid], R - 2, R) % R
            rc.insert(rng.randrange(len(rc) + 1), (n_free + j, cid))
        A.append(ra)
        B.append(rb)
        C.append(rc)
    return System(nc, n_free, A + B + C, values, witness)


def _dictionary(rng):
    """0, 1, r - 1, 2, r - 2, random values -- and two ids that hold the same value (1 twice, one random value twice)"""
    rnd = [rng.randrange(3, R - 2) for _ in range(5)]
    return [0, 1, R - 1, 2, R - 2, 1, rnd[0], rnd[0]] + rnd[1:]


def _picker(rng, values):
    n = len(values)

    def pick():
        x = rng.random()
        if x < 0.06:
            return 0                                            # a zero coefficient: the term is skipped
        if x < 0.55:
            return rng.choice([1, 2, 5])                        # +1 (both ids), -1
        return rng.randrange(3, n)
    return pick


@functools.lru_cache(maxsize=None)
def edge_system():
    rng = random.Random(20240611)
    values = _dictionary(rng)
    n_free = 48
    # witness values 0, 1, r - 1 and random; wire 0 is the constant 1
    free_values = [1, 0, R - 1, 1, 2, R - 2] + [rng.randrange(R) for _ in range(n_free - 6)]
    k = len(EDGE_LENGTHS)
    # every length occurs in every matrix; the C row of the first constraint has terms (a fresh wire to break)
    # (two passes with different offsets: the A row that goes with an empty C row is empty too, and is another length in each pass)
    lengths = [(EDGE_LENGTHS[j], EDGE_LENGTHS[(j + 4) % k], EDGE_LENGTHS[(j + 9) % k]) for j in range(k)]
    lengths += [(EDGE_LENGTHS[j], EDGE_LENGTHS[(j + 5) % k], EDGE_LENGTHS[(j + 7) % k]) for j in range(k)]
    assert lengths[0][2] > 0
    one, minus_one, one_again = 1, 2, 5
    special = [
        # a partial sum that lands exactly on r: w_3 + w_2 = 1 + (r - 1); times wire 0
        ([(3, one), (2, one)], [(0, one_again)], []),
        # (r - 1) (r - 1): the coefficient r - 1 on the wire that holds r - 1, on both sides
        ([(2, minus_one)], [(2, minus_one)], [(0, 3)]),
        # a wire repeated inside a row, with three different coefficients; wire 0 and the last free wire
        ([(7, one), (7, 6), (7, minus_one), (7, 8), (0, 4)], [(n_free - 1, 9), (n_free - 1, 9)], [(7, 7), (7, 6)]),
        # r - 2 times r - 1, 2 times r - 1
        ([(2, 4)], [(2, 3)], [(5, 4), (5, 3)]),
    ]
    s = _build(rng, n_free, lengths, values, _picker(rng, values), free_values, special)
    used = set(int(w) for w in s.term_wire)
    assert 0 in used and s.n_wires - 1 in used
    assert values[5] == values[1] and values[6] == values[7]
    for m in range(3):
        lens = {len(r) for r in s.rows[m * s.n_constraints:(m + 1) * s.n_constraints]}
        assert set(EDGE_LENGTHS) <= lens, "matrix %d misses a row length" % m
    return s


@functools.lru_cache(maxsize=None)
def random_system(n_constraints, seed=1):
    rng = random.Random(1000 * seed + n_constraints)
    values = _dictionary(rng)
    n_free = 24
    free_values = [1, 0, R - 1] + [rng.randrange(R) for _ in range(n_free - 3)]

    def length():
        x = rng.random()
        if x < 0.05:
            return 0
        if x < 0.70:
            return rng.randrange(1, BIN_LIMITS[0] + 2)
        if x < 0.95:
            return rng.randrange(BIN_LIMITS[0], BIN_LIMITS[1] // 2)
        return rng.randrange(BIN_LIMITS[1] - 2, BIN_LIMITS[1] + 40)
    lengths = [(length(), length(), max(length(), 1) if j in (0, n_constraints - 1) else length()) for j in range(n_constraints)]
    return _build(rng, n_free, lengths, values, _picker(rng, values), free_values)


@functools.lru_cache(maxsize=None)
def expected_cached(kind, arg, n, broken=()):
    """kind 'edge' (arg ignored) or 'random' (arg = n_constraints); broken: tuple of constraint indices"""
    s = edge_system() if kind == "edge" else random_system(arg)
    w = s.broken(broken) if broken else s.witness
    return (s, w) + expected(s, w, n)


def domain_size(n_constraints):
    n = 2
    while n < n_constraints:
        n *= 2
    return n
