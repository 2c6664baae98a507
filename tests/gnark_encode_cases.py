"""Shared by tests/test_gnark_encode_host.py and tests/test_gpu_gnark_encode.py (not a test module): records in gnark-crypto's memory
layout (Montgomery words) for the point encoders zklc_bn254_g{1,2}_encode_{host,dev}, with the expected class and slot of each.

The expectation of a record comes from Python alone, never from the code under test: the slot of an accepted record is `write_g1` /
`write_g2` on `words_to_points` of the record; a record with a coordinate whose eight words are >= p is BAD_ENCODING by rule; with
validation, a record that fails the curve equation in Python integers is NOT_ON_CURVE; the slot of a rejected record is all 0xFF.

The pattern is eight rounds of at most 32 records.  Every round holds every class and every kind of ordering edge (the word that
differs from (p - 1) / 2 is word r in round r), shuffled so that neighbouring lanes take different branches; an array is the
pattern repeated, so every 64 consecutive records hold a whole round (tests/test_gnark_encode_host.py asserts it)."""
import functools
import random

import numpy as np

import gnark_point_cases as PC
from oracle import bn254 as B
from zklc_amd import gnark_keys as K

P = B.P
HALF = (P - 1) // 2
OK, INFINITY, BAD_ENCODING, NOT_ON_CURVE = range(4)
ALL_ONES = (1 << 64) - 1
ROUNDS, ROUND_MAX, WINDOW = 8, 32, 64
EDGE_KINDS = ("y = 1", "y = (p - 1) / 2", "y = (p + 1) / 2", "y = p - 1", "one word above (p - 1) / 2", "one word below (p - 1) / 2")


def edge_tags(g2):
    """the tags of the ordering edges every round must hold"""
    if not g2:
        return ["edge: " + k for k in EDGE_KINDS]
    return ["edge, A1 = 0: " + k for k in EDGE_KINDS] + ["edge, A1 != 0: " + k for k in EDGE_KINDS]


def _edge_values(r):
    """the six y of round r; the one-word neighbours of (p - 1) / 2 differ from it in u32 word r alone (no word of it is 0 or
    2^32 - 1, so there is no carry)"""
    vals = [1, HALF, HALF + 1, P - 1, HALF + (1 << (32 * r)), HALF - (1 << (32 * r))]
    for v in vals[4:]:
        diff = [i for i in range(8) if (v >> (32 * i)) & 0xffffffff != (HALF >> (32 * i)) & 0xffffffff]
        assert diff == [r] and 0 < v < P
    return vals


def _int_words(v):
    """an integer below 2^256 as four u64 words, as it is (NOT into the Montgomery domain)"""
    return [(v >> (64 * i)) & ALL_ONES for i in range(4)]


def _coord_ints(words):
    w = [int(x) for x in words]
    return [sum(w[4 * j + i] << (64 * i) for i in range(4)) for j in range(len(w) // 4)]


def _on_curve(pt, g2):
    if not g2:
        x, y = pt
        return (y * y - x * x * x - 3) % P == 0
    x, y = pt
    b = K._twist_b()
    rhs = K._fp2_mul(K._fp2_mul(x, x), x)
    return K._fp2_mul(y, y) == ((rhs[0] + b[0]) % P, (rhs[1] + b[1]) % P)


def classify(words, g2, validate):
    """the class of one record, in Python integers"""
    c = _coord_ints(words)
    if not any(c):
        return INFINITY
    if any(v >= P for v in c):
        return BAD_ENCODING
    if validate and not _on_curve(K.words_to_points(np.array([words], dtype=np.uint64), g2=g2)[0], g2):
        return NOT_ON_CURVE
    return OK


def slot(words, g2, compressed, validate):
    """-> (class, slot bytes) of one record"""
    cls = classify(words, g2, validate)
    stride = (128 if g2 else 64) >> (1 if compressed else 0)
    if cls >= BAD_ENCODING:
        return cls, b"\xff" * stride
    pt = K.words_to_points(np.array([words], dtype=np.uint64), g2=g2)[0]
    assert (pt is None) == (cls == INFINITY)
    out = (K.write_g2 if g2 else K.write_g1)(pt, not compressed)
    assert len(out) == stride
    return cls, out


@functools.lru_cache(maxsize=None)
def _build(g2):
    """-> (records, extents of the rounds)"""
    width, ncoord = (16, 4) if g2 else (8, 2)
    gen, mul, neg = (B.G2, B.g2_mul, B.g2_neg) if g2 else (B.G1, B.mul, B.neg)
    one = lambda pt: K.points_to_words([pt], g2=g2)[0]
    accepted = [c[4] for c in PC.cases(g2, False) if c[1] == PC.OK]
    bad_values = [(v, j) for j in range(ncoord) for v in (P, P + 1, (1 << 256) - 1)]
    outside = PC.twist_point_outside_g2() if g2 else None
    out, bounds = [], []
    for r in range(ROUNDS):
        rnd = []
        add = lambda words, tag: rnd.append((np.array(words, dtype=np.uint64), tag))
        # the OK and INFINITY words of the decoder's cases
        for j in (2 * r, 2 * r + 1):
            add(accepted[j % len(accepted)], "decoder case")
        add(np.zeros(width, dtype=np.uint64), "infinity")
        # ordering edges: the coordinates need not be on a curve (validation off); x differs from record to record
        for kind, y in zip(EDGE_KINDS, _edge_values(r)):
            if not g2:
                add(one((5 + r, y)), "edge: " + kind)
            else:
                add(one(((5 + r, 7), (y, 0))), "edge, A1 = 0: " + kind)
                add(one(((9, 11 + r), (P - 1 if r & 1 else 1, y))), "edge, A1 != 0: " + kind)
        # not infinity: x = 0 with y != 0, and a record whose last word alone is non-zero (y, or Y.A1, is 2^192 in Montgomery form)
        add(one(((0, 0), (3 + r, 0))) if g2 else one((0, 3 + r)), "x = 0, y != 0")
        add([0] * (width - 1) + [1], "only the last word non-zero")
        # coordinates that are not canonical, each value in every coordinate position over the rounds
        base = one(mul(3 + r, gen))
        for v, j in (bad_values[(2 * r) % len(bad_values)], bad_values[(2 * r + 1) % len(bad_values)]):
            w = [int(x) for x in base]
            w[4 * j:4 * j + 4] = _int_words(v)
            add(w, "coordinate %d = %s" % (j, "p" if v == P else "p + 1" if v == P + 1 else "2^256 - 1"))
        # for validation: a multiple, the same with y negated, the same with one word changed, a twist point outside G2
        pt = mul(1000 + 37 * r, gen)
        add(one(pt), "multiple")
        add(one(neg(pt)), "multiple, -y")
        w = [int(x) for x in one(pt)]
        w[(3 * r + 1) % width] ^= 1
        assert all(v < P for v in _coord_ints(w))
        add(w, "multiple, one word changed")
        if g2:
            q = outside
            for _ in range(r % 3):
                q = B.g2_add(q, outside)
            add(one(q), "twist point outside G2")
        random.Random(40 + 8 * g2 + r).shuffle(rnd)
        assert len(rnd) <= ROUND_MAX
        bounds.append((len(out), len(out) + len(rnd)))
        out += rnd
    return out, bounds


def pattern(g2):
    """-> list of (words uint64 [8 | 16], tag), ROUNDS rounds one after the other"""
    return _build(g2)[0]


def round_bounds(g2):
    """-> [(first, end)] of the rounds in pattern(g2)"""
    return _build(g2)[1]


@functools.lru_cache(maxsize=None)
def expected_pattern(g2, compressed, validate):
    """-> list of (class, slot bytes) for the records of pattern(g2)"""
    return [slot(w, g2, compressed, validate) for w, _ in pattern(g2)]


def words(g2, n, start=0):
    """n records cycling through the pattern from `start` -> uint64 [n, 8 | 16]"""
    pat = pattern(g2)
    if not n:
        return np.zeros((0, 16 if g2 else 8), dtype=np.uint64)
    return np.stack([pat[(start + i) % len(pat)][0] for i in range(n)])


def expected(g2, compressed, validate, n, start=0):
    """-> (bytes, status uint32 [n], summary [OK, infinity, rejected, first rejected index | None]) of words(g2, n, start)"""
    exp = expected_pattern(g2, compressed, validate)
    pick = [exp[(start + i) % len(exp)] for i in range(n)]
    status = np.array([c for c, _ in pick], dtype=np.uint32)
    rej = np.nonzero(status >= BAD_ENCODING)[0]
    summary = [int((status == OK).sum()), int((status == INFINITY).sum()), int(len(rej)), int(rej[0]) if len(rej) else None]
    return b"".join(s for _, s in pick), status, summary
