"""Shared vectors of the fixed-base multiplication tests (tests/test_fixed_base_host.py, test_fixed_base_sanitized.py,
test_gpu_fixed_base.py): the edge scalars of a window width, the placements of zero scalars inside the groups that share an
inversion, the table digits in Python integers, and the expected points from oracle/bn254.py -- computed once per process."""
import functools
import random

import numpy as np

from oracle import bn254 as O

R = O.R
G1, G2 = 0, 1
INV_GROUP = 16            # csrc/bn254_fixed_mul.cuh FBM_INV_GROUP: point p of n is in group p % ceil(n / 16), at position p // ceil(n / 16)
SCALAR_BITS = 254
BASE_MULT = {G1: 7, G2: 5}                 # the non-generator bases: 7 G1 and 5 G2


def rows(c):
    return -(-SCALAR_BITS // c)


def digits(s, c):
    """the table digits of a scalar: digit k of s mod r selects entry (k, digit - 1), i.e. digit * 2^(c k) * P"""
    s %= R
    return [(s >> (c * k)) & ((1 << c) - 1) for k in range(rows(c))]


def edge_scalars(c):
    """what a window width c can get wrong: the ends of the range, values that are reduced first, a carry into and a borrow out of
    every window, the largest digit alone in every window, the largest value of the short top window, every digit the largest"""
    out = [0, 1, 2, R - 1, R - 2, R, R + 1, (1 << 256) - 1]
    n = rows(c)
    for k in range(n):
        if k:
            out += [1 << (c * k), (1 << (c * k)) - 1]
        m = ((1 << c) - 1) << (c * k)
        if m < R:
            out.append(m)
    top = c * (n - 1)
    out.append(((R - 1) >> top) << top)
    out.append(((1 << (c * n)) - 1) % R)
    return out


def random_scalars(k, seed):
    rng = random.Random(seed)
    return [rng.randrange(R) for _ in range(k)]


def table_probes():
    """(k, d) of a c = 16 table, each reached by the single-digit scalar d 2^(16 k): the first and the last entry of the first, of
    a middle and of the last row (whose digits end at r >> 240)"""
    return [(0, 1), (0, 0xffff), (7, 1), (7, 0xffff), (15, 1), (15, R >> 240)]


def oracle_scalars(group):
    """the scalars whose multiples the oracle computes (0.08 s each in G1, more in G2): the budget of the test suite"""
    ks5, ks13 = ((1, 25, 50), range(20)) if group == G1 else ((1, 50), (1, 10, 19))
    out = [0, 1, 2, R - 1, R - 2, R, R + 1, (1 << 256) - 1]
    for c, ks in ((5, ks5), (13, ks13)):
        e = edge_scalars(c)
        out += e[-2:]
        for k in ks:
            out += [1 << (c * k), (1 << (c * k)) - 1]
            if (((1 << c) - 1) << (c * k)) < R:
                out.append(((1 << c) - 1) << (c * k))
    out += [d << (16 * k) for k, d in table_probes()]
    out += random_scalars(16 if group == G1 else 8, 20 + group)
    seen, uniq = set(), []
    for s in out:
        if s not in seen:
            seen.add(s)
            uniq.append(s)
    return uniq


def point_words(group, pt):
    if group == G2:
        return tuple(O.g2_to_words(pt))
    return (0,) * 8 if pt is None else tuple(O.to_mont_words(pt[0]) + O.to_mont_words(pt[1]))


@functools.lru_cache(maxsize=None)
def base_point(group, generator=True):
    if generator:
        return O.G2 if group == G2 else O.G1
    return O.g2_mul(BASE_MULT[G2], O.G2) if group == G2 else O.mul(BASE_MULT[G1], O.G1)


@functools.lru_cache(maxsize=None)
def oracle_points(group):
    """{scalar mod r: words of scalar * generator}, the oracle's double-and-add in Python integers"""
    mul, g = (O.g2_mul, O.G2) if group == G2 else (O.mul, O.G1)
    out = {}
    for s in oracle_scalars(group):
        if s % R not in out:
            out[s % R] = point_words(group, mul(s % R, g))
    assert len(out) <= (150 if group == G1 else 60)
    return out


def other_base_scalars(group):
    return [0, 1, R - 1, (1 << 256) - 1] + random_scalars(6 if group == G1 else 3, 40 + group)


@functools.lru_cache(maxsize=None)
def other_base_points(group):
    mul = O.g2_mul if group == G2 else O.mul
    return [point_words(group, mul(s % R, base_point(group, False))) for s in other_base_scalars(group)]


def scalar_words(scalars):
    return np.array([[(int(s) >> (64 * i)) & ((1 << 64) - 1) for i in range(4)] for s in scalars], dtype=np.uint64).reshape(-1, 4)


def expected_words(group, scalars):
    pts = oracle_points(group)
    return np.array([pts[s % R] for s in scalars], dtype=np.uint64).reshape(len(scalars), 16 if group == G2 else 8)


def expected_summary(scalars):
    zeros = [i for i, s in enumerate(scalars) if s % R == 0]
    return len(zeros), (zeros[0] if zeros else None)


def zero_placements(group, n):
    """n scalars out of the oracle's set, none of them zero, then zeros (0 and r in turn) put where the shared inversion can go wrong:
    at the first position of group 0, at the last position of group 1, and all over group 2 (with fewer than three groups: what
    there is -- n = 1 is the one zero).  -> the scalars"""
    pool = [s for s in oracle_scalars(group) if s % R]
    s = [pool[(5 * i + n) % len(pool)] for i in range(n)]
    groups = -(-n // INV_GROUP)
    zero = [0, R]
    s[0] = zero[0]
    if groups > 1:
        s[max(p for p in range(n) if p % groups == 1)] = zero[1]
    elif n > 1:
        s[n - 1] = zero[1]
    if groups > 2:
        for j, p in enumerate(range(2, n, groups)):
            s[p] = zero[j % 2]
    return s


PLACEMENT_SIZES = (1, 15, 16, 17, 63, 64, 65, 257)      # one short of, at and one past a group (16) and a wave (64); several groups
