"""Operand sets for tests/test_gpu_devsim.py, with a big-integer model of the reduction steps of the asm statements
(tools/gen_gl_asm.py: mulmod_canonical, range4_stream) that says WHICH branch every tuple takes.

Under uniform operands the rare branches of the reductions never run (the borrow of LO - w3: ~2^-33 per product; TP >= p without a
carry: ~2^-32), so the sets interleave random tuples with operands CONSTRUCTED to take them, and `assert_coverage` checks -- on the
CPU, before anything is launched -- that every named branch is taken at every slot of every batch width, at least 64 times, and that
no 64 consecutive tuples (a wave) are uniform in any branch: the carries live in SGPR pairs as lane masks, a wave must mix lanes
that take a branch with lanes that do not.  tests/test_devsim_vectors.py runs these builders without a GPU."""
import random

P = 2**64 - 2**32 + 1
M64 = 2**64 - 1
EPS = 2**32 - 1

CANON = [0, 1, 2, 3, 4, P - 1, P - 2, 2**32 - 1, 2**32, 2**32 + 1, 2**63, P - 2**32, 0xFFFFFFFF00000000]
LOOSE = CANON + [P, P + 1, 2**64 - 1, 2**64 - 2**32, 2**64 - 2**32 + 1]
N_TUPLES = 1061        # not a multiple of 64, nine workgroups of 128 lanes


# ------------------------------------------------------------------------------------------------ the canonical multiplication
def mul_model(a, b):
    """the steps of mulmod_canonical on integers -> (result, borrow, carry, ge_p)"""
    v = a * b
    lo, w2, w3 = v & M64, (v >> 64) & EPS, v >> 96
    borrow = lo < w3
    t0 = (lo - w3) & M64
    if borrow:
        t0 = (t0 - EPS) & M64           # the wrapped value is 2^64 = eps too large
    tp = t0 + w2 * EPS
    carry = tp > M64
    tp &= M64
    ge_p = (not carry) and tp >= P
    r = (tp + EPS) & M64 if (carry or ge_p) else tp
    return r, borrow, carry, ge_p


def borrow_partner(b, lo):
    """a with (a * b) mod 2^64 = lo << tz(b): the low half of the product is tiny, the borrow of LO - w3 is taken whenever
    (a * b) >> 96 exceeds it"""
    assert b
    tz = (b & -b).bit_length() - 1
    return lo * pow(b >> tz, -1, 2**64) & M64


def ge_p_partner_small(b):
    """b < 2^32: a = ceil(p / b) puts the product in [p, p + b): no high words, TP = LO >= p"""
    return -(-P // b)


def ge_p_partner(b, max_steps=4096):
    """b < 2^40: the smallest k for which a multiple of b lies in the window [k 2^64 + p - k eps, (k + 1) 2^64 - k eps) of products
    whose reduction gives TP >= p without a carry; None if none within max_steps"""
    for k in range(1, max_steps):
        a = -(-(k * 2**64 + P - k * EPS) // b)
        if a <= M64 and mul_model(a, b)[3]:
            return a
    return None


def mul_pools(rng, count=160):
    """-> {"borrow": [(a, b)], "ge_p": [(a, b)]}: canonical pairs the model says take the branch"""
    borrow, ge = [], []
    mults = [pow(7, j, P) for j in range(1, 40)] + [rng.randrange(2**40, P) for _ in range(2 * count)]
    for b in mults:
        a = borrow_partner(b, rng.choice([1, 2, 3, 5]))
        if a < P and mul_model(a, b)[1]:
            borrow.append((a, b))
    for b in [7**i for i in range(1, 12)] + [rng.randrange(2, 2**32) for _ in range(count)]:
        a = ge_p_partner_small(b)
        if a < P and mul_model(a, b)[3]:
            ge.append((a, b))
    for b in [rng.randrange(2**32, 2**40) for _ in range(24)]:
        a = ge_p_partner(b)
        if a is not None and a < P:
            ge.append((a, b))
    return {"borrow": borrow[:count * 2], "ge_p": ge}


MUL_BRANCHES = ("borrow", "carry", "ge_p")


def mul_batch_vectors(width, n=N_TUPLES, seed=1):
    """n tuples of `width` products x[q] * t[q] -> (x, t, want, flags): flat lists of n * width values; flags[name][i * width + q].
    Slot q of tuple i is random, a borrow pair, a TP >= p pair or a pair from the edge alphabet by (i + q + i // 4) mod 4, so every
    kind visits every slot and consecutive lanes differ; constructed pairs go in both operand orders."""
    rng = random.Random(1000 * seed + width)
    pools = mul_pools(rng)
    x, t = [], []
    for i in range(n):
        for q in range(width):
            kind = (i + q + i // 4) % 4
            if kind == 1:
                a, b = rng.choice(pools["borrow"])
            elif kind == 2:
                a, b = rng.choice(pools["ge_p"])
            elif kind == 3:
                a, b = rng.choice(CANON), rng.choice(CANON + [rng.randrange(P)])
            else:
                a, b = rng.randrange(P), rng.randrange(P)
            if rng.random() < 0.5:
                a, b = b, a
            x.append(a)
            t.append(b)
    model = [mul_model(a, b) for a, b in zip(x, t)]
    want = [a * b % P for a, b in zip(x, t)]
    assert [m[0] for m in model] == want, "the big-integer model of mulmod_canonical disagrees with a * b mod p"
    flags = {"borrow": [m[1] for m in model], "carry": [m[2] for m in model], "ge_p": [m[3] for m in model]}
    return x, t, want, flags


# ------------------------------------------------------------------------------------------------ the range check of a two-bit limb
def loose_mul_model(a, b):
    """gen_poseidon_asm.mulmod (loose result) on integers -> (result, borrow, carry)"""
    v = a * b
    lo, w2, w3 = v & M64, (v >> 64) & EPS, v >> 96
    borrow = lo < w3
    t0 = (lo - w3) & M64
    if borrow:
        t0 = (t0 - EPS) & M64
    tp = t0 + w2 * EPS
    carry = tp > M64
    r = (tp + EPS) & M64 if carry else tp
    return r, borrow, carry


def range4_model(x):
    """range4_stream on integers -> (loose result, flags): "sub3_borrow" the borrow of x - 3, "add2_carry" the carry of y + 2,
    "mul1_borrow" the borrow inside the reduction of y = x (x - 3)"""
    sub3 = x < 3
    d = (x - 3) & M64
    if sub3:
        d = (d - EPS) & M64
    y, mul1_borrow, _ = loose_mul_model(x, d)
    add2 = y + 2 > M64
    y2 = (y + 2) & M64
    if add2:
        y2 = (y2 + EPS) & M64
    r, _, _ = loose_mul_model(y, y2)
    return r, {"sub3_borrow": sub3, "add2_carry": add2, "mul1_borrow": mul1_borrow}


def _sqrt_mod_p(a):
    """a square root of a mod p or None (Tonelli-Shanks; p - 1 = 2^32 (2^32 - 1))"""
    a %= P
    if a == 0:
        return 0
    if pow(a, (P - 1) // 2, P) != 1:
        return None
    q, s = 2**32 - 1, 32
    z = 7                               # a non-residue: the multiplicative generator
    m, c, t, r = s, pow(z, q, P), pow(a, q, P), pow(a, (q + 1) // 2, P)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2 = t2 * t2 % P
            i += 1
        b = pow(c, 1 << (m - i - 1), P)
        m, c, t, r = i, b * b % P, t * b * b % P, r * b % P
    return r


def add2_carry_candidates():
    """every canonical x whose y = x (x - 3) is congruent to 2^64 - 2 or 2^64 - 1, i.e. the only x for which the LOOSE y can be one
    of the two values whose y + 2 carries: the roots of x^2 - 3 x - c, c = eps - 2, eps - 1.  -> [(x, takes the carry)]"""
    out = []
    inv2 = pow(2, P - 2, P)
    for c in (EPS - 2, EPS - 1):
        s = _sqrt_mod_p(9 + 4 * c)
        if s is None:
            continue
        for root in {(3 + s) * inv2 % P, (3 - s) * inv2 % P}:
            assert root * (root - 3) % P == c
            out.append((root, range4_model(root)[1]["add2_carry"]))
    return out


def mul1_borrow_candidates(rng, count):
    """x with x (x - 3) = s (mod 2^64) for a small even s (Newton / Hensel from x = 0 or 1 mod 2; the derivative 2 x - 3 is odd): the
    low half of the first product is tiny, its reduction borrows"""
    out = []
    while len(out) < count:
        s, x = 2 * rng.randrange(1, 8), rng.randrange(2)
        for _ in range(7):
            x = (x - (x * x - 3 * x - s) * pow(2 * x - 3, -1, 2**64)) & M64
        assert (x * (x - 3) - s) & M64 == 0
        if 3 <= x < P and range4_model(x)[1]["mul1_borrow"]:
            out.append(x)
    return out


RANGE_BRANCHES = ("sub3_borrow", "mul1_borrow", "add2_carry")


def range4_vectors(width, n=N_TUPLES, seed=2):
    """n tuples of `width` canonical limbs -> (x, want mod p, flags).  Slot kinds by (i + q + i // 5) mod 5: random, {0, 1, 2} (the
    borrow of x - 3), constructed for the borrow of the first reduction, the alphabet (3, 4, p - 1, p - 2 included), the limbs that
    take the carry of y + 2."""
    rng = random.Random(1000 * seed + width)
    hard = mul1_borrow_candidates(rng, 64)
    carry = [x for x, takes in add2_carry_candidates() if takes]
    x = []
    for i in range(n):
        for q in range(width):
            kind = (i + q + i // 5) % 5
            x.append(rng.randrange(P) if kind == 0 else rng.randrange(3) if kind == 1 else rng.choice(hard) if kind == 2
                     else rng.choice(CANON) if kind == 3 or not carry else rng.choice(carry))
    model = [range4_model(v) for v in x]
    want = [v * (v - 1) * (v - 2) * (v - 3) % P for v in x]
    assert [m[0] % P for m in model] == want, "the big-integer model of range4_stream disagrees with the product"
    flags = {k: [m[1][k] for m in model] for k in ("sub3_borrow", "add2_carry", "mul1_borrow")}
    return x, want, flags


# ------------------------------------------------------------------------------------------------ coverage
def assert_coverage(flags, n, width, names, min_total=64, min_per_slot=8):
    for name in names:
        f = flags[name]
        assert len(f) == n * width
        assert sum(f) >= min_total, (name, sum(f))
        for q in range(width):
            col = f[q::width]
            assert min_per_slot <= sum(col) <= n - min_per_slot, (name, width, q, sum(col))
            run = 1
            for k in range(1, n):
                run = run + 1 if col[k] == col[k - 1] else 1
                assert run < 64, "64 consecutive tuples uniform in %s at slot %d of width %d (tuple %d)" % (name, q, width, k)


# ------------------------------------------------------------------------------------------------ butterfly groups
def ntt_group_ref(g, dit, inverse, x, t):
    """gl_ntt_group_plain with J = 0 (inner twiddles only) composed with the per-element table multiplication -> (values, products):
    products = the (value, table entry) pairs that go through gl_mul_batch"""
    M = 1 << g
    w = pow(7, (P - 1) >> g, P)
    if inverse:
        w = pow(w, P - 2, P)
    x = list(x)
    prods = []
    if dit:
        prods = [(x[m], t[m - 1]) for m in range(1, M)]
        for m in range(1, M):
            x[m] = x[m] * t[m - 1] % P
    for uu in range(g):
        u = g - 1 - uu if dit else uu
        bit = g - 1 - u
        for m in range(M):
            if m & (1 << bit):
                continue
            tw = pow(w, (m & ((1 << bit) - 1)) << u, P)
            a, b = x[m], x[m | (1 << bit)]
            if dit:
                b = b * tw % P
                x[m], x[m | (1 << bit)] = (a + b) % P, (a - b) % P
            else:
                x[m], x[m | (1 << bit)] = (a + b) % P, (a - b) * tw % P
    if not dit:
        prods = [(x[m], t[m - 1]) for m in range(1, M)]
        for m in range(1, M):
            x[m] = x[m] * t[m - 1] % P
    return x, prods


def ntt_group_vectors(g, dit, inverse, zp=0, n=389, seed=3):
    """n groups -> (x, t, want, flags of the table multiplications).  Inputs from the alphabet and random; the table entry of slot m
    is, by (i + m) mod 3, random, from the alphabet, or the borrow partner of the value it multiplies (the group's own butterfly
    output for a DIF group)."""
    rng = random.Random(seed * 7919 + g * 16 + dit * 4 + inverse * 2 + zp)
    M = 1 << g
    xs, ts, want, flags = [], [], [], {k: [] for k in MUL_BRANCHES}
    for i in range(n):
        x = [rng.choice(CANON) if rng.random() < 0.3 else rng.randrange(P) for _ in range(M)]
        for m in range(M >> zp if zp else M, M):
            x[m] = 0
        t = [rng.choice(CANON) if (i + m) % 3 == 1 else rng.randrange(P) for m in range(1, M)]
        vals = x if dit else ntt_group_ref(g, dit, inverse, x, [1] * (M - 1))[0]
        for m in range(1, M):
            if (i + m) % 3 == 2 and vals[m]:
                cand = borrow_partner(vals[m], rng.choice([1, 2, 3, 5]))
                if cand < P:
                    t[m - 1] = cand
        out, prods = ntt_group_ref(g, dit, inverse, x, t)
        for a, b in prods:
            r = mul_model(a, b)
            for k, name in enumerate(MUL_BRANCHES):
                flags[name].append(r[k + 1])
        xs += x
        ts += t
        want += out
    return xs, ts, want, flags


# ------------------------------------------------------------------------------------------------ Poseidon states
def poseidon_states(n, seed=4, loose=True):
    """n states of twelve words: every alphabet value at every position, all-equal edge states, random"""
    rng = random.Random(seed)
    alpha = LOOSE if loose else CANON
    top = 2**64 if loose else P
    out = []
    for i in range(n):
        if i < len(alpha):
            s = [alpha[i]] * 12
        elif i % 3 == 0:
            s = [rng.randrange(top) for _ in range(12)]
        elif i % 3 == 1:
            s = [rng.choice(alpha) for _ in range(12)]
        else:
            s = [rng.randrange(top) for _ in range(12)]
            s[i % 12] = alpha[(i // 12) % len(alpha)]
        out.append(s)
    return out
