"""Shared by tests/test_gnark_points_host.py and tests/test_gpu_gnark_points.py (not a test module): byte arrays of points in
gnark-crypto's own encoding (zklc_amd/gnark_keys.py), raw and compressed, G1 and G2, valid and defective slots interleaved so that
neighbouring lanes take different branches, with the expected class and words of every slot.

The expectation of a slot comes from the point-by-point Python reader (`read_g1` / `read_g2` on that slot alone, `points_to_words`
on its result, its ProofInvalid message mapped to a class) -- never from the code under test -- with two exceptions: a flag that
belongs to the other encoding is BAD_ENCODING by rule, and the membership class is known by construction (a sample is confirmed
with the oracle's [r] Q in the CPU test)."""
import functools
import random

import numpy as np

from oracle import bn254 as B
from zklc_amd import gnark_keys as K
from zklc_amd.formats import ProofInvalid

P = B.P
OK, INFINITY, BAD_ENCODING, NOT_ON_CURVE, NOT_IN_SUBGROUP = range(5)
WORKGROUP = K.DECODE_WORKGROUP
ALL_ONES = (1 << 64) - 1


def twist_point_outside_g2():
    from groth16_cases import twist_point_outside_g2 as f
    return f()


def _be(v):
    return int(v).to_bytes(32, "big")


def _flagged(b, flag):
    b = bytearray(b)
    b[0] = (b[0] & 0x3F) | (flag << 6)
    return bytes(b)


def real_rhs_twist_points():
    """twist points x = x0 + x1 u whose x^3 + b' is REAL: x0^2 = (x1^3 - b'_1) / (3 x1) when that is a square.  Their y is (y0, 0)
    or (0, y1): the only inputs that reach the a1 == 0 branch of the Fp2 square root and the A1 == 0 fallback of the ordering.
    On the twist, not in G2.  -> [(point, "y0" | "y1")]"""
    b0, b1 = K._twist_b()
    out = []
    for x1 in range(1, 12):
        t = (x1 ** 3 - b1) * pow(3 * x1, P - 2, P) % P
        x0 = pow(t, (P + 1) // 4, P)
        if x0 * x0 % P != t:
            continue
        x = (x0, x1)
        rhs = K._fp2_mul(K._fp2_mul(x, x), x)
        rhs = ((rhs[0] + b0) % P, (rhs[1] + b1) % P)
        assert rhs[1] == 0
        y = K._fp2_sqrt(rhs)
        assert K._fp2_mul(y, y) == rhs and (y[0] == 0) != (y[1] == 0)
        out.append(((x, y), "y0" if y[1] == 0 else "y1"))
    assert {k for _, k in out} == {"y0", "y1"}
    return out


def _class_of(msg):
    if "not reduced" in msg or "infinity flag with a non-zero coordinate" in msg:
        return BAD_ENCODING
    if "not on the" in msg:                 # "... not on the curve", "... not on the twist curve", compressed: "x is not on the ..."
        return NOT_ON_CURVE
    raise AssertionError("unmapped reader message: " + msg)


def _from_reader(slot, g2):
    """(class, words) of one slot by the Python reader"""
    width = 16 if g2 else 8
    try:
        pt = (K.read_g2 if g2 else K.read_g1)(K._Reader(slot))
    except ProofInvalid as e:
        return _class_of(str(e)), np.zeros(width, dtype=np.uint64)
    if pt is None:
        return INFINITY, np.zeros(width, dtype=np.uint64)
    return OK, K.points_to_words([pt], g2=g2)[0]


@functools.lru_cache(maxsize=None)
def cases(g2, compressed):
    """-> list of (slot bytes, class, class with the subgroup flag, words with the flag, words without it (uint64 [8 | 16]), tag)"""
    raw = not compressed
    stride = (128 if g2 else 64) >> (0 if raw else 1)
    coords = 4 if g2 else 2
    write = K.write_g2 if g2 else K.write_g1
    neg = B.g2_neg if g2 else B.neg
    out = []

    def by_reader(slot, tag, outside=False):
        assert len(slot) == stride
        cls, words = _from_reader(slot, g2)
        sub = NOT_IN_SUBGROUP if (outside and cls == OK) else cls
        out.append((slot, cls, sub, words if sub == cls else np.zeros_like(words), words, tag))

    def by_rule(slot, tag):
        assert len(slot) == stride
        z = np.zeros(16 if g2 else 8, dtype=np.uint64)
        out.append((slot, BAD_ENCODING, BAD_ENCODING, z, z, tag))

    gen = B.G2 if g2 else B.G1
    mulf = B.g2_mul if g2 else B.mul
    good = [mulf(k, gen) for k in (1, 2, 3, 5, 7, 11, 12345, B.R - 1)]
    for pt in good:
        by_reader(write(pt, raw), "multiple")
        by_reader(write(neg(pt), raw), "multiple, -y")
    # infinity in every form the reader accepts
    by_reader(write(None, raw), "infinity")
    if raw:
        by_reader(bytes([0x40]) + bytes(31) + bytes(range(1, stride - 31)), "infinity, padding not zero")
        by_reader(bytes(stride), "uncompressed (0, 0)")
    # coordinates >= p
    first = write(good[1], raw)
    by_reader(_flagged(_be(P), first[0] >> 6) + first[32:], "x = p")
    if g2:
        by_reader(first[:32] + _be(P + 5) + first[64:], "x.a0 = p + 5")
    if raw:
        by_reader(first[:stride - 32] + _be(P + 1), "y = p + 1")
        by_reader(first[:32 * (coords // 2)] + _be(P) + first[32 * (coords // 2) + 32:], "first y coordinate = p")
    # a flag of the other encoding
    if raw:
        by_rule(_flagged(first, 2), "raw array, flag 0b10")
        by_rule(_flagged(first, 3), "raw array, flag 0b11")
    else:
        by_rule(_flagged(first, 0), "compressed array, flag 0b00")
    # the infinity flag with a payload
    by_reader(_flagged(first, 1), "infinity flag, non-zero payload")
    if g2:
        by_reader(bytes([0x40]) + bytes(31) + first[32:], "infinity flag, non-zero x.a0")
    if raw:
        for pt in good[:3]:
            b = bytearray(write(pt, True))
            y = (int.from_bytes(b[-32:], "big") + 1) % P
            by_reader(bytes(b[:-32]) + _be(y), "y + 1")
    # an x with no y
    for x in ([(1, 1), (7, 1), (9, 1)] if g2 else [4, 10, 12]):
        if g2:
            xb = _be(x[1]) + _be(x[0])
            slot = xb + _be(1) + _be(2) if raw else _flagged(xb, 2)
        else:
            slot = _be(x) + _be(1) if raw else _flagged(_be(x), 3)
        by_reader(slot, "x without y")
        assert out[-1][1] == NOT_ON_CURVE
    if g2:
        q = twist_point_outside_g2()
        for pt in (q, B.g2_add(q, q), B.g2_add(B.g2_add(q, q), q)):
            by_reader(write(pt, raw), "twist point outside G2", outside=True)
            assert out[-1][1] == OK
        for pt, kind in real_rhs_twist_points():
            for p2 in (pt, B.g2_neg(pt)):
                by_reader(write(p2, raw), "real right-hand side, " + kind, outside=True)
                assert out[-1][1] == OK and K.read_g2(K._Reader(write(p2, raw))) == p2
    random.Random(20 + 2 * g2 + compressed).shuffle(out)
    # keep neighbours different where the shuffle left two slots of one class side by side
    for i in range(1, len(out) - 1):
        if out[i][1] == out[i - 1][1]:
            for j in range(i + 1, len(out)):
                if out[j][1] != out[i - 1][1]:
                    out[i], out[j] = out[j], out[i]
                    break
    return out


def array(g2, compressed, n, check_subgroup=False, only=None, start=0):
    """n slots cycling through the cases from `start` (only: keep the cases whose class is in this set)
    -> (bytes, status uint32 [n], words uint64 [n, w], summary [OK, infinity, rejected, first rejected index | None])"""
    cs = cases(g2, compressed)
    if only is not None:
        cs = [c for c in cs if (c[2] if check_subgroup else c[1]) in only]
        assert cs
    pick = [cs[(start + i) % len(cs)] for i in range(n)]
    status = np.array([c[2] if check_subgroup else c[1] for c in pick], dtype=np.uint32)
    words = np.stack([c[3] if check_subgroup else c[4] for c in pick]) if n else np.zeros((0, 16 if g2 else 8), dtype=np.uint64)
    rej = np.nonzero(status >= BAD_ENCODING)[0]
    summary = [int((status == OK).sum()), int((status == INFINITY).sum()), int(len(rej)), int(rej[0]) if len(rej) else None]
    return b"".join(c[0] for c in pick), status, words, summary
