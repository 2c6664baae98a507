"""Shared by tests/test_groth16_verifier_host.py and tests/test_gpu_groth16_verifier.py (not a test module): the verifying keys and
proofs of tests/golden/groth16_batch.json and groth16_kat.json, proof mutations, and an INDEPENDENT classification of a proof
built from oracle.bn254 and oracle.groth16.verify only -- reduced coordinates, then infinity, then the curve equations (A, C, B),
then [r - 1] B + B == O, then the oracle's verify.  Expected statuses always come from here, never from the code under test."""
import concurrent.futures as cf
import random

from conftest import load_golden
from oracle import bn254 as B, groth16 as G
from zklc_amd import formats as F

P, R = B.P, B.R
OK, BAD_ENCODING, INFINITY, NOT_ON_CURVE, NOT_IN_SUBGROUP, PAIRING = range(6)


def _g1(p):
    return (int(p[0]), int(p[1]))


def _g2(p):
    return ((int(p[0][0]), int(p[0][1])), (int(p[1][0]), int(p[1][1])))


def fixture_keys():
    """-> list of (vk, [(proof8, public_inputs)] x 3) for n_public = 3 and 40"""
    out = []
    for key in load_golden("groth16_batch.json")["keys"]:
        vk = key["vk"]
        vkd = {"alpha1": _g1(vk["alpha1"]), "beta2": _g2(vk["beta2"]), "gamma2": _g2(vk["gamma2"]), "delta2": _g2(vk["delta2"]),
               "K": [_g1(p) for p in vk["K"]]}
        assert len(vkd["K"]) == key["n_public"] + 1
        out.append((vkd, [([int(x) for x in p["proof"]], [int(x) for x in p["public_inputs"]]) for p in key["proofs"]]))
    return out


def kat():
    """the reference's known-answer vector: (vk, proof8, inputs, incorrect_inputs, incorrect_proof)"""
    j = load_golden("groth16_kat.json")
    v = {k: int(x) for k, x in j["vk"].items()}
    g2n = lambda n: B.g2_neg(((v[n + "_NEG_X_0"], v[n + "_NEG_X_1"]), (v[n + "_NEG_Y_0"], v[n + "_NEG_Y_1"])))
    vk = {"alpha1": (v["ALPHA_X"], v["ALPHA_Y"]), "beta2": g2n("BETA"), "gamma2": g2n("GAMMA"), "delta2": g2n("DELTA"),
          "K": [(v["CONSTANT_X"], v["CONSTANT_Y"])] + [(v["PUB_%d_X" % i], v["PUB_%d_Y" % i]) for i in range(4)]}
    ints = lambda xs: [int(x) for x in xs]
    return vk, ints(j["proof"]), ints(j["inputs"]), ints(j["incorrect_inputs"]), ints(j["incorrect_proof"])


def points(proof8):
    p = [int(x) for x in proof8]
    return (p[0], p[1]), ((p[3], p[2]), (p[5], p[4])), (p[6], p[7])


def classify(vk, proof8, public_inputs):
    a, b, c = points(proof8)
    if any(int(x) >= P for x in proof8):
        return BAD_ENCODING
    if a == (0, 0) or c == (0, 0) or b == ((0, 0), (0, 0)):
        return INFINITY
    if not B.is_on_curve(a) or not B.is_on_curve(c) or not B.g2_is_on_curve(b):
        return NOT_ON_CURVE
    if B.g2_add(B.g2_mul(R - 1, b), b) is not None:
        return NOT_IN_SUBGROUP
    return OK if G.verify(vk, (a, b, c), [int(x) % R for x in public_inputs]) else PAIRING


def _classify_job(job):
    return classify(*job)


_MEMO = {}


def classify_many(vk, cases):
    """cases: [(proof8, public_inputs)] -> statuses; the oracle's pairing is seconds of Python per proof, so the cases are spread
    over a few worker processes and remembered for the session"""
    kid = repr(sorted(vk.items()))
    keys = [(kid, tuple(int(x) for x in p), tuple(int(x) for x in xs)) for p, xs in cases]
    todo = sorted({k for k in keys if k not in _MEMO})
    if todo:
        jobs = [(vk, list(k[1]), list(k[2])) for k in todo]
        if len(jobs) > 2:
            with cf.ProcessPoolExecutor(max_workers=8) as ex:
                res = list(ex.map(_classify_job, jobs))
        else:
            res = [_classify_job(j) for j in jobs]
        _MEMO.update(zip(todo, res))
    return [_MEMO[k] for k in keys]


def rerandomise(proof8, t):
    """(A, B, C) -> ([t] A, [t^-1 mod r] B, C): another valid proof of the same statement"""
    a, b, c = points(proof8)
    return G.proof_to_uint256x8((B.mul(t % R, a), B.g2_mul(pow(t, R - 2, R), b), c))


def twist_point_outside_g2():
    from test_gpu_groth16 import _twist_point_outside_g2
    return _twist_point_outside_g2()


def set_b(proof8, pt):
    p = list(proof8)
    (x0, x1), (y0, y1) = pt
    p[2], p[3], p[4], p[5] = x1, x0, y1, y0
    return p


def mutate(proof8, kind, rng):
    """one defect: 'p' a coordinate >= p, 'zero' a point zeroed, 'curve' a point moved off its curve by y + 1, 'subgroup' B replaced
    by a twist point outside G2, 'two_g1' A replaced by [2] G1, 'none' unchanged"""
    p = list(proof8)
    if kind == "p":
        p[rng.randrange(8)] = P + rng.choice([0, 0, 1, 12345])
    elif kind == "zero":
        lo, hi = rng.choice([(0, 2), (2, 6), (6, 8)])
        for i in range(lo, hi):
            p[i] = 0
    elif kind == "curve":
        i = rng.choice([1, 7, 5])          # A.y, C.y, B.y0
        p[i] = (p[i] + 1) % P
    elif kind == "subgroup":
        p = set_b(p, twist_point_outside_g2())
    elif kind == "two_g1":
        p[0], p[1] = B.mul(2, B.G1)
    else:
        assert kind == "none"
    return p


MUTATIONS = ["p", "p", "zero", "zero", "curve", "curve", "subgroup", "subgroup", "two_g1", "none"]


def sweep(keys, n, seed):
    """n mutated proofs over the keys: [(key index, proof8, public_inputs)]"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        k = i % len(keys)
        proof, pubs = keys[k][1][rng.randrange(len(keys[k][1]))]
        out.append((k, mutate(proof, rng.choice(MUTATIONS), rng), pubs))
    return out
