"""Shared by tests/test_gpu_groth16_sizes.py and the compute_h tests of tests/test_gpu_bn254.py (not a test module): the two
constraint systems at the domain sizes where the prover's production kernels run, their key SCALARS (oracle.groth16.key_scalars),
witnesses, and the conversions between Python integers and the 4 x u64 words of the C ABI that stay affordable at 2^15 elements.
Everything here is CPU work on the oracle alone; nothing of the code under test is imported."""
import concurrent.futures as cf
import ctypes
import functools
import random

import numpy as np

from oracle import bn254 as B, groth16 as G

R = G.R
TOXIC = (0x1234567891, 0xabcdef12345, 0x777766665555, 0x3133731337, 0x42424242)
N_PUBLIC = 3
# domain 2^12: 4000 constraints (live padding); 2^13: exactly 2^13 (no padding); 2^14 (compute_h only); 2^15
N_CONSTRAINTS = {12: 4000, 13: 1 << 13, 14: (1 << 14) - 3, 15: 1 << 15}
_TWO256 = 1 << 256


def words_from_ints(vals):
    """integers below 2^256 -> uint64 [n, 4] little-endian words (regular form)"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def mont_words_from_ints(vals):
    """field elements -> uint64 [n, 4] in gnark-crypto's layout (x 2^256 mod r)"""
    return words_from_ints([v % R * _TWO256 % R for v in vals])


def ints_from_words(arr):
    b = np.ascontiguousarray(arr, dtype=np.uint64).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


_RINV = pow(_TWO256, R - 2, R)


def ints_from_mont_words(arr):
    return [v * _RINV % R for v in ints_from_words(arr)]


@functools.lru_cache(maxsize=None)
def system(kind, log_n):
    """kind 'chain' (oracle.groth16.square_chain_r1cs: uniform wires) or 'bits' (bit_recomposition_r1cs: mostly bits) at domain
    2^log_n -> dict: r1cs, n_public, publics, witness (satisfying), abc (A w, B w, C w padded to the domain), layout (bits only)"""
    n_con = N_CONSTRAINTS[log_n]
    publics = [pow(7, 1000 + 10 * log_n + i, R) for i in range(N_PUBLIC)]
    if kind == "chain":
        r1cs, wit = G.square_chain_r1cs(n_con, n_public=N_PUBLIC)
        w, layout = wit(publics, 0x5eed + log_n), None
    else:
        r1cs, wit, layout = G.bit_recomposition_r1cs(n_con, n_public=N_PUBLIC)
        w = wit(publics, 0x5eed + log_n, seed=log_n)
    n = G.domain_size(n_con)
    assert n == 1 << log_n
    abc = G.abc_evaluations(r1cs, w, n)
    assert all(x * y % R == z for x, y, z in zip(*abc)), "the witness satisfies the system"
    return {"kind": kind, "log_n": log_n, "n": n, "r1cs": r1cs, "n_public": N_PUBLIC, "publics": publics, "witness": w, "abc": abc,
            "layout": layout}


def unsatisfied(r1cs, witness, n):
    """(index of the first violated constraint, how many are violated) in Python integers"""
    a, b, c = G.abc_evaluations(r1cs, witness, n)
    bad = [j for j, (x, y, z) in enumerate(zip(a, b, c)) if x * y % R != z]
    return (bad[0] if bad else None), len(bad)


def sample_indices(scalars, count=32, seed=0):
    """a fixed sample of a key array: the first and the last point, EVERY zero scalar (a point at infinity), and random ones up to
    at least `count` non-zero scalars"""
    n = len(scalars)
    zeros = [i for i, s in enumerate(scalars) if s % R == 0]
    rng = random.Random(seed * 1000003 + n)
    picks = {0, n - 1} | {rng.randrange(n) for _ in range(count)}
    while len(picks - set(zeros)) < min(count, n - len(zeros)):
        picks.add(rng.randrange(n))
    return sorted(picks | set(zeros))


def _g1_words(s):
    p = B.mul(s % R, B.G1)
    return B.to_mont_words(p[0]) + B.to_mont_words(p[1])


def _g2_words(s):
    return B.g2_to_words(B.g2_mul(s % R, B.G2))


def expected_point_words(jobs):
    """jobs: [(group 1 | 2, scalar)] -> the words of scalar * generator by the oracle's B.mul / B.g2_mul (a zero scalar is the
    all-zero record); ~70 ms of Python integers per point, so the non-zero ones are spread over a few workers"""
    out = [None] * len(jobs)
    todo = []
    for i, (group, s) in enumerate(jobs):
        if s % R == 0:
            out[i] = [0] * (8 * group)
        else:
            todo.append(i)
    if todo:
        with cf.ProcessPoolExecutor(max_workers=8) as ex:
            g1 = [i for i in todo if jobs[i][0] == 1]
            g2 = [i for i in todo if jobs[i][0] == 2]
            for idx, res in ((g1, ex.map(_g1_words, [jobs[i][1] for i in g1], chunksize=8)),
                             (g2, ex.map(_g2_words, [jobs[i][1] for i in g2], chunksize=8))):
                for i, wds in zip(idx, res):
                    out[i] = wds
    return out


def msm_plan(hostsim, n, g1):
    """the library's plan of an n-point sum through tests/hostsim (g1: a G1 sum, where the endomorphism split may be on)"""
    out = (ctypes.c_uint32 * 9)()
    hostsim.hostsim_msm_plan_group(ctypes.c_uint64(n), 1 if g1 else 0, out)
    return dict(zip(("n_pad", "c", "windows", "buckets_per_window", "total_buckets", "chunks", "chunk_len", "seg", "glv"), list(out)))


def fr_ntt_plan(hostsim, log_n):
    """(t1, t2, two_pass) of a natural-order Fr transform of 2^log_n points"""
    out = (ctypes.c_uint32 * 3)()
    hostsim.hostsim_fr_ntt_plan(log_n, out)
    return out[0], out[1], bool(out[2])
