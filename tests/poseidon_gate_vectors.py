"""Wire rows of the Poseidon gate shared by tests/test_poseidon_gate_host.py and tests/test_gpu_poseidon_gate_stmt.py."""
import random

import numpy as np

from oracle import goldilocks as gl

P = gl.P
EDGE = [0, 1, P - 1, 2**32 - 1, 2**32, P - 2**32]
NW = 135
# two pairs of challenges: random, and the two whose limbs are the extremes of the alpha-power table
ALPHA_SEED = 78


def alphas():
    rng = random.Random(ALPHA_SEED)
    return [[rng.randrange(P), rng.randrange(P)], [P - 1, 2**32]]


def rows(extra=0):
    """-> [(expect, wires)]: 96 random / edge-alphabet rows (the swap wire 0 and 1 in half of them), 24 satisfying rows from the
    library's witness generator and the same 24 with one partial-round S-box wire off by one (positions 0..21, then 0 and 21
    again), then `extra` more random rows.  expect: 0 none, 1 every constraint zero, 2 some constraint non-zero"""
    from zklc_amd.plonky2.prover import poseidon_gate_rows
    rng = random.Random(77)
    out = []
    for i in range(96):
        r = [rng.randrange(P) for _ in range(NW)] if i % 3 else [rng.choice(EDGE) for _ in range(NW)]
        if i % 2:
            r[24] = (i // 2) % 2
        out.append((0, r))
    ins = np.array([[rng.randrange(P) for _ in range(12)] for _ in range(24)], dtype=np.uint64)
    sat = [[int(v) for v in r] for r in poseidon_gate_rows(ins, np.array([k % 2 for k in range(24)], dtype=np.uint64))]
    for r in sat:
        out.append((1, r))
    for k, r in enumerate(sat):
        pos = 65 + (k if k < 22 else 21 * (k - 22))
        broken = list(r)
        broken[pos] = (broken[pos] + 1) % P
        out.append((2, broken))
    for _ in range(extra):
        out.append((0, [rng.randrange(P) for _ in range(NW)]))
    return out
