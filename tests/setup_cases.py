"""Shared by tests/test_setup_host.py, tests/test_setup_host_sanitized.py and tests/test_gpu_groth16_setup.py (not a test module): the
constraint systems and toxic sets of the scalar stage of groth16.Setup, each with `oracle.groth16.key_scalars` as the expected
output.  Everything here is CPU work on the oracle alone; nothing of the code under test is imported.

A system is kept as three lists of rows of (wire, coefficient) PAIRS, so that a row can hold the same wire twice and a zero
coefficient (the hand-made system); the oracle reads the rows as dictionaries with the duplicates added up."""
import functools

import numpy as np

import groth16_size_cases as S
from oracle import bn254_fr as FR, groth16 as G

R = G.R
BIN_LIMITS = (4, 64)            # columns of at most 4 terms: one lane; of at most 64: eight lanes; longer ones: a wave or segments


def _pairs(r1cs):
    return tuple([[(w, c) for w, c in row.items()] for row in M] for M in r1cs)


def _hand_made():
    """5 constraints over 7 wires (n_public = 1): wire 4 occurs in no matrix (a_t = b_t = k = 0); row 1 of A has wire 3 twice
    (coefficients 1 and 5), row 4 of B has wire 1 twice with coefficients that cancel (9 and r - 9: b_t[1] = 0 from two general
    terms); row 3 of A carries a zero coefficient.  Not meant to be satisfiable: the scalar stage never sees a witness."""
    A = [[(2, 1)], [(3, 1), (3, 5)], [(5, R - 1), (0, 7)], [(6, 2), (2, 0)], [(1, 1)]]
    B = [[(2, 1)], [(0, 1)], [(5, 3)], [(6, 1)], [(1, 9), (1, R - 9)]]
    C = [[(3, 1)], [(5, 1)], [(6, 1), (0, R - 3)], [(2, 4)], [(0, 1)]]
    return A, B, C


SYSTEMS = {
    "chain1": lambda: (_pairs(G.square_chain_r1cs(1)[0]), 2),
    "chain3": lambda: (_pairs(G.square_chain_r1cs(3)[0]), 2),
    "chain100": lambda: (_pairs(G.square_chain_r1cs(100, n_public=3)[0]), 3),
    "chain4000": lambda: (_pairs(G.square_chain_r1cs(4000, n_public=3)[0]), 3),
    "bits8192": lambda: (_pairs(G.bit_recomposition_r1cs(1 << 13, n_public=3)[0]), 3),
    "hand5": lambda: (_hand_made(), 1),
}
SYSTEM_NAMES = tuple(SYSTEMS)
TOXIC_NAMES = ("base", "above_r", "tau_zero", "tau_in_domain", "alpha_beta_zero")
CASES = [(s, t) for s in SYSTEM_NAMES for t in TOXIC_NAMES]
CASE_IDS = ["%s-%s" % c for c in CASES]


@functools.lru_cache(maxsize=None)
def system(name):
    """-> dict: rows (A, B, C as pair rows), oracle_rows (dictionaries, duplicates added), n_public, n_constraints, n_wires, n
    (domain size), log_n, and the CSR arrays of zklc_r1cs_create"""
    rows, n_public = SYSTEMS[name]()
    oracle_rows = []
    for M in rows:
        out = []
        for row in M:
            d = {}
            for w, c in row:
                d[w] = (d.get(w, 0) + c) % R
            out.append(d)
        oracle_rows.append(out)
    n_con = len(rows[0])
    n_wires = 1 + max(max((max(w for w, _ in row) if row else 0) for M in rows for row in M), n_public)
    n = G.domain_size(n_con)
    ids, row_ptr, wires, cids = {}, [0], [], []
    for M in rows:
        for row in M:
            for w, c in row:
                wires.append(w)
                cids.append(ids.setdefault(c % R, len(ids)))
            row_ptr.append(len(wires))
    return {"name": name, "rows": rows, "oracle_rows": tuple(oracle_rows), "n_public": n_public, "n_constraints": n_con,
            "n_wires": n_wires, "n": n, "log_n": n.bit_length() - 1,
            "csr": (np.array(row_ptr, dtype=np.uint64), np.array(wires, dtype=np.uint32), np.array(cids, dtype=np.uint32),
                    S.mont_words_from_ints(list(ids)))}


def toxic(name, n):
    """(tau, alpha, beta, gamma, delta) of a toxic set for a domain of n points"""
    tau, alpha, beta, gamma, delta = S.TOXIC
    if name == "base":
        return S.TOXIC
    if name == "above_r":                       # every value at or above r (beta = r itself: 0); reduced by the library
        return (R + 5, (1 << 256) - 1, R, R + 7, 2 * R + 3)
    if name == "tau_zero":
        return (0, alpha, beta, gamma, delta)
    if name == "tau_in_domain":                 # L is the indicator of j = 3 mod n, z is all zero
        return (pow(FR.root(n.bit_length() - 1), 3, R), alpha, beta, gamma, delta)
    if name == "alpha_beta_zero":
        return (tau, 0, 0, gamma, delta)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def expected(system_name, toxic_name):
    """the oracle's scalars as integer lists: a_t, b_t, k (the vk part, then the pk part: the library's one array), z; and c_t"""
    sy = system(system_name)
    sc = G.key_scalars(sy["oracle_rows"], sy["n_public"], toxic(toxic_name, sy["n"]))
    assert sc["n"] == sy["n"] and sc["n_wires"] == sy["n_wires"]
    return {"a_t": sc["a_t"], "b_t": sc["b_t"], "c_t": sc["c_t"], "k": sc["k_vk"] + sc["k_pk"], "z": sc["z"], "scalars": sc}


def expected_words(system_name, toxic_name):
    """-> (a_t, b_t, k, z) as uint64 [., 4] arrays, regular form"""
    e = expected(system_name, toxic_name)
    return tuple(S.words_from_ints(e[k]) for k in ("a_t", "b_t", "k", "z"))


def column_lengths(system_name):
    """{(matrix, wire): number of terms} of the columns that have any (duplicates and zero coefficients are terms)"""
    out = {}
    for m, M in enumerate(system(system_name)["rows"]):
        for row in M:
            for w, _ in row:
                out[(m, w)] = out.get((m, w), 0) + 1
    return out


def expected_plan(system_name, seg_terms):
    """columns by 1 / 8 / 64 lanes, columns cut into segments, segments -- over all 3 n_wires columns, the empty ones included"""
    sy = system(system_name)
    lens = list(column_lengths(system_name).values())
    lens += [0] * (3 * sy["n_wires"] - len(lens))
    bins = [0, 0, 0, 0, 0]
    for v in lens:
        b = 0 if v <= BIN_LIMITS[0] else 1 if v <= BIN_LIMITS[1] else 2 if v <= seg_terms else 3
        bins[b] += 1
        if b == 3:
            bins[4] += -(-v // seg_terms)
    return dict(zip(("cols_1_lane", "cols_8_lanes", "cols_64_lanes", "cols_segmented", "segments"), bins))
