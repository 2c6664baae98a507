"""Shared by tests/test_gpu_bn254.py (the kernels) and tests/test_hostsim_fr_ntt.py (their host twin; not a test module): inputs
of the Fr NTT whose outputs have a closed form, so that a transform of any size is checked against the DEFINITION in
oracle/bn254_fr.py with a few hundred `pow` calls instead of a Python transform of that size.
  constant c:   forward = n c at 0 and exact zero elsewhere; inverse (with or without the coset) = c at 0 and zero elsewhere
                (whole array); forward on the coset = the geometric sum c (5^n - 1) / (5 w^k - 1)
  eight terms:  X[k] = sum_i c_i (g w^k)^(j_i), g = 5 on the coset; inverse x[i] = g^-i / n sum_i c_i w^(-i j_i)"""
import numpy as np

import groth16_size_cases as S

MODES = ((0, 0), (0, 1), (1, 0), (1, 1))          # (inverse, coset)


def sample_indices(log_n, t1, seed):
    """at least 256 output indices: the edges of k = k1 + N1 k2 (N1 = 2^t1), of the two-level tables (2048) and of the array, the
    index with the largest j2 k1 (k1 = N1 - 1 against j2 = N2 - 1), and random ones"""
    import random
    n, n1 = 1 << log_n, 1 << t1
    k_star = (n1 - 1) + n1 * ((n >> t1) - 1)                 # k1 = N1 - 1 (and the largest k2)
    fixed = [0, 1, n1 - 1, n1, n1 + 1, 2047, 2048, 2049, n // 2, n - 1, k_star]
    rng = random.Random(seed)
    idx = {k for k in fixed if 0 <= k < n}
    while len(idx) < 256 + len(fixed):
        idx.add(rng.randrange(n))
    return sorted(idx)


def transform_of_sparse(log_n, terms, inverse, coset, ks):
    """the transform of sum_i c_i X^(j_i) at the output indices ks, from the definition in oracle/bn254_fr.py:
    forward X[k] = sum_j x_j (g w^k)^j with g = 5 on the coset and 1 otherwise; inverse x[i] = g^-i / n sum_k X_k w^(-i k)"""
    from oracle import bn254_fr as FR
    Rr, n = FR.R, 1 << log_n
    w = FR.root(log_n)
    if inverse:
        w = pow(w, Rr - 2, Rr)
    out = []
    ninv, ginv = pow(n, Rr - 2, Rr), pow(FR.GENERATOR, Rr - 2, Rr)
    for k in ks:
        acc = 0
        for j, c in terms:
            t = c * pow(w, (j * k) % n, Rr)
            if coset and not inverse:
                t = t * pow(FR.GENERATOR, j, Rr)
            acc += t
        if inverse:
            acc = acc * ninv
            if coset:
                acc = acc * pow(ginv, k, Rr)
        out.append(acc % Rr)
    return out


def check_structured_inputs(ntt, log_n, t1, t2, modes=MODES):
    """ntt(words uint64 [n, 4] Montgomery, inverse, coset) -> transformed words; (t1, t2): the two-pass split of the size (the
    positions and the sample are placed on its digit boundaries whichever path the size takes)"""
    from oracle import bn254_fr as FR
    import random
    Rr = FR.R
    n, n2 = 1 << log_n, 1 << t2
    ks = sample_indices(log_n, t1, seed=log_n)
    assert len(ks) >= 256
    zero_row = np.zeros(4, dtype=np.uint64)
    g_n = pow(FR.GENERATOR, n, Rr)
    w = FR.root(log_n)
    for c in (1, Rr - 1):
        words = np.tile(S.mont_words_from_ints([c]), (n, 1))
        for inverse, coset in modes:
            out = ntt(words, inverse, coset)
            if coset and not inverse:
                got = S.ints_from_mont_words(out[ks])
                want = [c * (g_n - 1) % Rr * pow((FR.GENERATOR * pow(w, k, Rr) - 1) % Rr, Rr - 2, Rr) % Rr for k in ks]
                assert got == want, (c, inverse, coset)
            else:
                head = c if inverse else n * c % Rr
                assert S.ints_from_mont_words(out[:1]) == [head], (c, inverse, coset)
                nz = np.nonzero((out[1:] != zero_row).any(axis=1))[0]
                assert len(nz) == 0, "c = %#x, mode %s: output %d is %s, expected exact zero" % (c, (inverse, coset), nz[0] + 1, out[nz[0] + 1])
            del out
    rng = random.Random(1000 + log_n)
    positions = [0, 1, n2 - 1, n2, n2 + 1, n // 2, n - 1]
    extra = rng.randrange(n)
    while extra in positions:
        extra = rng.randrange(n)
    positions.append(extra)
    assert len(set(positions)) == 8
    terms = [(j, rng.randrange(1, Rr)) for j in positions]
    terms[1] = (terms[1][0], Rr - 1)
    words = np.zeros((n, 4), dtype=np.uint64)
    words[[j for j, _ in terms]] = S.mont_words_from_ints([c for _, c in terms])
    for inverse, coset in modes:
        out = ntt(words, inverse, coset)
        assert S.ints_from_mont_words(out[ks]) == transform_of_sparse(log_n, terms, inverse, coset, ks), (inverse, coset)
        del out
