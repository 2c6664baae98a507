"""GPU parity: Goldilocks NTT/LDE, Poseidon and Merkle kernels through the C ABI vs the oracle."""
import numpy as np
import pytest

from oracle import cport
from oracle import goldilocks as gl
from oracle import poseidon_gl as pg

pytestmark = pytest.mark.gpu
P = gl.P
INV, IN_BR, OUT_BR = 1, 2, 4


def rand_gl(rng, shape):
    # uniform in [0, p): rejection is irrelevant at 2^-32, clamp instead
    a = rng.integers(0, 2**64, size=shape, dtype=np.uint64)
    return np.where(a >= np.uint64(P), a - np.uint64(P), a)


def bitrev_perm(n):
    bits = n.bit_length() - 1
    return np.array([int(format(i, "0%db" % bits)[::-1], 2) if bits else 0 for i in range(n)])


@pytest.mark.parametrize("log_n", [0, 1, 2, 5, 8, 11, 12, 13, 14, 16, 18])
def test_ntt_forward_matches_oracle(zctx, log_n):
    rng = np.random.default_rng(log_n)
    batch = 3 if log_n < 16 else 2
    a = rand_gl(rng, (batch, 1 << log_n))
    want = cport.gl_ntt(a, nthreads=4)
    got = zctx.gl_ntt(a)
    assert np.array_equal(got, want)
    # bit-reversed output flag = same values, permuted
    got_br = zctx.gl_ntt(a, flags=OUT_BR)
    assert np.array_equal(got_br, want[:, bitrev_perm(1 << log_n)])
    # bit-reversed input (DIT path)
    got_dit = zctx.gl_ntt(a[:, bitrev_perm(1 << log_n)], flags=IN_BR)
    assert np.array_equal(got_dit, want)


@pytest.mark.parametrize("log_n", [1, 7, 12, 13, 17])
def test_ntt_inverse_roundtrip(zctx, log_n):
    rng = np.random.default_rng(100 + log_n)
    a = rand_gl(rng, (2, 1 << log_n))
    f = zctx.gl_ntt(a)
    assert np.array_equal(zctx.gl_ntt(f, flags=INV), a)
    assert np.array_equal(zctx.gl_ntt(a, flags=INV), cport.gl_ntt(a, inverse=True))
    # DIF forward (bit-reversed out) then DIT inverse (bit-reversed in): no permutation pass at all
    assert np.array_equal(zctx.gl_ntt(zctx.gl_ntt(a, flags=OUT_BR), flags=INV | IN_BR), a)


def test_small_ntt_matches_python_definition(zctx):
    rng = np.random.default_rng(9)
    a = rand_gl(rng, (1, 32))
    assert [int(x) for x in zctx.gl_ntt(a)[0]] == gl.naive_dft([int(x) for x in a[0]])


@pytest.mark.parametrize("log_n,rate_bits,batch", [(3, 3, 2), (9, 3, 5), (12, 3, 3), (10, 1, 2), (14, 3, 2), (12, 0, 1)])
def test_lde_matches_oracle(zctx, log_n, rate_bits, batch):
    rng = np.random.default_rng(log_n * 10 + rate_bits)
    c = rand_gl(rng, (batch, 1 << log_n))
    want = cport.gl_lde(c, rate_bits, 7, nthreads=4)
    assert np.array_equal(zctx.gl_lde(c, rate_bits, 7), want)
    N = 1 << (log_n + rate_bits)
    assert np.array_equal(zctx.gl_lde(c, rate_bits, 7, flags=OUT_BR), want[:, bitrev_perm(N)])
    # evaluation property: value k is the polynomial at 7 * w^k
    w = gl.root_of_unity(log_n + rate_bits)
    for k in [0, 1, N - 1]:
        assert int(want[0, k]) == gl.eval_poly([int(x) for x in c[0]], 7 * pow(w, k, P) % P)


@pytest.mark.parametrize("log_n,rate_bits", [(18, 3), (19, 3), (13, 0)])
def test_big_tile_sizes_match_oracle(zctx, log_n, rate_bits):
    """2^21 (the Ed25519 circuit's LDE) and 2^22 take the 2^13-element LDS tile (two passes instead of three), 2^13 a single pass:
    forward / inverse / DIT transforms and the LDE against the C oracle on one polynomial, round trip on a second"""
    rng = np.random.default_rng(500 + log_n)
    logN = log_n + rate_bits
    a = rand_gl(rng, (2, 1 << logN))
    want = cport.gl_ntt(a[:1], nthreads=8)
    f = zctx.gl_ntt(a, flags=OUT_BR)
    br = bitrev_fast(logN)
    assert np.array_equal(f[:1][:, br], want)
    assert np.array_equal(zctx.gl_ntt(f, flags=INV | IN_BR), a)
    assert np.array_equal(zctx.gl_ntt(a[:1], flags=INV), cport.gl_ntt(a[:1], inverse=True, nthreads=8))
    if rate_bits:
        c = rand_gl(rng, (1, 1 << log_n))
        assert np.array_equal(zctx.gl_lde(c, rate_bits, 7), cport.gl_lde(c, rate_bits, 7, nthreads=8))


def test_three_pass_size_matches_oracle(zctx):
    """2^23 is the smallest size whose default plan has three passes (csrc/gl_ntt_plan.h; 2^23 and 2^24 are accepted by
    zklc_plonky2_circuit_create): one polynomial forward to bit-reversed order against the C oracle, and the inverse brings it back"""
    rng = np.random.default_rng(523)
    a = rand_gl(rng, (1, 1 << 23))
    f = zctx.gl_ntt(a, flags=OUT_BR)
    assert np.array_equal(f[:, bitrev_fast(23)], cport.gl_ntt(a, nthreads=8))
    assert np.array_equal(zctx.gl_ntt(f, flags=INV | IN_BR), a)


def bitrev_fast(bits):
    idx = np.arange(1 << bits, dtype=np.uint64)
    out = np.zeros_like(idx)
    for b in range(bits):
        out |= ((idx >> np.uint64(b)) & np.uint64(1)) << np.uint64(bits - 1 - b)
    return out.astype(np.int64)


def test_lde_c3_shape_linearity(zctx):
    """Full C3 shape (2^17 -> 2^20) through size-independent properties: linearity and
    agreement with the oracle on one polynomial."""
    rng = np.random.default_rng(77)
    a, b = rand_gl(rng, (1, 1 << 17)), rand_gl(rng, (1, 1 << 17))
    s = ((a.astype(object) + b.astype(object)) % P).astype(np.uint64)
    la, lb, ls = (zctx.gl_lde(x, 3, 7, flags=OUT_BR) for x in (a, b, s))
    assert np.array_equal(((la.astype(object) + lb.astype(object)) % P).astype(np.uint64), ls)
    assert np.array_equal(la[:, bitrev_perm(1 << 20)], cport.gl_lde(a, 3, 7, nthreads=8))


def test_poseidon_permute(zctx):
    rng = np.random.default_rng(3)
    st = rand_gl(rng, (300, 12))
    st[0] = 0
    st[1] = P - 1
    out = zctx.poseidon_gl_permute(st)
    assert [int(x) for x in out[0]] == pg._J["kat_permute_zero"]  # goldilocks_test.go:47-53
    for i in range(300):
        assert [int(x) for x in out[i]] == cport.poseidon_gl_permute([int(x) for x in st[i]])


@pytest.mark.parametrize("width,log_leaves,cap", [(1, 0, 0), (3, 3, 0), (4, 4, 4), (5, 6, 2), (135, 9, 4), (20, 12, 4), (234, 10, 4), (16, 1, 0)])
def test_merkle_commit(zctx, width, log_leaves, cap):
    rng = np.random.default_rng(width * 31 + log_leaves)
    mat = rand_gl(rng, (width, 1 << log_leaves))
    cap_gpu, levels = zctx.gl_merkle_commit(mat, cap)
    want = cport.gl_merkle_commit(mat, cap, nthreads=4)
    assert len(levels) == len(want)
    for g, w in zip(levels, want):
        assert np.array_equal(g, w)
    if log_leaves <= 6:  # pin the C port against the Python restatement too, and open every leaf
        leaves = [[int(mat[p, i]) for p in range(width)] for i in range(1 << log_leaves)]
        cap_py, layers = pg.merkle_tree(leaves, cap)
        assert [[int(x) for x in d] for d in cap_gpu] == cap_py
        for i in range(1 << log_leaves):
            sib = [[int(x) for x in levels[l][(i >> l) ^ 1]] for l in range(log_leaves - cap)]
            assert pg.merkle_verify(leaves[i], i, sib, cap_py)


def test_hash_no_pad_kat_through_merkle(zctx):
    # tests/public_inputs_hash_test.go:54-55 is hash_no_pad([0,1,x]); a width-3 leaf is <= 4 elements (noop),
    # so pin the sponge through a width-5 leaf against the Python oracle and the KAT through the permutation
    kat = pg._J["kat_hash_no_pad"]
    st = np.zeros((1, 12), dtype=np.uint64)
    st[0, :3] = kat["in"]
    assert [int(x) for x in zctx.poseidon_gl_permute(st)[0, :4]] == kat["out"]


# ---- edge operands through the public kernels: the values at which a reduction can go wrong (tests/devsim_vectors.py) instead of
# uniform random data, which never takes the rare branches of the multiply-reduce
def edge_polys(n, seed):
    """six polynomials of n coefficients: alphabet draws, all p - 1, the powers of two 2^k, one non-zero coefficient at 0 / 1 / n - 1"""
    import random
    import devsim_vectors as DV
    rng = random.Random(seed)
    polys = [[rng.choice(DV.CANON) for _ in range(n)], [P - 1] * n, [pow(2, k, P) for k in range(n)]]
    for idx, v in ((0, P - 1), (1 % n, 2**32), (n - 1, 1)):
        d = [0] * n
        d[idx] = v
        polys.append(d)
    return np.array(polys, dtype=np.uint64)


@pytest.mark.parametrize("log_n", [4, 9, 13, 14])
def test_ntt_edge_inputs_match_oracle(zctx, log_n):
    n = 1 << log_n
    polys = edge_polys(n, log_n)
    br = bitrev_fast(log_n)
    for a in (polys[:3], polys[3:]):           # batch 3
        want = cport.gl_ntt(a, nthreads=4)
        want_inv = cport.gl_ntt(a, inverse=True, nthreads=4)
        assert np.array_equal(zctx.gl_ntt(a), want)
        assert np.array_equal(zctx.gl_ntt(a, flags=INV), want_inv)
        assert np.array_equal(zctx.gl_ntt(a, flags=OUT_BR), want[:, br])
        assert np.array_equal(zctx.gl_ntt(np.ascontiguousarray(a[:, br]), flags=IN_BR), want)
        assert np.array_equal(zctx.gl_ntt(np.ascontiguousarray(a[:, br]), flags=INV | IN_BR), want_inv)
        assert np.array_equal(zctx.gl_ntt(a, flags=INV | OUT_BR), want_inv[:, br])
    # a single coefficient 1 at index 0 transforms to all ones; all p - 1 to (-n, 0, 0, ...)
    assert np.array_equal(cport.gl_ntt(polys[1:2], nthreads=1)[0], np.array([(P - n) % P] + [0] * (n - 1), dtype=np.uint64))


@pytest.mark.parametrize("log_n,rate_bits", [(3, 3), (9, 3), (11, 3)])
def test_lde_edge_inputs_match_oracle(zctx, log_n, rate_bits):
    """the alphabet polynomials, and one whose coefficient j is built so that its multiplication by the coset scale 7^j takes a rare
    branch of the reduction: the borrow (low half of the product tiny; ~2^-33 per product under uniform data), or, for the small
    scales 7^j < 2^40 whose products have no top word to borrow, the result >= p without a carry (~2^-32)"""
    import random
    import devsim_vectors as DV
    n = 1 << log_n
    rng = random.Random(40 + log_n)
    hard, taken = [], 0
    for j in range(n):
        m = pow(7, j, P)
        c = DV.borrow_partner(m, rng.choice([1, 2, 3, 5]))
        if c >= P or not DV.mul_model(c, m)[1]:
            c = DV.ge_p_partner_small(m) if 1 < m < 2**32 else DV.ge_p_partner(m) if 1 < m < 2**40 else None
        if c is None or c >= P:
            c = rng.choice(DV.CANON)
        r = DV.mul_model(c, m)
        taken += r[1] or r[3]
        hard.append(c)
    assert taken >= n - 2, taken
    polys = np.concatenate([edge_polys(n, 100 + log_n), np.array([hard], dtype=np.uint64)])
    want = cport.gl_lde(polys, rate_bits, 7, nthreads=4)
    assert np.array_equal(zctx.gl_lde(polys, rate_bits, 7), want)
    assert np.array_equal(zctx.gl_lde(polys, rate_bits, 7, flags=OUT_BR), want[:, bitrev_fast(log_n + rate_bits)])
    w = gl.root_of_unity(log_n + rate_bits)
    for k in [0, 1, (n << rate_bits) - 1]:
        assert int(want[6, k]) == gl.eval_poly(hard, 7 * pow(w, k, P) % P)


def test_poseidon_permute_edge_states(zctx):
    import devsim_vectors as DV
    states = DV.poseidon_states(256, seed=21, loose=False)
    out = zctx.poseidon_gl_permute(np.array(states, dtype=np.uint64))
    for s, o in zip(states, out):
        want = pg.permute(s)
        assert [int(x) for x in o] == want == cport.poseidon_gl_permute(s)


@pytest.mark.parametrize("width", [5, 9, 135])
@pytest.mark.parametrize("cap", [0, 2])
def test_merkle_commit_edge_leaves(zctx, width, cap):
    import random
    import devsim_vectors as DV
    rng = random.Random(width * 7 + cap)
    log_leaves = 6
    mat = np.array([[rng.choice(DV.CANON) for _ in range(1 << log_leaves)] for _ in range(width)], dtype=np.uint64)
    mat[0, :] = P - 1
    mat[width - 1, 1::2] = 0
    cap_gpu, levels = zctx.gl_merkle_commit(mat, cap)
    want = cport.gl_merkle_commit(mat, cap, nthreads=4)
    assert len(levels) == len(want)
    for g, w in zip(levels, want):
        assert np.array_equal(g, w)
    leaves = [[int(mat[p, i]) for p in range(width)] for i in range(1 << log_leaves)]
    cap_py, _ = pg.merkle_tree(leaves, cap)
    assert [[int(x) for x in d] for d in cap_gpu] == cap_py
