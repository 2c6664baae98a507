"""The kernel arithmetic op tables ON THE DEVICE with edge operands: tests/devsim/devsim.hip compiles the arithmetic headers
(csrc/*.cuh) with hipcc and the library's flags behind one-lane-per-tuple kernels, so the device-only forms -- the inline-asm
statements of goldilocks_mul_asm.inc / poseidon_gl_asm.inc, the real DPP quad broadcast, hipcc's lowering of the limb arithmetic --
meet the operands tests/hostsim feeds the g++ build, plus operands constructed for the rare branches of the reductions
(tests/devsim_vectors.py).  References are Python integers; canonical results must be equal (and < p), loose results equal mod p.
No tolerances."""
import ctypes
import importlib
import importlib.util
import os
import random

import numpy as np
import pytest

import devsim_vectors as DV
from oracle import goldilocks as gl
from oracle import poseidon_gl as pg

pytestmark = pytest.mark.gpu
P = gl.P
M = 2**64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def devsim():
    import zklc_amd  # noqa: F401  (first: the package's hardware-queue setting applies to this process)
    b = importlib.import_module("zk-light-client-implementation_amd.build")
    if os.path.exists(b.HIPCC) and not b.devsim_is_current():
        b.build_devsim(verbose=False)
    if not os.path.exists(b.DEVSIM_LIB):
        pytest.fail("tests/devsim/libdevsim.so is missing and there is no hipcc to build it: run __graft_entry__.build()")
    return ctypes.CDLL(b.DEVSIM_LIB)


def _load_tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def arr(vals, dtype=np.uint64):
    return np.ascontiguousarray(np.array(vals, dtype=dtype).reshape(-1))


def ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def run(fn, *args):
    """numpy arrays go as pointers, integers as 32-bit values; a non-zero return is a HIP error"""
    rc = fn(*[ptr(a) if isinstance(a, np.ndarray) else ctypes.c_uint32(a) for a in args])
    assert rc == 0, "%s: HIP error %d" % (fn.__name__, rc)


def ints(a):
    return [int(v) for v in a]


# ------------------------------------------------------------------------------------------------ Goldilocks
def gl_op(devsim, op, a, b):
    aa, bb = arr(a), arr(b)
    out = np.zeros(len(aa), dtype=np.uint64)
    run(devsim.devsim_gl_op, op, aa, bb, out, len(aa))
    return ints(out)


def test_gl_field_ops(devsim):
    rng = random.Random(1)
    vals = DV.CANON + [P >> 1, 0xFFFFFFFF] + [rng.randrange(P) for _ in range(60)]
    pairs = [(a, b) for a in vals for b in DV.CANON + rng.sample(vals, 6)]
    pools = DV.mul_pools(rng)
    hard = pools["borrow"] + pools["ge_p"]
    pairs = [p for k, p in enumerate(pairs)] + hard + [(b, a) for a, b in hard]
    rng.shuffle(pairs)                       # constructed and ordinary operands side by side in every wave
    assert len(pairs) % 64 and len(pairs) > 1024
    flags = [DV.mul_model(a, b) for a, b in pairs]
    assert sum(f[1] for f in flags) >= 64 and sum(f[3] for f in flags) >= 64
    a, b = [p[0] for p in pairs], [p[1] for p in pairs]
    assert gl_op(devsim, 0, a, b) == [(x + y) % P for x, y in pairs]
    assert gl_op(devsim, 1, a, b) == [(x - y) % P for x, y in pairs]
    assert gl_op(devsim, 2, a, b) == [x * y % P for x, y in pairs]
    inv_in = [v for v in vals if v][:70]
    assert gl_op(devsim, 3, inv_in, [0] * len(inv_in)) == [pow(v, P - 2, P) for v in inv_in]
    ks = list(range(0, 33))
    assert gl_op(devsim, 5, ks, [0] * len(ks)) == [gl.root_of_unity(k) for k in ks]
    # reduce128 (canonical and loose) on (lo, hi): corners, the products of the constructed pairs, random
    wide = [(M - 1, M - 1), (0, M - 1), (M - 1, 0), (0, 0xFFFFFFFF), (0, 0xFFFFFFFF00000000), (P - 1, P - 1), (0, 0xFFFFFFFF00000001)]
    wide += [((x * y) % M, (x * y) >> 64) for x, y in hard] + [(rng.getrandbits(64), rng.getrandbits(64)) for _ in range(1500)]
    wide += [(lo, hi) for lo in DV.LOOSE for hi in DV.LOOSE]
    rng.shuffle(wide)
    lo, hi = [w[0] for w in wide], [w[1] for w in wide]
    want = [((h << 64) | l) % P for l, h in wide]
    assert gl_op(devsim, 4, lo, hi) == want
    assert [v % P for v in gl_op(devsim, 6, lo, hi)] == want


def test_gl_loose_ops(devsim):
    rng = random.Random(11)
    loose = DV.LOOSE + [rng.randrange(P, M) for _ in range(50)] + [rng.randrange(M) for _ in range(20)]
    canon = DV.CANON + [rng.randrange(P) for _ in range(50)]
    assert gl_op(devsim, 9, loose, [0] * len(loose)) == [a % P for a in loose]
    pairs = [(a, b) for a in loose for b in canon]
    got = gl_op(devsim, 7, [p[0] for p in pairs], [p[1] for p in pairs])
    assert [g % P for g in got] == [(a + b) % P for a, b in pairs]
    pools = DV.mul_pools(rng)
    pairs = [(a, b) for a in loose for b in DV.LOOSE + canon[:12]] + pools["borrow"] + pools["ge_p"]
    rng.shuffle(pairs)
    assert sum(DV.loose_mul_model(a, b)[1] for a, b in pairs) >= 64
    got = gl_op(devsim, 8, [p[0] for p in pairs], [p[1] for p in pairs])
    assert [g % P for g in got] == [a * b % P for a, b in pairs]


@pytest.mark.parametrize("fixed", [1, 0], ids=["constant_exponent", "runtime_exponent"])
def test_gl_mul_2exp(devsim, fixed):
    rng = random.Random(7)
    xs = DV.LOOSE + [rng.randrange(P) for _ in range(20)] + [rng.randrange(M) for _ in range(6)]
    tuples = [(x, e) for e in range(96) for x in xs]
    rng.shuffle(tuples)
    x, e = arr([t[0] for t in tuples]), arr([t[1] for t in tuples], np.uint32)
    out = np.zeros(len(tuples), dtype=np.uint64)
    run(devsim.devsim_gl_mul_2exp, x, e, fixed, out, len(tuples))
    assert ints(out) == [v * pow(2, k, P) % P for v, k in tuples]


def test_gl_accumulators(devsim):
    rng = random.Random(12)
    n = 70
    for length in [1, 2, 12, 13, 200]:
        xs, ys = [], []
        for i in range(n):
            xs += [[M - 1] * length, [rng.randrange(P, M) for _ in range(length)], [rng.randrange(M) for _ in range(length)],
                   [rng.choice(DV.LOOSE) for _ in range(length)]][i % 4]
            ys += [M - 1 if (k + i) % 2 else P - 1 for k in range(length)] if i % 8 < 4 else [rng.choice(DV.LOOSE) for _ in range(length)]
        x, y, out = arr(xs), arr(ys), np.zeros(n, dtype=np.uint64)
        run(devsim.devsim_gl_acc, x, y, length, out, n)
        want = [sum(a * b for a, b in zip(xs[i * length:(i + 1) * length], ys[i * length:(i + 1) * length])) % P for i in range(n)]
        assert ints(out) == want, length
    for length, fold in [(1, 0), (3, 0), (357, 0), (511, 0), (2000, 480), (2000, 384), (1000, 1)]:
        xs, ks = [], []
        for i in range(n):
            kind = i % 4
            xs += [M - 1] * length if kind < 2 else [rng.randrange(M) for _ in range(length)] if kind == 2 else \
                [rng.choice(DV.LOOSE) for _ in range(length)]
            ks += [P - 1] * length if kind == 0 else [(1 << 44) - 1 | ((1 << 20) - 1) << 44] * length if kind == 1 else \
                [rng.randrange(P) for _ in range(length)] if kind == 2 else [rng.choice(DV.CANON) for _ in range(length)]
        x, k, out = arr(xs), arr(ks), np.zeros(n, dtype=np.uint64)
        run(devsim.devsim_gl_acc3, x, k, length, fold, out, n)
        want = [sum(a * b for a, b in zip(xs[i * length:(i + 1) * length], ks[i * length:(i + 1) * length])) % P for i in range(n)]
        assert ints(out) == want, (length, fold)


def test_gl2_extension_ops(devsim):
    from oracle.plonky2_verifier import ext_pow
    rng = random.Random(9)
    comps = [0, 1, P - 1, P - 2, 2**32 - 1, 2**32, 2**63, P - 2**32]
    vals = [(0, 0), (1, 0), (0, 1), (P - 1, P - 1), (P - 1, 0)] + [(a, b) for a in comps[:4] for b in comps[4:]] + \
        [(rng.randrange(P), rng.randrange(P)) for _ in range(40)]
    pairs = [(a, b) for a in vals for b in rng.sample(vals, 5)]
    es = [rng.getrandbits(40) for _ in pairs]

    def call(op, ps):
        a, b, e = arr([c for p in ps for c in p[0]]), arr([c for p in ps for c in p[1]]), arr(es[:len(ps)])
        out = np.zeros(2 * len(ps), dtype=np.uint64)
        run(devsim.devsim_gl2_op, op, a, b, e, out, len(ps))
        o = ints(out)
        return [(o[2 * i], o[2 * i + 1]) for i in range(len(ps))]
    assert call(0, pairs) == [gl.ext_add(a, b) for a, b in pairs]
    assert call(1, pairs) == [gl.ext_sub(a, b) for a, b in pairs]
    assert call(2, pairs) == [gl.ext_mul(a, b) for a, b in pairs]
    assert call(3, pairs) == [gl.ext_mul(a, a) for a, _ in pairs]
    nz = [p for p in pairs if p[0] != (0, 0)]
    assert [gl.ext_mul(r, p[0]) for r, p in zip(call(4, nz), nz)] == [(1, 0)] * len(nz)
    assert call(5, pairs[:80]) == [ext_pow(a, e) for (a, _), e in zip(pairs[:80], es)]


@pytest.mark.parametrize("width", [1, 2, 3, 4, 5, 6, 7, 8, 15])
def test_gl_mul_batch_takes_every_reduction_branch_at_every_slot(devsim, width):
    """gl_mul_batch<N> = the statements gl_mul{4,3,2}_asm in every split (N = 5 is 3 + 2, 15 is 4 + 4 + 4 + 3) and gl_mul for a
    last single element.  The set is classified by the big-integer model first: borrow, carry and TP >= p at every slot, in every
    wave next to lanes that do not take them."""
    x, t, want, flags = DV.mul_batch_vectors(width)
    n = DV.N_TUPLES
    DV.assert_coverage(flags, n, width, DV.MUL_BRANCHES)
    xa, ta, out = arr(x), arr(t), np.zeros(n * width, dtype=np.uint64)
    run(devsim.devsim_gl_mul_batch, width, xa, ta, out, n)
    got = ints(out)
    bad = [(k // width, k % width, x[k], t[k], got[k], want[k]) for k in range(n * width) if got[k] != want[k]]
    assert not bad, "%d wrong products (tuple, slot, a, b, got, want): %s" % (len(bad), bad[:4])


@pytest.mark.parametrize("width", [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16, 18])
def test_p2_range_products4_takes_every_branch_at_every_slot(devsim, width):
    """p2_range_products4<N> = p2_range4_{4,3,2}_asm in every split (1..9) and the widths the evaluators use (12, 16, 18): the
    borrow of x - 3 (x = 0, 1, 2), the carry of y + 2 (its two operands) and the borrow of the first reduction at every slot"""
    x, want, flags = DV.range4_vectors(width)
    n = DV.N_TUPLES
    DV.assert_coverage(flags, n, width, DV.RANGE_BRANCHES)
    xa, out = arr(x), np.zeros(n * width, dtype=np.uint64)
    run(devsim.devsim_p2_range_products4, width, xa, out, n)
    got = [v % P for v in ints(out)]
    bad = [(k // width, k % width, x[k], got[k], want[k]) for k in range(n * width) if got[k] != want[k]]
    assert not bad, "%d wrong range products (tuple, slot, x, got, want): %s" % (len(bad), bad[:4])


@pytest.mark.parametrize("g,dit,inverse,zp", [(g, d, i, 0) for g in (1, 2, 3, 4) for d in (0, 1) for i in (0, 1)] + [(3, 0, 0, 3), (4, 0, 0, 3)])
def test_gl_ntt_group(devsim, g, dit, inverse, zp):
    """gl_ntt_group_regs<G, DIT, INV, ZP>: shift twiddles inside, gl_mul_batch<2^G - 1> on the way out (DIF) or in (DIT), against
    the definition; table entries include the borrow partners of the values they multiply"""
    n = 389
    x, t, want, flags = DV.ntt_group_vectors(g, dit, inverse, zp, n=n)
    assert sum(flags["borrow"]) >= 64 and sum(flags["carry"]) >= 64
    if zp:      # the padded positions must not be read: the harness poisons them, hand it garbage as well
        Mg = 1 << g
        x = [v if k % Mg < (Mg >> zp) else 0x0123456789ABCDEF for k, v in enumerate(x)]
    xa, ta, out = arr(x), arr(t), np.zeros(n << g, dtype=np.uint64)
    run(devsim.devsim_gl_ntt_group, g, dit, inverse, zp, xa, ta, out, n)
    assert ints(out) == want


# ------------------------------------------------------------------------------------------------ Poseidon-Goldilocks
@pytest.fixture(scope="module")
def pgl_consts():
    return _load_tool("gen_poseidon_asm").load_constants()[0]


def _full_round_ref(c, st, layer):
    y = [pow(x, 7, P) for x in st]
    mds = [17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20]
    return [(sum(mds[i] * y[(i + r) % 12] for i in range(12)) + (8 * y[0] if r == 0 else 0) + c["next"][layer][r]) % P for r in range(12)]


def _pgl_piece(devsim, piece, layer, use_asm, states):
    a = arr([v for s in states for v in s])
    out = np.zeros(len(a), dtype=np.uint64)
    run(devsim.devsim_pgl_piece, piece, layer, use_asm, a, out, len(states))
    o = ints(out)
    return [[v % P for v in o[12 * i:12 * i + 12]] for i in range(len(states))]


@pytest.mark.parametrize("use_asm", [1, 0], ids=["asm", "compiled"])
def test_pgl_gate_full_rounds(devsim, pgl_consts, use_asm):
    """pgl_gate_full_round<ASM> for the constant layers 0-2 and 4-7 and pgl_gate_full_round_init<ASM>, loose states in and out: the
    statement pgl_asm_full_round / pgl_asm_full_round_init, and the loose C++ forms as hipcc compiles them"""
    states = DV.poseidon_states(197, seed=5)
    for layer in (0, 1, 2, 4, 5, 6, 7):
        assert _pgl_piece(devsim, 0, layer, use_asm, states) == [_full_round_ref(pgl_consts, s, layer) for s in states], layer
    want = []
    for s in states:
        t = _full_round_ref(pgl_consts, s, 3)
        want.append([t[0]] + [sum(t[r] * pgl_consts["init"][r - 1][d - 1] for r in range(1, 12)) % P for d in range(1, 12)])
    assert _pgl_piece(devsim, 1, 0, use_asm, states) == want


def test_pgl_partial_rounds_statement(devsim, pgl_consts):
    """pgl_asm_partial_rounds (two lazy blocks of eleven rounds + the constant layer behind them) against the 22 fast partial rounds
    round by round"""
    c = pgl_consts
    states = DV.poseidon_states(197, seed=6)
    want = []
    for st in states:
        cur = [v % P for v in st]
        for rnd in range(22):
            y = (pow(cur[0], 7, P) + c["fp_rc"][rnd]) % P
            d = (25 * y + sum(c["w"][rnd][j - 1] * cur[j] for j in range(1, 12))) % P
            cur = [d] + [(cur[j] + y * c["v"][rnd][j - 1]) % P for j in range(1, 12)]
        want.append([(x + k) % P for x, k in zip(cur, c["rc26"])])
    assert _pgl_piece(devsim, 2, 0, 1, states) == want


def test_poseidon_gl_permute_hash_two_to_one(devsim):
    rng = random.Random(2)
    states = DV.poseidon_states(197, seed=7, loose=False)
    a = arr([v for s in states for v in s])
    out = np.zeros(len(a), dtype=np.uint64)
    run(devsim.devsim_poseidon_gl_permute, a, out, len(states))
    o = ints(out)
    assert o[:12] == pg._J["kat_permute_zero"] and max(o) < P
    assert [o[12 * i:12 * i + 12] for i in range(len(states))] == [pg.permute(s) for s in states]
    n = 67
    for length in list(range(18)) + [135]:
        rows = [[rng.choice(DV.CANON) if (i + k) % 3 == 0 else rng.randrange(P) for k in range(length)] for i in range(n)]
        a = arr([v for r in rows for v in r] or [0])
        out = np.zeros(4 * n, dtype=np.uint64)
        run(devsim.devsim_poseidon_gl_hash, a, length, out, n)
        o = ints(out)
        assert [o[4 * i:4 * i + 4] for i in range(n)] == [pg.hash_or_noop(r) for r in rows], length
    ls = [[rng.choice(DV.CANON) if i % 2 else rng.randrange(P) for _ in range(4)] for i in range(n)]
    rs = [[rng.choice(DV.CANON) if i % 3 == 0 else rng.randrange(P) for _ in range(4)] for i in range(n)]
    la, ra, out = arr([v for r in ls for v in r]), arr([v for r in rs for v in r]), np.zeros(4 * n, dtype=np.uint64)
    run(devsim.devsim_poseidon_gl_two_to_one, la, ra, out, n)
    o = ints(out)
    assert [o[4 * i:4 * i + 4] for i in range(n)] == [pg.two_to_one(l, r) for l, r in zip(ls, rs)]


# ------------------------------------------------------------------------------------------------ gate evaluators
def _gate_rows(g, n, rng, special):
    """n wire rows: random / values 0..3 (the range-check products around their roots) / the alphabet / the alphabet and the
    operands of the rare range-check branches, interleaved"""
    rows = []
    for i in range(n):
        pick = [lambda: rng.randrange(P), lambda: rng.randrange(4), lambda: rng.choice(DV.CANON), lambda: rng.choice(special)][i % 4]
        rows.append([pick() for _ in range(max(g.num_wires, 1))])
    return rows


def _eval_gate(devsim, code, g, rows, consts, pih, alphas):
    from zklc_amd.plonky2 import gates as G, synthetic as SY
    params = arr(list(g.params), np.uint32)
    extra = np.zeros(1, dtype=np.uint64)
    if g.code == G.COSET_INTERPOLATION:
        w = SY.root_of_unity(g.subgroup_bits)
        extra = arr(list(g.weights) + [pow(w, j, P) for j in range(1 << g.subgroup_bits)])
    n, nw, nc = len(rows), len(rows[0]), len(consts[0])
    wa, ca, pa, aa = arr([v for r in rows for v in r]), arr([v for r in consts for v in r]), arr(pih), arr(alphas)
    out = np.zeros(2 * n, dtype=np.uint64)
    run(devsim.devsim_p2_eval_gate, code, params, extra, len(extra), wa, nw, ca, nc, pa, aa, 2, out, n)
    o = ints(out)
    return [o[2 * i:2 * i + 2] for i in range(n)]


def _gates():
    from test_hostsim_plonky2_gates import GATES
    return GATES


@pytest.mark.parametrize("k", range(27))
def test_gate_evaluators(devsim, k):
    """p2_eval_gate on the device for every entry of GATES (tests/test_hostsim_plonky2_gates.py): one gate type per kernel as in the
    quotient kernels, one row per lane, sum_i alpha^i constraint_i for two challenges against the oracle's evaluators"""
    from oracle import plonky2_gates as OG
    gates = _gates()
    assert len(gates) == 27
    g = gates[k]
    og = OG.gate_from_id(g.id())
    rng = random.Random(1000 + k)
    special = DV.CANON + [x for x, _ in DV.add2_carry_candidates()] + DV.mul1_borrow_candidates(rng, 8)
    n = 150
    rows = _gate_rows(g, n, rng, special)
    consts = [[rng.choice(DV.CANON) if i % 5 == 4 else rng.randrange(P) for _ in range(g.num_constants)] + [0] for i in range(n)]
    pih = [rng.randrange(P) for _ in range(4)]
    alphas = [rng.randrange(P), rng.choice([P - 1, 2**32, rng.randrange(P)])]
    got = _eval_gate(devsim, g.code, g, rows, consts, pih, alphas)
    for i in range(n):
        cs = og.eval(OG.BaseK, consts[i][:g.num_constants], rows[i], pih)
        assert got[i] == [OG.reduce_with_powers(OG.BaseK, cs, a) for a in alphas], (g.id(), i)


@pytest.mark.parametrize("code", [7, 100, 101, 110], ids=["default", "lazy", "lazy_rolled", "loose"])
def test_poseidon_gate_forms(devsim, code):
    """the default evaluator of the Poseidon gate and its A/B forms (types 100, 101, 110: the full-round statements between the
    constraints, the lazy partial rounds unrolled / rolled over LDS, the loose round-by-round form) on random rows, rows from the
    edge alphabet, and satisfying rows (every constraint zero) next to rows with one S-box wire off by one"""
    from oracle import plonky2_gates as OG
    from zklc_amd.plonky2 import gates as G
    from zklc_amd.plonky2.prover import poseidon_gate_rows
    g = G.PoseidonGate()
    assert g.code == 7
    og = OG.gate_from_id(g.id())
    rng = random.Random(77)
    rows = []
    for i in range(96):
        r = [rng.randrange(P) for _ in range(g.num_wires)] if i % 3 else [rng.choice(DV.CANON) for _ in range(g.num_wires)]
        if i % 2:
            r[24] = rng.randrange(2)
        rows.append(r)
    ins = np.array([[rng.randrange(P) for _ in range(12)] for _ in range(24)], dtype=np.uint64)
    sat = [ints(r) for r in poseidon_gate_rows(ins, np.array([k % 2 for k in range(24)], dtype=np.uint64))]
    for k, r in enumerate(sat):
        rows.append(r)
        broken = list(r)
        broken[65 + k % 22] = (broken[65 + k % 22] + 1) % P
        rows.append(broken)
    alphas = [rng.randrange(P), rng.randrange(P)]
    got = _eval_gate(devsim, code, g, rows, [[0]] * len(rows), [0] * 4, alphas)
    for i, r in enumerate(rows):
        cs = og.eval(OG.BaseK, [], r, [0] * 4)
        assert got[i] == [OG.reduce_with_powers(OG.BaseK, cs, a) for a in alphas], i
    assert all(got[96 + 2 * k] == [0, 0] and got[97 + 2 * k] != [0, 0] for k in range(24))


# ------------------------------------------------------------------------------------------------ BN254
def w8(x):
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def from_w(ws):
    return sum(int(w) << (32 * i) for i, w in enumerate(ws))


def test_bn254_fp_ops(devsim):
    from oracle import bn254 as bn
    Q, R = bn.P, bn.MONT_R
    rinv = bn.inv(R)
    rng = random.Random(4)
    edge = [0, 1, 2, 3, Q - 1, Q - 2, (Q - 1) // 2]
    vals = edge + [rng.randrange(Q) for _ in range(60)]
    pairs = [(a, b) for a in vals for b in rng.sample(vals, 6) + edge]

    def fop(op, ps):
        a = arr([w for p in ps for w in w8(p[0] * R % Q)], np.uint32)
        b = arr([w for p in ps for w in w8(p[1] * R % Q)], np.uint32)
        out = np.zeros(8 * len(ps), dtype=np.uint32)
        run(devsim.devsim_fp_op, op, a, b, out, len(ps))
        return [from_w(out[8 * i:8 * i + 8]) * rinv % Q for i in range(len(ps))]
    assert fop(0, pairs) == [(a + b) % Q for a, b in pairs]
    assert fop(1, pairs) == [(a - b) % Q for a, b in pairs]
    assert fop(2, pairs) == [a * b % Q for a, b in pairs]
    assert fop(3, pairs) == [a * a % Q for a, _ in pairs]
    assert fop(5, pairs) == [((a * b - a - 2 * b) * (a + b + a * a)) % Q for a, b in pairs]
    nz = [(a, 0) for a in vals if a][:70]
    assert fop(4, nz) == [pow(a, Q - 2, Q) for a, _ in nz]


def test_bn254_weak_reduction_edges(devsim):
    """fp_wred on raw lazy limb vectors (|value| <= 64 p): the operands of tests/test_hostsim_pairing.py, in one batch"""
    from oracle import bn254 as B
    rng = random.Random(1)
    lims, vals = [], []
    for trial in range(1200):
        k = rng.choice([-64, -63, -17, -2, -1, 0, 1, 2, 9, 31, 63, 64])
        x = rng.randrange(B.P) if trial % 3 else rng.choice([0, 1, B.P - 1])
        target = x + k * B.P if trial % 2 else max(min(x + k * B.P, 64 * B.P), -64 * B.P)
        limbs = [rng.randrange(-(1 << 29), 1 << 29) for _ in range(9)]
        rest = target - sum(l << (26 * i) for i, l in enumerate(limbs))
        top, rem = divmod(rest, 1 << 234)
        limbs[0] += rem & 0x3ffffff
        limbs[1] += (rem >> 26) & 0x3ffffff
        val = sum(l << (26 * i) for i, l in enumerate(limbs)) + (top << 234)
        if abs(top) >= (1 << 30) or abs(val) > 64 * B.P:
            continue
        lims.append(limbs + [top])
        vals.append(val)
    n = len(vals)
    assert n > 900
    la = arr([l for v in lims for l in v], np.int32)
    out_l, out_w = np.zeros(10 * n, dtype=np.int32), np.zeros(8 * n, dtype=np.uint32)
    run(devsim.devsim_fp_wred, la, out_l, out_w, n)
    for i, val in enumerate(vals):
        ol = ints(out_l[10 * i:10 * i + 10])
        got = sum(l << (26 * k) for k, l in enumerate(ol))
        assert (got - val) % B.P == 0 and abs(got) < 2 * B.P, i
        assert all(0 <= l < (1 << 26) for l in ol[:9])
        assert from_w(out_w[8 * i:8 * i + 8]) == val % B.P


def test_bn254_fp12_tower_ops(devsim):
    from oracle import bn254 as B
    from oracle import bn254_pairing as PR
    rng = random.Random(2)
    rinv = B.inv(B.MONT_R)

    def f12w(a):
        return [w for x in PR.f12_flat(a) for w in w8(x * B.MONT_R % B.P)]

    def f12_from(w):
        v = [from_w(w[8 * i:8 * i + 8]) * rinv % B.P for i in range(12)]
        c = [(v[2 * i], v[2 * i + 1]) for i in range(6)]
        return ((c[0], c[1], c[2]), (c[3], c[4], c[5]))

    def rand_f12():
        return tuple(tuple((rng.randrange(B.P), rng.randrange(B.P)) for _ in range(3)) for _ in range(2))
    edge = (((B.P - 1, B.P - 1),) * 3,) * 2
    sparse = (((1, 0), (0, 0), (B.P - 1, 0)), ((0, 0), (0, 1), (0, 0)))
    pairs = [(rand_f12(), rand_f12()) for _ in range(8)] + [(edge, edge), (PR.F12_ONE, rand_f12()), (sparse, edge), (edge, sparse)]
    pairs = pairs * 6          # 72 lanes: more than a wave, every operand kind beside every other
    a, b = arr([w for p in pairs for w in f12w(p[0])], np.uint32), arr([w for p in pairs for w in f12w(p[1])], np.uint32)
    refs = [lambda x, y: PR.f12_mul(x, y), lambda x, y: PR.f12_sqr(x), lambda x, y: PR.f12_inv(x), lambda x, y: PR.f12_frobenius(x, 1),
            lambda x, y: PR.f12_frobenius(x, 2), lambda x, y: PR.f12_conj(x)]
    want = [[f(x, y) for x, y in pairs[:12]] * 6 for f in refs]
    for op in range(6):
        out = np.zeros(96 * len(pairs), dtype=np.uint32)
        run(devsim.devsim_f12_op, op, a, b, out, len(pairs))
        assert [f12_from(out[96 * i:96 * i + 96]) for i in range(len(pairs))] == want[op], op


def test_bn254_curve_ops(devsim):
    from oracle import bn254 as B
    rng = random.Random(5)
    rinv = B.inv(B.MONT_R)
    mw = lambda x: w8(x * B.MONT_R % B.P)
    un = lambda ws: from_w(ws) * rinv % B.P
    G1 = B.G1
    A, Bp = B.mul(12345, G1), B.mul(99999, G1)
    rnd = [(B.hash_to_curve(7, rng.randrange(10**6)), B.hash_to_curve(7, rng.randrange(10**6))) for _ in range(6)]
    # (op, P, Q, repetitions, expected)
    cases = [(0, A, Bp, 0, B.add(A, Bp)), (1, A, Bp, 0, B.add(A, B.neg(Bp))), (2, A, None, 0, B.add(A, A)), (0, A, A, 0, B.add(A, A)),
             (1, A, A, 0, None), (0, None, Bp, 0, Bp), (0, A, None, 0, A), (3, A, Bp, 0, B.mul(2, B.add(A, Bp))), (5, A, Bp, 0, B.add(A, Bp)),
             (5, A, B.neg(A), 0, None), (5, None, Bp, 0, Bp), (4, A, Bp, 50, B.add(A, B.mul(50, Bp))), (4, None, G1, 7, B.mul(7, G1))]
    cases += [(0, X, Y, 0, B.add(X, Y)) for X, Y in rnd] + [(5, X, Y, 0, B.add(X, Y)) for X, Y in rnd]
    for op in range(6):
        cs = [c for c in cases if c[0] == op] * 9          # the same op for the whole launch, as hostsim's switch
        if not cs:
            continue
        pt = lambda p: [0] * 16 if p is None else mw(p[0]) + mw(p[1])
        pa, qa = arr([w for c in cs for w in pt(c[1])], np.uint32), arr([w for c in cs for w in pt(c[2])], np.uint32)
        pi, qi = arr([int(c[1] is None) for c in cs], np.uint32), arr([int(c[2] is None) for c in cs], np.uint32)
        reps = arr([c[3] for c in cs], np.uint32)
        out, inf = np.zeros(16 * len(cs), dtype=np.uint32), np.zeros(len(cs), dtype=np.uint32)
        run(devsim.devsim_g1_op, op, pa, pi, qa, qi, reps, out, inf, len(cs))
        got = [None if inf[i] else (un(out[16 * i:16 * i + 8]), un(out[16 * i + 8:16 * i + 16])) for i in range(len(cs))]
        assert got == [c[4] for c in cs], op
    p, q = B.g2_mul(1234567, B.G2), B.g2_mul(7654321, B.G2)
    g2w = lambda t: mw(t[0][0]) + mw(t[0][1]) + mw(t[1][0]) + mw(t[1][1])
    g2cases = [(0, p, q, B.g2_add(p, q)), (1, p, q, B.g2_add(p, B.g2_neg(q))), (2, p, q, B.g2_add(p, p)), (0, p, p, B.g2_add(p, p)),
               (1, p, p, None), (3, p, q, B.g2_add(B.g2_add(p, q), p)), (0, q, p, B.g2_add(p, q)), (2, q, p, B.g2_add(q, q))]
    for op in range(4):
        cs = [c for c in g2cases if c[0] == op] * 33
        pa, qa = arr([w for c in cs for w in g2w(c[1])], np.uint32), arr([w for c in cs for w in g2w(c[2])], np.uint32)
        out, inf = np.zeros(32 * len(cs), dtype=np.uint32), np.zeros(len(cs), dtype=np.uint32)
        run(devsim.devsim_g2_op, op, pa, qa, out, inf, len(cs))
        got = []
        for i in range(len(cs)):
            c = [un(out[32 * i + 8 * k:32 * i + 8 * k + 8]) for k in range(4)]
            got.append(None if inf[i] else ((c[0], c[1]), (c[2], c[3])))
        assert got == [c[3] for c in cs], op


@pytest.mark.parametrize("coop", [0, 1], ids=["one_lane", "four_lanes_dpp"])
def test_poseidon_bn254_permute(devsim, coop):
    """the permutation on one lane, and poseidon_bn254_permute_coop with the REAL quad broadcast (DPP; hostsim walks an emulation):
    37 states = 148 lanes, so the last wave holds idle quads next to live ones"""
    from oracle import poseidon_bn254 as pb
    rng = random.Random(1)
    states = [k["in"] for k in pb.KATS] + [[0] * 4, [pb.R - 1] * 4, [1, pb.R - 1, 0, 2**253]]
    states += [[rng.randrange(pb.R) for _ in range(4)] for _ in range(37 - len(states))]
    assert len(states) == 37
    a = arr([w for s in states for x in s for w in w8(x)], np.uint32)
    out = np.zeros(len(a), dtype=np.uint32)
    run(devsim.devsim_poseidon_bn254_permute, coop, a, out, len(states))
    got = [[from_w(out[32 * i + 8 * k:32 * i + 8 * k + 8]) for k in range(4)] for i in range(len(states))]
    for k, kat in enumerate(pb.KATS):
        assert got[k] == kat["out"]
    assert got == [pb.permute(s) for s in states]


# ------------------------------------------------------------------------------------------------ Ed25519
def test_ed25519_field_ops(devsim):
    from oracle import ed25519_ref as ref
    Q = ref.P
    rng = random.Random(1)
    T = 2**255
    edge = [0, 1, 2, 19, 38, Q - 1, Q, Q + 1, T - 1, T - 19, T - 20, 2**254, 2**26 - 1, 2**51 - 1, (1 << 230) - 1]
    vals = edge + [rng.getrandbits(255) for _ in range(60)]
    pairs = [(a, b) for a in vals for b in rng.sample(vals, 8) + edge[:6] + [T - 1]]

    def fe_op(op, ps):
        a, b = arr([w for p in ps for w in w8(p[0])], np.uint32), arr([w for p in ps for w in w8(p[1])], np.uint32)
        out = np.zeros(8 * len(ps), dtype=np.uint32)
        run(devsim.devsim_fe_op, op, a, b, out, len(ps))
        return [from_w(out[8 * i:8 * i + 8]) for i in range(len(ps))]
    assert fe_op(0, pairs) == [(a + b) % Q for a, b in pairs]
    assert fe_op(1, pairs) == [(a - b) % Q for a, b in pairs]
    assert fe_op(2, pairs) == [a * b % Q for a, b in pairs]
    assert fe_op(8, pairs) == [((2 * a + b) * (b - 2 * a)) % Q for a, b in pairs]
    ones = [(a, 0) for a in vals]
    assert fe_op(3, ones) == [a * a % Q for a in vals]
    assert fe_op(7, ones) == [2 * a * a % Q for a in vals]
    assert fe_op(6, ones) == [a % Q for a in vals]
    assert fe_op(4, ones) == [pow(a, Q - 2, Q) for a in vals]
    assert fe_op(5, ones) == [pow(a, (Q - 5) // 8, Q) for a in vals]


def test_ed25519_scalars(devsim):
    from oracle import ed25519_ref as ref
    L = ref.L
    rng = random.Random(2)
    top = 2**512 // L
    xs = [0, 1, L - 1, L, L + 1, 2**512 - 1, 2**512 - L, top * L, top * L - 1, 2**252, 2**253 - 1, 2**504, 2**256 - 1, 2**256]
    for k in [2, 3, 2**125, 2**128, 2**252, 2**253, 2**259 - 1, top // 2, top - 1, top] + [rng.randrange(top) for _ in range(40)]:
        xs += [v for v in (k * L - 1, k * L, k * L + 1) if 0 <= v < 2**512]
    xs += [rng.getrandbits(512) for _ in range(300)] + [rng.getrandbits(b) for b in (253, 256, 260, 300, 400) for _ in range(8)]
    a = arr([(x >> (32 * i)) & 0xFFFFFFFF for x in xs for i in range(16)], np.uint32)
    out = np.zeros(8 * len(xs), dtype=np.uint32)
    run(devsim.devsim_sc_reduce512, a, out, len(xs))
    assert [from_w(out[8 * i:8 * i + 8]) for i in range(len(xs))] == [x % L for x in xs]
    ys = [0, 1, L - 1, L, L + 1, 2**256 - 1, 2**252, 2**253, L - 2**32, L + 2**224] + [rng.getrandbits(b) for b in (252, 253, 256) for _ in range(30)]
    a = arr([w for y in ys for w in w8(y)], np.uint32)
    out = np.zeros(len(ys), dtype=np.uint32)
    run(devsim.devsim_sc_is_canonical, a, out, len(ys))
    assert ints(out) == [int(y < L) for y in ys]


def test_ed25519_decompress_compress(devsim):
    """dalek's decompression (y not checked for canonicity, x = 0 with the sign bit accepted) and the canonical re-encoding"""
    from oracle import ed25519_ref as ref
    Q = ref.P
    rng = random.Random(3)
    ys = [0, 1, 2, Q - 1, Q, Q + 1, Q + 2, 2**255 - 1, 2**255 - 19, 2**254, 4 * pow(5, Q - 2, Q) % Q]
    encs = [(y | (s << 255)).to_bytes(32, "little") for y in ys for s in (0, 1)]
    encs += [ref.compress(ref.pt_mul(rng.randrange(1, ref.L), ref.BASE)) for _ in range(40)]
    encs += [rng.getrandbits(256).to_bytes(32, "little") for _ in range(60)]
    a = arr(np.frombuffer(b"".join(encs), dtype=np.uint32), np.uint32)
    out, ok = np.zeros(8 * len(encs), dtype=np.uint32), np.zeros(len(encs), dtype=np.uint32)
    run(devsim.devsim_decompress_compress, a, out, ok, len(encs))
    want = [ref.decompress(e) for e in encs]
    assert ints(ok) == [int(p is not None) for p in want]
    assert 50 < sum(ints(ok)) < len(encs) - 10
    for i, p in enumerate(want):
        if p is not None:
            assert out[8 * i:8 * i + 8].tobytes() == ref.compress(p), i
