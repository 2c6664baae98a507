#!/usr/bin/env python3
"""Generates csrc/poseidon_gate_asm.inc: the lazy partial block of the Poseidon GATE as a hand-scheduled gfx950 statement.

The gate (poseidon_gate.go:84-181) constrains every S-box input of the permutation to a wire, so inside a block of eleven fast
partial rounds nothing is a chain: z_q = wire_q^7 is known up front and the value round q leaves for the next S-box input is the
linear form  25 z_q + K_q + <u, w_q> + sum_{k<q} z_k c_q[k]  of the block's inputs (u = the state words 1..11 entering the
block).  The statement takes the eleven wires, the twelve words that enter the block and a table pointer, and returns
  * in place of the wires the eleven differences `computed - wire` (loose: the consumer multiplies 32-bit halves),
  * in place of the state the twelve words that leave the block (word 0 = the last linear form, words 1..11 materialised).
Scheduler, flag-pair pool, simulator, hazard and constant-bus checks are those of tools/gen_poseidon_asm.py, used as a library;
the multiply-accumulate slots are consumed in the order of the hash kernel's looped statement, so the table is PGL_ASM_PBLOCKS
(poseidon_gl_asm.inc) itself -- asserted here, nothing is duplicated.

Streams of one block: two S-box streams (even / odd q), the multiply-accumulate stream (filler: it carries no flags), two fold
streams (fold of three columns, then the difference); afterwards the materialisation in groups of four words as in the hash
kernel.  Every list is executed by the simulator against big-integer arithmetic (tests/test_poseidon_gate_asm_gen.py).
"""
import importlib.util
import os
import random
import sys


def _library():
    """a PRIVATE copy of tools/gen_poseidon_asm.py: tools/gen_gl_asm.py replaces functions of the copy in sys.modules (its own flag
    pairs start at s36), and a process that has loaded it must still render this file with the hash kernel's register convention"""
    spec = importlib.util.spec_from_file_location("gen_poseidon_asm_for_gate", os.path.join(os.path.dirname(os.path.abspath(__file__)), "gen_poseidon_asm.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _library()

P, M32 = G.P, G.M32
T, F, hi = G.T, G.F, G.hi
INC_PATH = os.path.join(G.ROOT, "zk-light-client-implementation_amd", "csrc", "poseidon_gate_asm.inc")
EDGE = [0, 1, P - 1, 2**32 - 1, 2**32, P - 2**32]

S0 = ("q0l", "q0h")
U = [("q%dl" % j, "q%dh" % j) for j in range(1, 12)]
W = [("w%dl" % q, "w%dh" % q) for q in range(11)]
OPERANDS = [r for x in W for r in x] + list(S0) + [r for x in U for r in x]


def diff(c, w, fl, fd):
    """w <- c - w for a loose c and a canonical w (loose result): a borrow means the wrapped value is eps too large, and
    x - eps b = (x.lo + b, x.hi - (b & ~carry)) as in reduce128; no second borrow (the wrapped value is > eps)"""
    x1 = G.xflag()
    return [
        ("sub_co", w[0], fl, c[0], w[0]),
        ("subb", w[1], fl, c[1], w[1], fl),
        ("addc", w[0], x1, w[0], 0, fl),
        ("sandn2", fl, fl, x1),
        ("subb", w[1], fd, w[1], 0, fl),
    ]


def build_gate_partial_block(cs, b):
    """-> (program, operands, nops, table, n_groups).  Temporaries: Z_k in T(0..21); phase 1 (linear forms): S-box streams
    T(22..31) / T(32..41), two accumulator sets T(42..53), fold scratch T(54..57); phase 2 (materialisation) as the hash
    kernel's: four accumulator sets T(22..45), fold scratch T(46..61)."""
    fd = F(0)
    Z = [(T(2 * k), T(2 * k + 1)) for k in range(11)]
    ACC = [(T(42), T(44), T(46)), (T(48), T(50), T(52))]
    B = cs["blocks"][b]
    sbox = [[], []]
    for q in range(11):
        sbox[q % 2] += G.sbox_stream(W[q], 22 + 10 * (q % 2), F(1 + q % 2), fd, out=Z[q]) + [("signal", "z%d" % q)]
    D = G.MacStream(fd)
    fold = [[("wait", "z0")] + diff(S0, W[0], F(3), fd), []]          # the word that enters is the first computed S-box input
    for q in range(11):
        acc, t = ACC[q % 2], q % 2
        if q >= 2:
            D.raw(("wait", "fold%d" % (q - 2)))
        D.const(acc, B["K"][q])
        for i in range(11):
            D.mac(acc, U[i], B["w"][q][i])
        for k in range(q):
            D.raw(("wait", "z%d" % k))
            D.mac(acc, Z[k], B["c"][q][k])
        D.raw(("wait", "z%d" % q), ("mad", acc[0], fd, Z[q][0], 25, acc[0]), ("mad", acc[1], fd, Z[q][1], G.S25K, acc[1]),
              ("signal", "dot%d" % q))
        TP = T(54 + 2 * t)
        out = S0 if q == 10 else (TP, hi(TP))
        fold[t] += [("wait", "dot%d" % q)] + G.fold3(acc, TP, None, out, F(3 + t), fd) + [("signal", "fold%d" % q)]
        if q < 10:
            fold[t] += [("wait", "z%d" % (q + 1))] + diff(out, W[q + 1], F(3 + t), fd)
    fold[0].append(("signal", "forms0"))
    fold[1].append(("signal", "forms1"))
    # the words 1..11 that leave the block: u_j += Kv_j + sum_k z_k v_k[j], four at a time
    accs = [(T(22 + 6 * t), T(24 + 6 * t), T(26 + 6 * t)) for t in range(4)]
    mfold = [[] for _ in range(4)]
    groups = [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10]]
    for g, js in enumerate(groups):
        D.raw(("wait", "forms0"), ("wait", "forms1"), *[("wait", "mf%d_%d" % (g - 1, t)) for t in range(len(groups[g - 1]) if g else 0)])
        for t, j in enumerate(js):
            D.const(accs[t], B["Kv"][j])
            D.raw(("mad", accs[t][0], fd, U[j][0], 1, accs[t][0]), ("mad", accs[t][1], fd, U[j][1], G.S10, accs[t][1]))
        for k in range(11):
            for t, j in enumerate(js):
                D.mac(accs[t], Z[k], B["v"][k][j])
        D.raw(("signal", "mat%d" % g))
        for t, j in enumerate(js):
            mfold[t] += [("wait", "mat%d" % g)] + G.fold3(accs[t], T(46 + 4 * t), None, U[j], F(1 + t), fd) + [("signal", "mf%d_%d" % (g, t))]
    n_groups = D.finish(even_groups=True)
    prog, nops = G.schedule(sbox + fold + mfold + [D.ins], G.STMT_PRE + G.prefetch0(), priority=True, pool=[F(5), F(6), F(7)])
    return prog, list(OPERANDS), nops, D.table, n_groups


# ------------------------------------------------------------------------------------------------------ self-test
def block_reference(consts, b, s0, u, w):
    """the eleven rounds of block b as poseidon_gate.go runs them (round by round, the S-box input replaced by the wire):
    -> (differences, words leaving the block) mod p"""
    cur = [s0 % P] + [x % P for x in u]
    d = []
    for q in range(11):
        rnd = 11 * b + q
        d.append((cur[0] - w[q]) % P)
        y = (pow(w[q], 7, P) + consts["fp_rc"][rnd]) % P
        nxt = (25 * y + sum(consts["w"][rnd][j - 1] * cur[j] for j in range(1, 12))) % P
        cur = [nxt] + [(cur[j] + y * consts["v"][rnd][j - 1]) % P for j in range(1, 12)]
    if b == 1:
        cur = [(x + c) % P for x, c in zip(cur, consts["rc26"])]
    return d, cur


def satisfying_wires(consts, b, s0, u):
    """the wires for which every difference of the block is zero"""
    cur = [s0 % P] + [x % P for x in u]
    w = []
    for q in range(11):
        rnd = 11 * b + q
        w.append(cur[0])
        y = (pow(cur[0], 7, P) + consts["fp_rc"][rnd]) % P
        nxt = (25 * y + sum(consts["w"][rnd][j - 1] * cur[j] for j in range(1, 12))) % P
        cur = [nxt] + [(cur[j] + y * consts["v"][rnd][j - 1]) % P for j in range(1, 12)]
    return w


def test_vectors(consts, b, rng, n_random=10):
    """(s0, u, wires): random, all-edge and satisfying inputs, and satisfying ones with one wire off by one"""
    vecs = []
    for _ in range(n_random):
        vecs.append((G.rnd64(rng), [G.rnd64(rng) for _ in range(11)], [rng.randrange(P) for _ in range(11)]))
    for e in EDGE:
        vecs.append((e, [e] * 11, [e] * 11))
    for i in range(6):
        vecs.append((rng.choice(EDGE), [rng.choice(EDGE + [2**64 - 1, P]) for _ in range(11)], [rng.choice(EDGE) for _ in range(11)]))
    for i in range(4):
        s0, u = rng.randrange(P), [rng.randrange(P) for _ in range(11)]
        w = satisfying_wires(consts, b, s0, u)
        vecs.append((s0, u, w))
        broken = list(w)
        broken[(3 * i + b) % 11] = (broken[(3 * i + b) % 11] + 1) % P
        vecs.append((s0, u, broken))
    return vecs


def run_block(prog, table, s0, u, w):
    regs = {}
    for pair, x in [(S0, s0)] + list(zip(U, u)) + list(zip(W, w)):
        regs[pair[0]], regs[pair[1]] = x & M32, x >> 32
    R = G.simulate(prog, regs, table)
    return [G.get64(R, p) % P for p in W], [G.get64(R, p) % P for p in [S0] + U]


def selftest(consts, tables):
    rng = random.Random(2025)
    built = [build_gate_partial_block(consts, b) for b in range(2)]
    assert built[0][0] == built[1][0], "the two blocks must share one instruction list"
    prog, n_groups = built[0][0], built[0][4]
    # slot for slot the table of the hash kernel's looped statement
    assert built[0][3] + built[1][3] + [0] * 24 == tables["pblocks"] and len(built[0][3]) == 24 * n_groups
    G.check_hazards(prog + prog)
    G.check_constant_bus(prog)
    for b in range(2):
        tab = tables["pblocks"][24 * n_groups * b:]
        for s0, u, w in test_vectors(consts, b, rng):
            got_d, got_s = run_block(prog, tab, s0, u, w)
            want_d, want_s = block_reference(consts, b, s0, u, w)
            assert got_d == want_d, "gate partial block %d: differences" % b
            assert got_s == want_s, "gate partial block %d: words leaving the block" % b
    return True


def render(consts=None, tables=None):
    """-> (text of csrc/poseidon_gate_asm.inc, (instructions, s_nop)); writes nothing"""
    if consts is None:
        consts, tables = G.load_constants()
    prog, ops, nops, _, n_groups = build_gate_partial_block(consts, 0)
    parts = ["// GENERATED by tools/gen_poseidon_gate_asm.py -- do not edit.  The lazy block of eleven fast partial rounds of the Poseidon GATE",
             "// (every S-box input is a wire) as one hand-scheduled gfx950 statement; see the generator for the derivation and the simulator",
             "// that checks the list.  Table: a block of PGL_ASM_PBLOCKS (poseidon_gl_asm.inc), PGL_GATE_BLOCK_DWORDS apart.",
             "// instructions %d (of which s_nop %d)" % (len(prog), nops),
             "#define PGL_GATE_BLOCK_DWORDS %d" % (24 * n_groups),
             "#if defined(__HIP_DEVICE_COMPILE__)",
             G.statement("pgl_gate_asm_partial_block", prog, ops, [], ptr=True,
                         comment="w: the block's eleven S-box-input wires -> computed - wire; q: the twelve words entering -> leaving the block"),
             "#endif"]
    return "\n".join(parts) + "\n", (len(prog), nops)


def main():
    consts, tables = G.load_constants()
    selftest(consts, tables)
    if "--check" in sys.argv:
        print("gen_poseidon_gate_asm: simulator self-test OK")
        return
    text, stats = render(consts, tables)
    if os.path.exists(INC_PATH) and open(INC_PATH).read() == text:
        print("poseidon_gate_asm.inc is current:", stats)
        return
    open(INC_PATH, "w").write(text)
    print("generated poseidon_gate_asm.inc:", stats)


if __name__ == "__main__":
    main()
