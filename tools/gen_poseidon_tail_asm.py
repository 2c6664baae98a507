#!/usr/bin/env python3
"""Generates csrc/poseidon_gl_tail_asm.inc: the LAST full round of the Poseidon-Goldilocks permutation for a caller that reads
only four of the twelve words afterwards, as one hand-scheduled gfx950 statement.

The sponge overwrites the rate words s[0..7] with the next chunk (only the capacity words s[8..11] survive a permutation), a
digest is s[0..3], the proof of work reads s[7]: of the twelve rows of the last MDS layer at most four are ever read, and a row
is 31-33 instructions (`mds_row_stream` of tools/gen_poseidon_asm.py).  The statement runs the twelve S-boxes and then FOUR rows;
no constants follow the last round, so it fetches no table.

The MDS is circulant plus a diagonal term on word 0 only: out[r] = sum_i C[i] y[(i + r) % 12] (+ 8 y[0] for r = 0).  The
statement computes rows 0..3 OF ITS OPERANDS, out[r] = sum_i C[i] x[(i + r) % 12] + dg x[0] [r = 0], and returns them IN PLACE
of x[0..3] (the words a caller keeps are the very registers of its state: no moves around the statement; x is dead once the
twelve S-boxes have run, and the rows start after them).  A caller that binds x[j] = s[(j + FIRST) % 12] gets rows
FIRST..FIRST+3 of the state in s[FIRST..FIRST+3]: FIRST = 0 with dg = 8 (digest), FIRST = 8 (capacity words) and FIRST = 4 (proof
of work) with dg = 0.  The diagonal multiplier is an OPERAND (a VGPR holding 8 or 0), not a flag at generation
time: it costs two multiply-adds in row 0 and a v_mov, against a second copy of the whole statement (~7.5 KB of code) in the leaf
kernel, which needs both forms and has to stay inside the 64 KB instruction cache.

Scheduler, flag-pair pool, simulator, hazard and constant-bus checks are those of tools/gen_poseidon_asm.py, used as a library
(a private copy, as tools/gen_poseidon_gate_asm.py does); that file's render() and poseidon_gl_asm.inc are untouched.
Streams: three S-box streams of four words (results in temporaries, as in the full-round statement), then four row streams.
The list is executed by the simulator against big-integer arithmetic (tests/test_poseidon_tail_asm_gen.py).
"""
import importlib.util
import os
import random
import sys


def _library():
    spec = importlib.util.spec_from_file_location("gen_poseidon_asm_for_tail", os.path.join(os.path.dirname(os.path.abspath(__file__)), "gen_poseidon_asm.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _library()

P, M32 = G.P, G.M32
T, F, hi = G.T, G.F, G.hi
INC_PATH = os.path.join(G.ROOT, "zk-light-client-implementation_amd", "csrc", "poseidon_gl_tail_asm.inc")

XS = [("x%dl" % i, "x%dh" % i) for i in range(12)]
OUT = XS[:4]                 # the four rows replace the first four operands
DIAG = "dg"
# (FIRST, dg): the three uses; the caller's rotation is x[j] = s[(j + FIRST) % 12]
CASES = [(0, 8), (8, 0), (4, 0)]


def tail_row_stream(r, lo, hi_, out, base, fl, fd, diag=None):
    """row r of the MDS layer with no constant layer behind it: out = sum_i C[i] y[(i + r) % 12] (+ diag y[0] when given), loose.
    Two accumulator pairs per half as in mds_row_stream (two independent chains); diag <= 8 keeps the bounds of that function."""
    Al, Bl, Ah, Bh = T(base), T(base + 2), T(base + 4), T(base + 6)
    terms = [((i + r) % 12, G.MDS_C[i]) for i in range(12)]
    ins = []
    x1 = G.xflag()
    for k, (j, c) in enumerate(terms[:6]):
        ins.append(("mad", Al, fd, lo[j], c, Al if k else None))
        ins.append(("mad", Ah, fd, hi_[j], c, Ah if k else None))
    if diag is not None:
        ins.append(("mad", Al, fd, lo[0], diag, Al))
        ins.append(("mad", Ah, fd, hi_[0], diag, Ah))
    for k, (j, c) in enumerate(terms[6:]):
        ins.append(("mad", Bl, fd, lo[j], c, Bl if k else None))
        ins.append(("mad", Bh, fd, hi_[j], c, Bh if k else None))
    ins += [
        ("add64", Al, Al, Bl),                         # sl < 2^42
        ("add64", Ah, Ah, Bh),                         # sh < 2^42; value = sl + sh 2^32
        ("mad", Al, fd, hi(Ah), -1, Al),               # sh.hi 2^64 = sh.hi eps: no carry (both < 2^42)
        ("add_co", hi(Al), fl, hi(Al), Ah),            # + sh.lo 2^32, carry c: + eps (as in reduce128)
        ("subb", out[0], x1, Al, 0, fl),
        ("sandn2", fl, fl, x1),
        ("addc", out[1], fd, hi(Al), 0, fl),
    ]
    return ins


def build_tail_round():
    """-> (program, in-out operands, input operands, nops).  Temporaries: the S-box results Y in T(0..23); the S-box streams use T(24..59) as in the
    full-round statement; the four row streams, which start when every S-box is done, eight of those registers each."""
    fd = F(0)
    Y = [(T(2 * i), T(2 * i + 1)) for i in range(12)]
    streams = []
    for k in range(3):
        st = []
        for i in range(k, 12, 3):
            st += G.sbox_stream(XS[i], 24 + 12 * k, F(1 + k), fd, out=Y[i])
            st.append(("signal", "sb%d" % i))
        streams.append(st)
    lo, hi_ = [y[0] for y in Y], [y[1] for y in Y]
    for r in range(4):
        st = [("wait", "sb%d" % i) for i in range(12)]
        st += tail_row_stream(r, lo, hi_, OUT[r], 24 + 8 * r, F(1 + r), fd, diag=DIAG if r == 0 else None)
        streams.append(st)
    prog, nops = G.schedule(streams, [], pool=[F(5), F(6), F(7)])
    return prog, [r for o in OUT for r in o], [r for x in XS[4:] for r in x] + [DIAG], nops


# ------------------------------------------------------------------------------------------------------ self-test
def mds_rows(y, first):
    """rows first..first+3 of the MDS layer of the twelve words y, mod p (the definition; the tests compare it with oracle/poseidon_gl.py)"""
    return [(sum(G.MDS_C[i] * y[(i + r) % 12] for i in range(12)) + (8 * y[0] if r == 0 else 0)) % P for r in range(first, first + 4)]


def run_tail(prog, state, first, dg):
    """the statement on the state `state` (twelve loose 64-bit words) bound with the rotation `first` -> the four outputs mod p"""
    regs = {DIAG: dg}
    for j in range(12):
        x = state[(j + first) % 12]
        regs[XS[j][0]], regs[XS[j][1]] = x & M32, x >> 32
    R = G.simulate(prog, regs)
    return [G.get64(R, o) % P for o in OUT]


def test_vectors(rng, n_random=20):
    edge = [0, 1, P - 1, P, 2**32 - 1, 2**32, 2**64 - 1]
    vecs = [[G.rnd64(rng) for _ in range(12)] for _ in range(n_random)]
    vecs += [[e] * 12 for e in edge]
    vecs += [[rng.choice(edge) for _ in range(12)] for _ in range(8)]
    return vecs


def selftest():
    rng = random.Random(2026)
    prog, outs, ins_ops, _ = build_tail_round()
    assert len(outs) == 8 and len(ins_ops) == 17
    # in place: nothing reads an operand once the first row has been written
    first_write = min(k for k, i in enumerate(prog) if i[0] in ("subb", "addc") and i[1] in outs)
    assert not any(isinstance(x, str) and x[0] == "x" for i in prog[first_write:] for x in i[3:]), "an operand is read after a row was written"
    G.check_hazards(prog + prog)
    G.check_constant_bus(prog)
    for first, dg in CASES:
        for st in test_vectors(rng):
            want = mds_rows([pow(x, 7, P) for x in st], first)
            assert run_tail(prog, st, first, dg) == want, "tail round, rows %d..%d" % (first, first + 3)
    return True


def render():
    """-> (text of csrc/poseidon_gl_tail_asm.inc, (instructions, s_nop)); writes nothing"""
    prog, outs, ins_ops, nops = build_tail_round()
    parts = ["// GENERATED by tools/gen_poseidon_tail_asm.py -- do not edit.  The last full round of the Poseidon-Goldilocks permutation for a",
             "// caller that reads four words afterwards: twelve S-boxes, FOUR rows of the MDS layer, no constants (none follow the last round).",
             "// x[r] <- sum_i C[i] x[(i + r) % 12]^7 + dg x[0]^7 [r = 0], r < 4: bind x[j] = s[(j + FIRST) % 12] for rows FIRST..FIRST+3 of the state,",
             "// dg = 8 for FIRST = 0 and 0 otherwise (the diagonal of the MDS matrix is (8, 0, ..., 0)).  See the generator.",
             "// instructions %d (of which s_nop %d)" % (len(prog), nops),
             "#if defined(__HIP_DEVICE_COMPILE__)",
             G.statement("pgl_asm_tail_round", prog, outs, ins_ops,
                         comment="x: the twelve words entering the last full round, rotated by the caller; x0..x3 <- rows 0..3 of the MDS layer (loose); dg: 8 or 0"),
             "#endif"]
    return "\n".join(parts) + "\n", (len(prog), nops)


def main():
    selftest()
    if "--check" in sys.argv:
        print("gen_poseidon_tail_asm: simulator self-test OK")
        return
    text, stats = render()
    if os.path.exists(INC_PATH) and open(INC_PATH).read() == text:
        print("poseidon_gl_tail_asm.inc is current:", stats)
        return
    open(INC_PATH, "w").write(text)
    print("generated poseidon_gl_tail_asm.inc:", stats)


if __name__ == "__main__":
    main()
