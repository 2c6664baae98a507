"""tools/gen_poseidon_tail_asm.py: the statement of the permutation's last full round with a four-row MDS layer
(csrc/poseidon_gl_tail_asm.inc).  The instruction list is executed by the generator's simulator in its three uses -- rows 0..3 with
the diagonal term, and the operand rotations by 8 and by 4 without it -- and compared with the MDS layer of oracle/poseidon_gl.py;
the flag-hazard and constant-bus rules are checked; the committed file is what the generator renders; the generator of the
permutation's other statements renders what it rendered before."""
import importlib.util
import os
import random
import sys

from oracle import poseidon_gl as PG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gen():
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    spec = importlib.util.spec_from_file_location("gen_poseidon_tail_asm", os.path.join(tools, "gen_poseidon_tail_asm.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    return g


def test_tail_statement_selftest_and_committed_file_is_current():
    g = _gen()
    assert g.selftest()
    text, (n_ins, n_nop) = g.render()                       # compared in memory: the test never writes into csrc/
    assert open(g.INC_PATH).read() == text, "poseidon_gl_tail_asm.inc is stale: run tools/gen_poseidon_tail_asm.py"
    # 12 S-boxes of 68 and four rows of 31-33: ~945; a list far from that is not the statement this test was written for
    assert 900 < n_ins < 1000 and n_nop < 20, (n_ins, n_nop)
    # the permutation's own generator is a library here and its file is untouched
    assert open(g.G.INC_PATH).read() == g.G.render()[0]


def test_tail_statement_three_uses_against_the_oracle_mds():
    g = _gen()
    prog, outs, ins_ops, _ = g.build_tail_round()
    assert len(outs) == 8 and len(ins_ops) == 17            # four 64-bit words in and out, eight in, and the diagonal multiplier
    g.G.check_hazards(prog + prog)
    g.G.check_constant_bus(prog)
    assert not any(i[0] in ("sload", "waitcnt") for i in prog)          # no table: the constants after the last round are zero
    assert [c for c in g.CASES] == [(0, 8), (8, 0), (4, 0)]
    rng = random.Random(5)
    for first, dg in g.CASES:
        for st in g.test_vectors(rng, n_random=12):
            want = PG.mds([PG.sbox(x % g.P) for x in st])[first:first + 4]
            assert g.run_tail(prog, st, first, dg) == want, (first, dg)
    # the diagonal term is the operand's doing: rows 0..3 with dg = 0 miss exactly 8 y[0] in row 0
    st = [rng.randrange(g.P) for _ in range(12)]
    full = PG.mds([PG.sbox(x) for x in st])
    got = g.run_tail(prog, st, 0, 0)
    assert got[1:] == full[1:4] and (got[0] + 8 * PG.sbox(st[0])) % g.P == full[0]
