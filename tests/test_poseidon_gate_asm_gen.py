"""tools/gen_poseidon_gate_asm.py: the statement of the Poseidon gate's lazy partial block (csrc/poseidon_gate_asm.inc).  The
instruction list is executed by the generator's simulator against big-integer arithmetic round by round, on random, all-edge and
satisfying inputs; the flag-hazard and constant-bus rules are checked; the committed file is what the generator renders."""
import importlib.util
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gen():
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    spec = importlib.util.spec_from_file_location("gen_poseidon_gate_asm", os.path.join(tools, "gen_poseidon_gate_asm.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    return g


def test_gate_statement_selftest_and_committed_file_is_current():
    g = _gen()
    consts, tables = g.G.load_constants()
    assert g.selftest(consts, tables)
    text, (n_ins, n_nop) = g.render(consts, tables)      # compared in memory: the test never writes into csrc/
    assert open(g.INC_PATH).read() == text, "poseidon_gate_asm.inc is stale: run tools/gen_poseidon_gate_asm.py"
    # 11 S-boxes of 68, 297 products of 6 + 22 constants of 3 + 22 additions of 2, 22 folds of 16, 11 differences of 5 and the scalar
    # instructions of 80 table groups: ~3 300; a list far from that is not the statement this test was written for
    assert 3000 < n_ins < 3600 and n_nop < 100, (n_ins, n_nop)


def test_gate_statement_on_every_edge_value_at_every_wire():
    """one wire at a time through the edge alphabet (the others random), both blocks; and a block whose every difference is zero
    next to the same block with each of its eleven wires off by one"""
    g = _gen()
    consts, tables = g.G.load_constants()
    prog, _, _, _, n_groups = g.build_gate_partial_block(consts, 0)
    g.G.check_hazards(prog + prog)
    g.G.check_constant_bus(prog)
    rng = random.Random(31)
    for b in range(2):
        tab = tables["pblocks"][24 * n_groups * b:]
        s0, u = rng.randrange(g.P), [g.G.rnd64(rng) for _ in range(11)]
        for q in range(11):
            w = [rng.randrange(g.P) for _ in range(11)]
            w[q] = g.EDGE[(q + b) % len(g.EDGE)]
            assert g.run_block(prog, tab, s0, u, w) == g.block_reference(consts, b, s0, u, w), (b, q)
        sat = g.satisfying_wires(consts, b, s0, u)
        d, _ = g.run_block(prog, tab, s0, u, sat)
        assert d == [0] * 11
        for q in range(11):
            w = list(sat)
            w[q] = (w[q] + 1) % g.P
            d, out = g.run_block(prog, tab, s0, u, w)
            assert (d, out) == g.block_reference(consts, b, s0, u, w) and d[q] == g.P - 1, (b, q)
