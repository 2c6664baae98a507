"""The witness-generator instruction set (csrc/plonky2_witness_ops.h, csrc/wit25519.cuh) through the HOST interpreter
(zklc_plonky2_witness_run) against Python integers: tests/witops_vectors.py holds the programs, the references and the operand
sets.  One instruction per program, the tuples of a case as the witnesses of one call.  tests/test_gpu_witops.py runs the same table
through the device interpreter; this file puts the host build of the same header under the same references (the whole-circuit
tests compare device with host, so a mistake the two share is seen only here) and lets the table be debugged without a GPU."""
import ctypes

import numpy as np
import pytest

import witops_vectors as WV


def _lib():
    from zklc_amd import _lib
    return _lib.load()


def host_run(prog, vals, threads=8):
    """-> (public inputs [n, n_pi], wires [n, num_wires, n_rows], status [n], messages)"""
    vals = np.ascontiguousarray(vals, dtype=np.uint64).reshape(-1, max(1, len(prog["input_slots"])))
    n = vals.shape[0]
    npi = len(prog["pi_slots"])
    pis = np.zeros((n, max(npi, 1)), dtype=np.uint64)
    wires = np.zeros((n, prog["num_wires"], prog["n_rows"]), dtype=np.uint64)
    status = np.full(n, -1, dtype=np.int32)
    err = ctypes.create_string_buffer(200 * n)
    rc = _lib().zklc_plonky2_witness_run(
        prog["code"].ctypes.data, len(prog["code"]), prog["params"].ctypes.data, prog["n_slots"], prog["input_slots"].ctypes.data,
        len(prog["input_slots"]), vals.ctypes.data, n, prog["wire_slot"].ctypes.data, prog["wire_index"].ctypes.data,
        len(prog["wire_slot"]), prog["num_wires"], prog["n_rows"], wires.ctypes.data, prog["pi_slots"].ctypes.data, npi,
        pis.ctypes.data, status.ctypes.data, err, threads)
    assert rc == 0
    return pis[:, :npi], wires, status, [err.raw[200 * i:200 * i + 200].split(b"\0")[0].decode() for i in range(n)]


def check_case(c, pis, status, msgs):
    """every tuple of a case against its reference: outputs for the tuples that have them, the error text for the others"""
    for i, want in enumerate(c.want):
        where = "%s tuple %d %r" % (c.name, i, c.tuples[i] if c.n_in <= 24 else c.tuples[i][:24])
        if isinstance(want, int):
            assert status[i] != 0, where + ": expected '%s'" % WV.ERR_TEXT[want]
            assert msgs[i].startswith(WV.ERR_TEXT[want] + " at "), where + ": " + msgs[i]
        else:
            assert status[i] == 0, where + ": " + msgs[i]
            got = [int(x) for x in pis[i]]
            assert got == want, where + ": first difference at output %d" % next(k for k in range(len(want)) if got[k] != want[k])


@pytest.fixture(scope="module")
def table():
    from zklc_amd.plonky2.prover import poseidon_gate_rows
    cases = WV.table()
    print("coverage:", WV.assert_coverage(cases))            # asserted on the model before the library computes anything
    print("tuples per opcode:", WV.tuples_per_opcode(cases), "total", sum(len(c.tuples) for c in cases))
    WV.fill_poseidon(poseidon_gate_rows)
    return cases


def test_table_conditions_hold_on_the_model():
    """nothing compiled runs here: the counts the operand sets are built for, the model of Knuth's division on hand-made pairs, the
    decompression reference against the builder's Python generator, the model of the device's launch plan"""
    cov = WV.assert_coverage(WV.table())
    assert cov["error_codes"] == sorted([WV.WIT_ERR_SPLIT, WV.WIT_ERR_MULADD, WV.WIT_ERR_ADD_MANY, WV.WIT_ERR_SUB, WV.WIT_ERR_RANGE,
                                         WV.WIT_ERR_RANDOM_ACCESS, WV.WIT_ERR_INV_ZERO, WV.WIT_ERR_DIV_ZERO,
                                         WV.WIT_ERR_DECOMPRESS, WV.WIT_ERR_POSEIDON, WV.WIT_ERR_COSET_SHIFT, WV.WIT_ERR_INTERLEAVE])
    B = 2**32
    assert WV.divmod_model(5, 7) == (0, 5, {"lt"})
    assert WV.divmod_model(B**3 - 1, 3)[2] == {"one_limb"}
    assert "qhat_big" in WV.divmod_model((0x80000000 << 64) | 5, (0x80000000 << 32) | 7)[2]      # top limbs equal: qhat = 2^32
    # the decompression reference is the builder's generator: the copy in the table cannot drift from it
    from zklc_amd.plonky2 import ed25519_circuit as E
    for t in WV.by_name("decompress").tuples:
        val = int("".join(map(str, t)), 2)
        y, sign = val & (2**255 - 1), val >> 255
        try:
            x = E._recover_x(y % E.P25519, sign)
        except ValueError:
            x = None
        assert x == WV.recover_x(y % WV.P25519, sign)
    # the launch plan of the device, on made-up levels
    assert WV.plan_launches([[(1, False)] * 64, [(1, False)] * 10, [(1, False)] * 65, [(2, False), (15, True)]], 64) == \
        [("step", 2), ("light", 65), ("light", 1), ("heavy", 1)]
    assert WV.plan_launches([[(1, False)] * 3 + [(2, False)] * 2], 5) == [("step", 1)]
    assert WV.plan_launches([[(1, False)] * 500 + [(2, False)] * 9], 5) == [("light", 504 + 16)]


OPS = sorted({c.op for c in WV.table()})


@pytest.mark.parametrize("op", OPS, ids=[WV.OP_NAMES[o] for o in OPS])
def test_host_interpreter_equals_python_integers(table, op):
    """one instruction per program, every tuple of the case one witness; outputs read back as public inputs"""
    for c in table:
        if c.op != op:
            continue
        prog = WV.assemble([c.instr])
        pis, _, status, msgs = host_run(prog, c.tuples)
        check_case(c, pis, status, msgs)


def test_poseidon_rows_satisfy_the_oracle_gate(table):
    """the reference rows themselves: every constraint of the oracle's PoseidonGate is zero on them, so the equality above pins the
    interpreter to rows that the gate accepts and not only to the library's own host function"""
    from oracle.plonky2_gates import BaseK, PoseidonGate
    rows = WV.fill_poseidon(__import__("zklc_amd.plonky2.prover", fromlist=["x"]).poseidon_gate_rows)
    gate = PoseidonGate()
    for tup, row in rows:
        assert row[:12] == tup[:12] and row[24] == tup[12]
        res = gate.eval(BaseK, [], row, None)
        assert len(res) == gate.num_constraints and not any(res), tup


def test_outputs_as_wire_cells_and_a_program_of_many_instructions(table):
    """several instructions in one program, outputs scattered into the wire matrix; the cell of the slot nobody writes stays 0"""
    names = ["nn_mul_p25519_8x8_q8", "div_rem_16x8", "comparison_5x7", "u32_muladd", "split_base10_x20", "ext_inv", "poseidon"]
    cases = [WV.by_name(n) for n in names]
    n = 20
    picks = [c.good()[:n] for c in cases]
    assert all(len(p) == n for p in picks)
    prog = WV.assemble([c.instr for c in cases], outputs="wires")
    vals = [[x for c, p in zip(cases, picks) for x in c.tuples[p[w]]] for w in range(n)]
    _, wires, status, msgs = host_run(prog, vals)
    assert not status.any(), msgs
    assert len(prog["wire_slot"]) % 256 and prog["spare"] in prog["wire_slot"]
    for w in range(n):
        want = [x for c, p in zip(cases, picks) for x in c.want[p[w]]]
        flat = wires[w].reshape(-1)
        got = [int(flat[i]) for i in prog["wire_index"]]
        assert got[:len(want)] == want and not any(got[len(want):]), w
