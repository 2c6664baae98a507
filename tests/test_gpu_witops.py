"""The witness-generator instruction set ON THE DEVICE (csrc/plonky2_witness_dev.hip running `wit_exec` of
csrc/plonky2_witness_ops.h and the word arithmetic of csrc/wit25519.cuh) against Python integers, on constructed operands:
the table of tests/witops_vectors.py through zklc_plonky2_witness_program_create / zklc_plonky2_witness_run_dev.
tests/test_witops_host.py runs the same table through the host interpreter; tests/test_gpu_witness.py compares device and host on
three whole circuits with operands from real signatures, which never take the rare branches and cannot see a shared mistake.

Which kernel runs an instruction is decided by `wit_plan` (restated as WV.plan_launches, checked against
zklc_plonky2_witness_program_info before every run): with Wp = the power of two >= W lanes per instruction, a dependence level
without heavy instructions and of at most 4096 lanes is stepped through by ONE workgroup together with its small neighbours
(wit_levels_small_kernel); any other level is one launch of wit_level_kernel<false> for its light instructions and one of
wit_level_kernel<true> for its heavy ones (OP_DIV_REM, non-native ops over a modulus other than 2^255 - 19).  Every program below
is sized by that rule to reach the kernel it names.  Failures are return codes of the interpreter for operands inside the checked
domain of the ABI; nothing here goes outside it."""
import ctypes

import numpy as np
import pytest
import torch

import witops_vectors as WV

pytestmark = pytest.mark.gpu


class DevProgram:
    """plain ctypes over the three entry points: the status array and the messages are read as they are"""

    def __init__(self, ctx, prog):
        from zklc_amd import _lib
        self.ctx, self.prog, self.lib = ctx, prog, _lib.load()
        h = ctypes.c_void_p()
        ctx._check(self.lib.zklc_plonky2_witness_program_create(
            ctx._h, prog["code"].ctypes.data, len(prog["code"]), prog["params"].ctypes.data, len(prog["params"]), prog["n_slots"],
            prog["input_slots"].ctypes.data, len(prog["input_slots"]), prog["wire_slot"].ctypes.data, prog["wire_index"].ctypes.data,
            len(prog["wire_slot"]), prog["num_wires"], prog["n_rows"], prog["pi_slots"].ctypes.data, len(prog["pi_slots"]),
            ctypes.byref(h)))
        self.h = h

    def info(self, W):
        a, b, c = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32()
        self.ctx._check(self.lib.zklc_plonky2_witness_program_info(self.h, W, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return {"instructions": a.value, "levels": b.value, "launches": c.value}

    def run(self, vals):
        """-> (public inputs [W, n_pi], wires [W, num_wires, n_rows], status [W], messages)"""
        p = self.prog
        vals = np.ascontiguousarray(vals, dtype=np.uint64).reshape(-1, len(p["input_slots"]))
        W, npi = vals.shape[0], len(p["pi_slots"])
        assert 1 <= W <= 64
        d = torch.zeros((W, p["num_wires"], p["n_rows"]), dtype=torch.int64, device="cuda")
        pis = np.zeros((W, max(npi, 1)), dtype=np.uint64)
        status = np.full(W, -1, dtype=np.int32)
        err = ctypes.create_string_buffer(200 * W)
        torch.cuda.synchronize()
        self.ctx._check(self.lib.zklc_plonky2_witness_run_dev(self.ctx._h, self.ctx.stream_ptr(), self.h, vals.ctypes.data, W,
                                                              d.data_ptr(), pis.ctypes.data, status.ctypes.data, err))
        torch.cuda.synchronize()
        return pis[:, :npi], d.cpu().numpy().view(np.uint64), status, \
            [err.raw[200 * i:200 * i + 200].split(b"\0")[0].decode() for i in range(W)]

    def close(self):
        if self.h:
            self.lib.zklc_plonky2_witness_program_destroy(self.h)
            self.h = None


class CircuitStandIn:
    """what zklc_amd.plonky2.builder.DeviceWitness reads of a CircuitData"""

    def __init__(self, prog):
        self._program = dict(prog, input_targets=list(range(len(prog["input_slots"]))))
        self.config = {"num_wires": prog["num_wires"]}
        self.n = prog["n_rows"]
        self._container = None


@pytest.fixture(scope="module")
def table():
    from zklc_amd.plonky2.prover import poseidon_gate_rows
    cases = WV.table()
    print("coverage:", WV.assert_coverage(cases))            # asserted on the model before anything is launched
    WV.fill_poseidon(poseidon_gate_rows)
    return cases


def batched(cases, W, max_chunks=None, outputs="pi"):
    """one instruction per W good tuples of every case (the last chunk of a case is filled up from its first tuples) ->
    (program, input matrix [W, n_inputs], expected outputs per witness, [(opcode, heavy)] of the single level)"""
    instrs, picks = [], []
    for c in cases:
        g = c.good()
        assert g, c.name
        chunks = [g[k:k + W] for k in range(0, len(g), W)][:max_chunks]
        for ch in chunks:
            instrs.append(c)
            picks.append([ch[w] if w < len(ch) else g[(w - len(ch)) % len(g)] for w in range(W)])
    prog = WV.assemble([c.instr for c in instrs], outputs=outputs)
    vals = [[x for c, p in zip(instrs, picks) for x in c.tuples[p[w]]] for w in range(W)]
    want = [[x for c, p in zip(instrs, picks) for x in c.want[p[w]]] for w in range(W)]
    level = [(c.op, WV.is_heavy(c.op, c.params, c.n_in)) for c in instrs]
    return prog, vals, want, level


def first_difference(got, want):
    k = next(i for i in range(len(want)) if got[i] != want[i])
    return "output %d of the witness: got %d, want %d" % (k, got[k], want[k])


def run_and_compare(zctx, prog, vals, want, level, plan):
    W = len(vals)
    dp = DevProgram(zctx, prog)
    try:
        assert WV.plan_launches([level], W) == plan
        info = dp.info(W)
        assert info == {"instructions": len(level), "levels": 1, "launches": len(plan)}, info
        pis, wires, status, msgs = dp.run(vals)
        assert not status.any(), [m for m in msgs if m]
        for w in range(W):
            if len(prog["pi_slots"]):
                got = [int(x) for x in pis[w]]
            else:
                flat = wires[w].reshape(-1)
                got = [int(flat[i]) for i in prog["wire_index"]]
                assert not any(got[len(want[w]):]), "a cell of the slot nobody writes is not zero (witness %d)" % w
                got = got[:len(want[w])]
            assert got == want[w], "witness %d: %s" % (w, first_difference(got, want[w]))
    finally:
        dp.close()


def test_light_instructions_in_one_large_level(zctx, table):
    """wit_level_kernel<false>: every light case of the table, 64 tuples per instruction, W = 64: one level of far more than 4096
    lanes.  The 2^255 - 19 word arithmetic, point decompression, both inverse routes of the comparison, 64-bit % and / of OP_SPLIT,
    the device's own Poseidon rows, the extension and recursion gadgets."""
    light = [c for c in table if not WV.is_heavy(c.op, c.params, c.n_in) and c.good()]      # (poseidon_12_inputs: its own test)
    prog, vals, want, level = batched(light, 64)
    assert len(level) * 64 > 2 * WV.WIT_SMALL
    run_and_compare(zctx, prog, vals, want, level, [("light", len(level))])


def test_heavy_and_light_instructions_share_a_level(zctx, table):
    """wit_level_kernel<true>: OP_DIV_REM in eight limb shapes (Knuth's qhat correction, qhat >= 2^32 and add-back, by the model)
    and the non-native ops over L and 2^256 - 2^32 - 977 (generic `Big` code in scratch), in ONE level with light instructions: the
    level is split into a light and a heavy launch"""
    heavy = [c for c in table if WV.is_heavy(c.op, c.params, c.n_in)]
    light = [WV.by_name(n) for n in ("comparison_5x7_small_inverses", "u32_muladd", "nn_inv_p25519_8", "split_base7_x23")]
    assert {c.op for c in heavy} == {WV.OP_NN_ADD, WV.OP_NN_SUB, WV.OP_NN_MUL, WV.OP_NN_INV, WV.OP_DIV_REM}
    prog, vals, want, level = batched(light + heavy, 64)
    n_heavy = sum(h for _, h in level)
    run_and_compare(zctx, prog, vals, want, level, [("light", len(level) - n_heavy), ("heavy", n_heavy)])


@pytest.mark.parametrize("W", [5, 1])
def test_small_batches_and_the_wire_matrix(zctx, table, W):
    """W = 5 runs with Wp = 8 lanes per instruction: three idle lanes beside every instruction, opcode groups padded to wavefront
    boundaries; W = 1 has 64 instructions per wavefront.  Outputs go to the wire matrix: an entry count that is no multiple of the
    scatter kernel's tile of 256, and one cell mapped to a slot nobody writes, which stays zero."""
    names = ["nn_add_p25519_8x8", "nn_sub_p25519_8x8", "nn_mul_p25519_8x8_q9", "nn_mul_p25519_1x8_q1", "nn_inv_p25519_8", "decompress",
             "comparison_5x7_small_inverses", "comparison_1x32", "u32_muladd", "add_many_16", "sub_u32", "split_base10_x20",
             "split_base9223372036854775808_x2", "random_access_6", "exponentiation_64", "coset_interp_4_6", "reducing_43",
             "reducing_ext_32", "poseidon_mds", "poseidon", "uninterleave_b32_1", "is_equal", "ext_inv",
             "div_rem_16x8", "div_rem_16x3", "div_rem_39x20", "div_rem_16x1", "nn_mul_L_8x8_q8", "nn_inv_secp_8", "nn_add_secp_8x8"]
    prog, vals, want, level = batched([WV.by_name(n) for n in names], W, max_chunks=4, outputs="wires")
    assert len(prog["wire_slot"]) % 256 and len(prog["wire_slot"]) > 256 and prog["spare"] in prog["wire_slot"]
    plan = WV.plan_launches([level], W)
    assert [k for k, _ in plan] == ["light", "heavy"]
    run_and_compare(zctx, prog, vals, want, level, plan)


def chain_reference(t):
    ml = WV.limbs_of(WV.P25519, 8)
    r = WV.reference(WV.OP_NN_MUL, [8, 8] + ml, t, 16)
    iv = WV.reference(WV.OP_NN_INV, [8] + ml, r[:8], 16)
    r2 = WV.reference(WV.OP_NN_MUL, [8, 8] + ml, r[:8] + iv[:8], 16)
    assert r2[:8] == [1, 0, 0, 0, 0, 0, 0, 0]
    return r + iv + WV.reference(WV.OP_COMPARISON, [1, 32], [r[0], r[1]], 40) + WV.reference(WV.OP_U32_MULADD, [], r[:3], 35) + r2 + \
        WV.reference(WV.OP_IS_EQUAL, [], [r2[0], 1], 2) + WV.reference(WV.OP_IS_EQUAL, [], [r2[1], 1], 2)


@pytest.mark.parametrize("W", [64, 5])
def test_chain_of_levels_in_the_stepping_kernel(zctx, table, W):
    """wit_levels_small_kernel: four dependence levels of at most 4096 lanes inside one launch, values handed from level to level
    through the slot array (non-native product -> its inverse -> x x^-1 -> is_equal), through DeviceWitness with a stand-in for the
    circuit data.  The references are computed along the chain."""
    from zklc_amd.plonky2.builder import DeviceWitness
    c = WV.by_name("nn_mul_p25519_8x8_q8")
    usable = [t for t in c.tuples if (WV.value_of(t[:8]) % WV.P25519) * (WV.value_of(t[8:]) % WV.P25519) % WV.P25519]
    n_chains = 8
    assert len(usable) >= n_chains * W
    pr = WV.Program()
    ins = [pr.inputs(16) for _ in range(n_chains)]
    ml = WV.limbs_of(WV.P25519, 8)
    one = pr.emit(WV.OP_CONST, [1], [], 1)
    levels, pis = [[WV.OP_CONST], [], [], []], []
    for s in ins:
        r = pr.emit(WV.OP_NN_MUL, [8, 8] + ml, s, 16)
        iv = pr.emit(WV.OP_NN_INV, [8] + ml, r[:8], 16)
        cmp_ = pr.emit(WV.OP_COMPARISON, [1, 32], [r[0], r[1]], 40)
        mad = pr.emit(WV.OP_U32_MULADD, [], r[:3], 35)
        r2 = pr.emit(WV.OP_NN_MUL, [8, 8] + ml, r[:8] + iv[:8], 16)
        e0 = pr.emit(WV.OP_IS_EQUAL, [], [r2[0], one[0]], 2)
        e1 = pr.emit(WV.OP_IS_EQUAL, [], [r2[1], one[0]], 2)
        levels[0].append(WV.OP_NN_MUL)
        levels[1] += [WV.OP_NN_INV, WV.OP_COMPARISON, WV.OP_U32_MULADD]
        levels[2].append(WV.OP_NN_MUL)
        levels[3] += [WV.OP_IS_EQUAL, WV.OP_IS_EQUAL]
        pis += r + iv + cmp_ + mad + r2 + e0 + e1
    prog = pr.finish(pi_slots=pis)
    vals = [[x for k in range(n_chains) for x in usable[k * W + w]] for w in range(W)]
    want = [[x for k in range(n_chains) for x in chain_reference(usable[k * W + w])] for w in range(W)]
    assert WV.plan_launches([[(op, False) for op in lv] for lv in levels], W) == [("step", 4)]
    dw = DeviceWitness(zctx, CircuitStandIn(prog))
    try:
        assert dw.info(W) == {"instructions": 1 + 7 * n_chains, "levels": 4, "launches": 1}
        d = torch.zeros((W, 1, prog["n_rows"]), dtype=torch.int64, device="cuda")
        got = dw.run(d.data_ptr(), input_values=np.array(vals, dtype=np.uint64))
        torch.cuda.synchronize()
        for w in range(W):
            g = [int(x) for x in got[w]]
            assert g == want[w], "witness %d: %s" % (w, first_difference(g, want[w]))
    finally:
        dw.close()


def test_copy_classes(zctx):
    """two instructions write one slot (the compare-and-swap output path): equal values pass, different values give
    WIT_ERR_COPY to that witness only; a slot with a single writer takes the plain store"""
    import random
    rng = random.Random(5)
    pr = WV.Program()
    x, u = pr.inputs(3), pr.inputs(1)
    s = pr.emit(WV.OP_ARITH, [1, 0], x, 1)                   # x0 x1
    pr.emit(WV.OP_LE_SUM, [], u, out_slots=s)                # u, into the same slot
    t = pr.emit(WV.OP_ARITH, [1, 1], x, 1)                   # x0 x1 + x2: the only writer of its slot
    prog = pr.finish(pi_slots=s + t)
    W, bad = 64, 37
    xs = [[rng.choice(WV.DV.CANON), rng.randrange(WV.P), rng.randrange(WV.P)] for _ in range(W)]
    good = [v + [v[0] * v[1] % WV.P] for v in xs]
    vals = [list(v) for v in good]
    vals[bad][3] = (vals[bad][3] + 1) % WV.P
    dp = DevProgram(zctx, prog)
    try:
        assert dp.info(W) == {"instructions": 3, "levels": 1, "launches": 1}
        for batch, failing in ((vals, [bad]), (good, []), (vals[:5], []), (vals[33:38], [4])):
            pis, _, status, msgs = dp.run(batch)
            for w, v in enumerate(batch):
                if w in failing:
                    assert status[w] != 0 and msgs[w].startswith(WV.ERR_TEXT[WV.WIT_ERR_COPY] + " at scheduled instruction"), msgs[w]
                else:
                    assert status[w] == 0 and msgs[w] == "", (w, msgs[w])
                    assert [int(a) for a in pis[w]] == [v[0] * v[1] % WV.P, (v[0] * v[1] + v[2]) % WV.P], w
    finally:
        dp.close()


def test_poseidon_with_twelve_inputs_fails_for_every_witness(zctx, table):
    """the input count belongs to the instruction, so every witness of the batch fails, with the Poseidon text"""
    c = WV.by_name("poseidon_12_inputs")
    dp = DevProgram(zctx, WV.assemble([c.instr]))
    try:
        _, _, status, msgs = dp.run(c.tuples)
        assert status.all() and msgs == [WV.ERR_TEXT[WV.WIT_ERR_POSEIDON] + " at scheduled instruction 1"] * len(c.tuples), msgs
    finally:
        dp.close()


def failure_cases():
    """one (case, code) per opcode, kernel class and error code the table holds"""
    seen, out = set(), []
    for c in WV.table():
        for i in c.bad():
            key = (c.op, WV.is_heavy(c.op, c.params, c.n_in), c.want[i])
            if key not in seen and c.good():
                seen.add(key)
                out.append((c.name, i))
    return out


FAILURES = failure_cases()


@pytest.mark.parametrize("name,index", FAILURES, ids=["%s-%d" % f for f in FAILURES])
def test_one_failing_witness_among_good_ones(zctx, table, name, index):
    """every error code the table produces, as ONE failing witness in a batch of good ones of the same instruction: only its status
    is set, its message is the text of wit_strerror, the other witnesses' outputs are right, the next batch is clean"""
    c = WV.by_name(name)
    code, g = c.want[index], c.good()
    W = 13
    at = (index * 5 + 3) % W
    rows = [g[w % len(g)] for w in range(W)]
    prog = WV.assemble([c.instr])
    dp = DevProgram(zctx, prog)
    try:
        for failing in (True, False):
            sel = list(rows)
            if failing:
                sel[at] = index
            pis, _, status, msgs = dp.run([c.tuples[i] for i in sel])
            for w, i in enumerate(sel):
                if failing and w == at:
                    assert status[w] != 0, "expected '%s'" % WV.ERR_TEXT[code]
                    assert msgs[w] == WV.ERR_TEXT[code] + " at scheduled instruction 1", msgs[w]
                else:
                    assert status[w] == 0 and msgs[w] == "", (w, msgs[w])
                    assert [int(x) for x in pis[w]] == c.want[i], (w, c.tuples[i][:24])
    finally:
        dp.close()


def test_failures_cover_every_code_of_the_table(table):
    assert {WV.by_name(n).want[i] for n, i in FAILURES} == set(WV.assert_coverage(table)["error_codes"])
    assert len(FAILURES) <= 24
