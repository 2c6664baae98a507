"""Programs, Python-integer references and operand sets for the witness-generator instruction set (csrc/plonky2_witness_ops.h:
`wit_exec`, the `Big` limb integers, `g_inv` / `g_inv_small`, and the 2^255 - 19 word arithmetic of csrc/wit25519.cuh).

tests/test_witops_host.py runs the table through the host interpreter (zklc_plonky2_witness_run), tests/test_gpu_witops.py through
the device interpreter (zklc_plonky2_witness_program_create / _run_dev).  Nothing here imports the library or needs a GPU.

Layout of a run: ONE INSTRUCTION PER OPERAND SHAPE, the W witnesses of a batch are W operand tuples of that instruction, and the
outputs come back as public inputs or as wire cells.  The references are written from the semantics stated in the comments of
plonky2_witness_ops.h (one instruction = one generator of the reference), on Python integers; they return the output list or the
WIT_ERR_* code the instruction must report.  `divmod_model` restates Knuth's algorithm D on 32-bit limbs only to say WHICH branch
an operand pair takes (qhat correction, qhat >= 2^32, add-back): random operands never reach the add-back, the sets construct it."""
import functools
import random

import numpy as np

import devsim_vectors as DV

P = DV.P
W7 = 7                                        # the quadratic extension is GF(p)[X] / (X^2 - 7)
P25519 = 2**255 - 19
L25519 = 2**252 + 27742317777372353535851937790883648493
SECP = 2**256 - 2**32 - 977
D25519 = (-121665 * pow(121666, P25519 - 2, P25519)) % P25519
BASE_Y = 4 * pow(5, P25519 - 2, P25519) % P25519
B32 = 2**32

(OP_CONST, OP_ARITH, OP_SPLIT, OP_LE_SUM, OP_U32_MULADD, OP_ADD_MANY, OP_SUB_U32, OP_RANGE_CHECK, OP_COMPARISON, OP_IS_EQUAL,
 OP_RANDOM_ACCESS, OP_NN_ADD, OP_NN_SUB, OP_NN_MUL, OP_NN_INV, OP_DIV_REM, OP_DECOMPRESS, OP_POSEIDON, OP_EXT_ARITH, OP_EXT_MUL,
 OP_EXT_INV, OP_EXPONENTIATION, OP_COSET_INTERP, OP_POSEIDON_MDS, OP_REDUCING, OP_REDUCING_EXT, OP_INTERLEAVE,
 OP_UNINTERLEAVE) = range(28)
OP_NAMES = ["CONST", "ARITH", "SPLIT", "LE_SUM", "U32_MULADD", "ADD_MANY", "SUB_U32", "RANGE_CHECK", "COMPARISON", "IS_EQUAL",
            "RANDOM_ACCESS", "NN_ADD", "NN_SUB", "NN_MUL", "NN_INV", "DIV_REM", "DECOMPRESS", "POSEIDON", "EXT_ARITH", "EXT_MUL",
            "EXT_INV", "EXPONENTIATION", "COSET_INTERP", "POSEIDON_MDS", "REDUCING", "REDUCING_EXT", "INTERLEAVE", "UNINTERLEAVE"]

(WIT_OK, WIT_ERR_COPY, WIT_ERR_INPUT_NA, WIT_ERR_SPLIT, WIT_ERR_MULADD, WIT_ERR_ADD_MANY, WIT_ERR_SUB, WIT_ERR_RANGE,
 WIT_ERR_COMPARISON, WIT_ERR_RANDOM_ACCESS, WIT_ERR_INV_ZERO, WIT_ERR_DIV_ZERO, WIT_ERR_DECOMPRESS, WIT_ERR_POSEIDON,
 WIT_ERR_COSET_ARITY, WIT_ERR_COSET_SHIFT, WIT_ERR_REDUCING, WIT_ERR_INTERLEAVE, WIT_ERR_OPCODE, WIT_ERR_OUT_COUNT, WIT_ERR_PI,
 WIT_ERR_NEEDS_HEAVY) = range(22)
# the texts of wit_strerror, by code
ERR_TEXT = ["ok", "copy constraint violated", "input not available", "split: value does not fit", "u32 mul-add overflows the field",
            "add-many carry does not fit", "u32 subtraction out of range", "range check: value exceeds 32 bits",
            "comparison: most significant difference out of range", "random access: index out of range", "inverse of zero",
            "division by zero", "point decompression: not a curve point", "poseidon: 12 inputs and a boolean swap expected",
            "coset interpolation: bad arity", "coset interpolation: zero shift", "reducing: bad arity",
            "interleave: value exceeds 32 bits", "unknown opcode", "output count mismatch", "public input was never assigned",
            "instruction scheduled into the wrong kernel class"]


def limbs_of(v, n):
    """the low n 32-bit limbs, little-endian"""
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def value_of(limbs):
    return sum(int(x) << (32 * i) for i, x in enumerate(limbs))


# ------------------------------------------------------------------------------------------------ program assembler
class Program:
    """A witness program in the encoding of include/zklc.h (above zklc_plonky2_witness_run): code = [opcode, n_params, n_in, n_out,
    input slots.., output slots..]* as u32 words, the parameters of all instructions consecutive in `params` (i64: field elements
    above 2^63 wrap), a slot = one value per witness."""

    def __init__(self):
        self.code, self.params, self.input_slots, self.outs = [], [], [], []
        self.n_slots = 0

    def slots(self, n):
        r = list(range(self.n_slots, self.n_slots + n))
        self.n_slots += n
        return r

    def inputs(self, n):
        s = self.slots(n)
        self.input_slots += s
        return s

    def emit(self, op, params, in_slots, n_out=None, out_slots=None):
        outs = self.slots(n_out) if out_slots is None else list(out_slots)
        self.code += [op, len(params), len(in_slots), len(outs)] + list(in_slots) + outs
        self.params += [int(x) for x in params]
        self.outs.append(outs)
        return outs

    def finish(self, pi_slots=(), wire_slots=(), n_rows=8):
        """-> the arguments of the two entry points.  pi_slots: slots read back as public inputs.  wire_slots: slots read back as
        wire cells; cell k of the list goes to the wire matrix at a column-major index that is a permutation of 0..n-1 (7 k mod n
        for n coprime to 7), so the scatter is not the identity.  n_slots counts one spare slot nobody writes: `spare`."""
        spare = self.n_slots
        ws = list(wire_slots)
        n = len(ws)
        while n and n % 7 == 0:
            ws.append(spare)                  # keeps 7 k mod n a permutation; the cell stays zero
            n += 1
        return {"code": np.array(self.code, dtype=np.uint32),
                "params": np.array([x - 2**64 if x >= 2**63 else x for x in self.params] + [0], dtype=np.int64),
                "n_slots": self.n_slots + 1, "spare": spare, "input_slots": np.array(self.input_slots, dtype=np.uint32),
                "pi_slots": np.array(list(pi_slots), dtype=np.uint32), "wire_slot": np.array(ws, dtype=np.uint32),
                "wire_index": np.array([7 * k % n for k in range(n)], dtype=np.uint32),
                "num_wires": max(1, -(-n // n_rows)), "n_rows": n_rows, "outs": self.outs}


def assemble(instrs, outputs="pi"):
    """instrs: [(opcode, params, n_in, n_out)], every instruction on fresh input slots (a witness's input vector = the inputs of the
    instructions in order) and fresh output slots.  outputs = "pi": every output is a public input, in order; "wires": every output
    is a wire cell (Program.finish), plus one cell mapped to the spare slot, which must stay zero."""
    pr = Program()
    outs = []
    for op, params, n_in, n_out in instrs:
        outs += pr.emit(op, params, pr.inputs(n_in), n_out)
    if outputs == "pi":
        return pr.finish(pi_slots=outs)
    return pr.finish(wire_slots=outs + [pr.n_slots])


# ------------------------------------------------------------------------------------------------ Goldilocks helpers
def e_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def e_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def e_mul(a, b):
    return ((a[0] * b[0] + W7 * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def e_scalar(c, a):
    return (c * a[0] % P, c * a[1] % P)


def inv(x):
    return pow(x % P, P - 2, P)


def root_of_unity(bits):
    return pow(1753635133440165772, 1 << (32 - bits), P)      # plonky2's generator of the 2^32-subgroup


def barycentric_weights(bits):
    pts = [pow(root_of_unity(bits), i, P) for i in range(1 << bits)]
    out = []
    for i, x in enumerate(pts):
        d = 1
        for j, y in enumerate(pts):
            if i != j:
                d = d * (x - y) % P
        out.append(inv(d))
    return out


MDS_CIRC = [17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20]
MDS_DIAG = [8] + [0] * 11


def two_bit_limbs(v, n):
    return [(v >> (2 * j)) & 3 for j in range(n)]


def recover_x(y, sign):
    """zklc_amd/plonky2/ed25519_circuit.py `_recover_x`, the builder's generator of the point decompression"""
    xx = (y * y - 1) * pow(D25519 * y * y + 1, P25519 - 2, P25519) % P25519
    x = pow(xx, (P25519 + 3) // 8, P25519)
    if (x * x - xx) % P25519:
        x = x * pow(2, (P25519 - 1) // 4, P25519) % P25519
    if (x * x - xx) % P25519:
        return None
    if (x & 1) != sign:
        x = (P25519 - x) % P25519
    return x


# ------------------------------------------------------------------------------------------------ references, one per opcode
def reference(op, pr, v, n_out):
    """the outputs of one instruction on Python integers (all mod p), or the WIT_ERR_* code it must report.
    pr: parameters (field elements as non-negative integers), v: input values (canonical field elements)"""
    if op == OP_CONST:
        return [pr[0] % P]
    if op == OP_ARITH:
        return [(pr[0] * v[0] * v[1] + pr[1] * v[2]) % P]
    if op == OP_SPLIT:
        base, x, out = pr[0], v[0], []
        for _ in range(pr[1]):
            out.append(x % base)
            x //= base
        return WIT_ERR_SPLIT if x else out
    if op == OP_LE_SUM:
        return [sum(x << i for i, x in enumerate(v)) % P]
    if op == OP_U32_MULADD:
        t = v[0] * v[1] + v[2]
        if t >= P:
            return WIT_ERR_MULADD
        lo, hi = t & 0xFFFFFFFF, t >> 32
        d = (0xFFFFFFFF - hi) % P
        return [lo, hi, inv(d) if d else 0] + two_bit_limbs(t, 32)
    if op == OP_ADD_MANY:
        s = sum(v)
        lo, hi = s & 0xFFFFFFFF, s >> 32
        if hi >= 16:
            return WIT_ERR_ADD_MANY
        return [lo, hi] + two_bit_limbs(lo, 16) + two_bit_limbs(hi, 2)
    if op == OP_SUB_U32:
        d = v[0] - v[1] - v[2]
        bout = 1 if d < 0 else 0
        res = d + (bout << 32)
        if not 0 <= res < B32:
            return WIT_ERR_SUB
        return [res, bout] + two_bit_limbs(res, 16)
    if op == OP_RANGE_CHECK:
        out = []
        for x in v:
            if x >> 32:
                return WIT_ERR_RANGE
            out += two_bit_limbs(x, 16)
        return out
    if op == OP_COMPARISON:
        nc, cb = pr
        size, msd, out = 1 << cb, 0, []
        for i in range(nc):
            ca, cy = (v[0] >> (cb * i)) & (size - 1), (v[1] >> (cb * i)) & (size - 1)
            eq = 1 if ca == cy else 0
            inter = msd if eq else 0
            out += [ca, cy, 1 if eq else inv(cy - ca), eq, inter]
            if not eq:
                msd = (cy - ca) % P
        top = (size + msd) % P
        if top >= 2 * size:
            return WIT_ERR_COMPARISON
        return out + [msd] + [(top >> i) & 1 for i in range(cb + 1)] + [(top >> cb) & 1]
    if op == OP_IS_EQUAL:
        return [1, 0] if v[0] == v[1] else [0, inv(v[0] - v[1])]
    if op == OP_RANDOM_ACCESS:
        if v[0] >> pr[0]:
            return WIT_ERR_RANDOM_ACCESS
        return [v[1 + v[0]]] + [(v[0] >> i) & 1 for i in range(pr[0])]
    if op in (OP_NN_ADD, OP_NN_SUB):
        na, m = pr[0], value_of(pr[1:9])
        a, b = value_of(v[:na]) % m, value_of(v[na:]) % m
        if op == OP_NN_ADD:
            ov = 1 if a + b > m else 0                      # strictly greater: a + b == m stays unreduced
            return limbs_of(a + b - ov * m, 8) + [ov]
        return limbs_of((a - b) % m, 8) + [1 if a < b else 0]
    if op == OP_NN_MUL:
        na, nover, m = pr[0], pr[1], value_of(pr[2:10])
        q, r = divmod((value_of(v[:na]) % m) * (value_of(v[na:]) % m), m)
        return limbs_of(r, 8) + limbs_of(q, nover)
    if op == OP_NN_INV:
        n, m = pr[0], value_of(pr[1:9])
        x = value_of(v) % m
        if x == 0:
            return WIT_ERR_INV_ZERO
        iv = pow(x, m - 2, m)
        return limbs_of(iv, n) + limbs_of((x * iv - 1) // m, n)
    if op == OP_DIV_REM:
        a_len, n_div, n_rem = pr
        a, b = value_of(v[:a_len]), value_of(v[a_len:])
        if b == 0:
            return WIT_ERR_DIV_ZERO
        return limbs_of(a // b, n_div) + limbs_of(a % b, n_rem)
    if op == OP_DECOMPRESS:
        val = 0
        for bit in v:
            val = (val << 1) | bit
        sign, y = val >> 255, val & (2**255 - 1)
        # the header leaves two cases open; both are what the builder's generator (plonky2/ed25519_circuit.py point_decompress)
        # returns (tests/test_witops_host.py compares `recover_x` with that generator on every tuple): y = 1 with the sign bit
        # set has x = 0, whose negation is 0 -- the canonical value, as curve25519-dalek's conditional negation gives it, so the
        # compression check of the circuit then rejects the encoding; and for y >= p the square root is taken of y mod p while
        # the y output is the UNREDUCED 255-bit string
        x = recover_x(y % P25519, sign)
        if x is None:
            return WIT_ERR_DECOMPRESS
        return limbs_of(x, 8) + limbs_of(y, 8)
    if op == OP_EXT_ARITH:
        return list(e_add(e_scalar(pr[0], e_mul(v[0:2], v[2:4])), e_scalar(pr[1], v[4:6])))
    if op == OP_EXT_MUL:
        return list(e_scalar(pr[0], e_mul(v[0:2], v[2:4])))
    if op == OP_EXT_INV:
        if v[0] == 0 and v[1] == 0:
            return WIT_ERR_INV_ZERO
        d = inv(v[0] * v[0] - W7 * v[1] * v[1])
        return [v[0] * d % P, (-v[1]) * d % P]
    if op == OP_EXPONENTIATION:
        n, cur, out = len(v) - 1, 1, []
        for i in range(n):                                   # most significant bit first
            cur = (1 if i == 0 else cur * cur) * (v[0] if v[n - i] else 1) % P
            out.append(cur)
        return out + [cur]
    if op == OP_COSET_INTERP:
        sb, d, wts = pr[0], pr[1], pr[2:]
        npts = 1 << sb
        if len(v) != 1 + 2 * npts + 2 or len(wts) != npts:
            return WIT_ERR_COSET_ARITY
        if v[0] == 0:
            return WIT_ERR_COSET_SHIFT
        dom = [pow(root_of_unity(sb), i, P) for i in range(npts)]
        vals = [(v[1 + 2 * i], v[2 + 2 * i]) for i in range(npts)]
        shifted = e_scalar(inv(v[0]), (v[1 + 2 * npts], v[2 + 2 * npts]))
        ev, prod = (0, 0), (1, 0)
        out = list(shifted)
        # the partial evaluations after the first d points, then after every further d - 1
        bounds = [d] + [min(1 + (d - 1) * (i + 2), npts) for i in range((npts - 2) // (d - 1))]
        at = 0
        for k, end in enumerate(bounds):
            for i in range(at, end):
                term = e_sub(shifted, (dom[i], 0))
                ev = e_add(e_mul(ev, term), e_mul(e_scalar(wts[i], vals[i]), prod))
                prod = e_mul(prod, term)
            at = end
            out += list(ev) + (list(prod) if k < len(bounds) - 1 else [])
        return out
    if op == OP_POSEIDON_MDS:
        out = []
        for r in range(12):
            for c in range(2):
                out.append((sum(MDS_CIRC[i] * v[2 * ((i + r) % 12) + c] for i in range(12)) + MDS_DIAG[r] * v[2 * r + c]) % P)
        return out
    if op in (OP_REDUCING, OP_REDUCING_EXT):
        n, ext = pr[0], op == OP_REDUCING_EXT
        if len(v) != 4 + (2 * n if ext else n):
            return WIT_ERR_REDUCING
        alpha, acc, out = v[0:2], v[2:4], []
        for i in range(n):
            c = (v[4 + 2 * i], v[5 + 2 * i]) if ext else (v[4 + i], 0)
            acc = e_add(e_mul(acc, alpha), c)
            out += list(acc)
        return out
    if op == OP_INTERLEAVE:
        x = v[0]
        if x >> 32:
            return WIT_ERR_INTERLEAVE
        return [sum(((x >> j) & 1) << (2 * j) for j in range(32))] + [(x >> (31 - j)) & 1 for j in range(32)]
    if op == OP_UNINTERLEAVE:
        step, x = (2 if pr[0] else 1), v[0]
        return [sum(((x >> (2 * j + 1)) & 1) << (step * j) for j in range(32)) % P,
                sum(((x >> (2 * j)) & 1) << (step * j) for j in range(32)) % P] + [(x >> (63 - j)) & 1 for j in range(64)]
    raise ValueError("no reference for opcode %d" % op)


# ------------------------------------------------------------------------------------------------ Knuth D, branch by branch
DIV_BRANCHES = ("lt", "one_limb", "qhat_corr", "qhat_big", "add_back")


def divmod_model(a, b):
    """Knuth's algorithm D on 32-bit limbs (TAOCP 4.3.1) -> (q, r, branches taken): "lt" dividend < divisor, "one_limb" short
    division, "qhat_big" the estimate is >= 2^32, "qhat_corr" the estimate fails the two-limb test and is decreased, "add_back"
    the multiply-subtract goes negative (step D6)"""
    assert b
    if a < b:
        return 0, a, {"lt"}
    n = -(-b.bit_length() // 32)
    if n == 1:
        return a // b, a % b, {"one_limb"}
    na = -(-a.bit_length() // 32)
    m = na - n
    s = 32 * n - b.bit_length()
    vn, un = limbs_of(b << s, n), limbs_of(a << s, na + 1)
    vv = value_of(vn)
    taken, q = set(), 0
    for j in range(m, -1, -1):
        qhat, rhat = divmod(un[j + n] * B32 + un[j + n - 1], vn[n - 1])
        while qhat >= B32 or qhat * vn[n - 2] > rhat * B32 + un[j + n - 2]:
            taken.add("qhat_big" if qhat >= B32 else "qhat_corr")
            qhat -= 1
            rhat += vn[n - 1]
            if rhat >= B32:
                break
        t = value_of(un[j:j + n + 1]) - qhat * vv
        if t < 0:
            taken.add("add_back")
            qhat -= 1
            t += vv
        assert 0 <= t < vv
        un[j:j + n + 1] = limbs_of(t, n + 1)
        q |= qhat << (32 * j)
    r = value_of(un[:n]) >> s
    assert (q, r) == divmod(a, b), "the model of Knuth's algorithm D disagrees with divmod"
    return q, r, taken


# ------------------------------------------------------------------------------------------------ operand sets
ALPHA32 = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF]


def structured(rng, n):
    """n limbs drawn from the edge alphabet"""
    return value_of([rng.choice(ALPHA32) for _ in range(n)])


def nn_edges(m, n=8):
    """the edge operands of a non-native op over modulus m, as values below 2^(32 n)"""
    e = [0, 1, 2, 18, 19, 20, 37, 38, 39, m - 2, m - 1, m, m + 1, m + 18, m + 19, 2**255 - 1, 2**255, 2**256 - 39, 2**256 - 38,
         2**256 - 1, (m - 1) // 2, (m + 1) // 2]
    return sorted({x for x in e if 0 <= x < 2**(32 * n)})


def nn_pairs(rng, m, na, nb, n_mixed, full_edges):
    ea, eb = nn_edges(m, na), nn_edges(m, nb)
    pool_a = ea + [structured(rng, na) for _ in range(24)] + [rng.randrange(2**(32 * na)) for _ in range(24)]
    pool_b = eb + [structured(rng, nb) for _ in range(24)] + [rng.randrange(2**(32 * nb)) for _ in range(24)]
    pairs = [(a, b) for a in ea for b in eb] if full_edges else [(rng.choice(ea), rng.choice(eb)) for _ in range(64)]
    pairs += [(rng.choice(pool_a), rng.choice(pool_b)) for _ in range(n_mixed)]
    lim_a, lim_b = 2**(32 * na), 2**(32 * nb)
    for k in range(24):                                      # a + b in {m - 1, m, m + 1}, also with an unreduced a
        a = rng.choice(pool_a) % m
        for t in (m - 1, m, m + 1):
            b = t - a
            if 0 <= b < lim_b and a < lim_a:
                pairs.append((a + m if k % 4 == 3 and a + m < lim_a else a, b))
    if na == nb == 8:
        # a b = q m + k with a small k: for m = 2^255 - 19 the remainder candidate of w25519_divmod after its two folds is >= p
        # (its conditional subtraction runs) iff k < 19 (q - (a b >> 255)), a window of at most a few hundred values
        for k in range(96):
            a = rng.randrange(1, m)
            pairs.append((a, (0, 1, 2, 18, 19, 20, 37, 38, 200, 400, 2**32, m - 1)[k % 12] * pow(a, m - 2, m) % m))
    for k in range(24):                                      # a == b
        a = rng.choice(pool_a)
        if a < lim_b:
            pairs.append((a, a))
    return pairs


class Case:
    """one instruction shape with its operand tuples; want[i] = the output list or the error code of tuple i (None: the test computes
    it -- the Poseidon rows come from the library's host function)"""

    def __init__(self, name, op, params, n_in, n_out, tuples, want=None):
        self.name, self.op, self.params, self.n_in, self.n_out, self.tuples = name, op, [int(x) for x in params], n_in, n_out, tuples
        assert all(len(t) == n_in and all(0 <= x < P for x in t) for t in tuples), name
        self.want = [reference(op, self.params, list(t), n_out) for t in tuples] if want is None else want
        for w in self.want:
            assert w is None or isinstance(w, int) or (len(w) == n_out and all(0 <= x < P for x in w)), (name, w)

    @property
    def instr(self):
        return (self.op, self.params, self.n_in, self.n_out)

    def good(self):
        return [i for i, w in enumerate(self.want) if not isinstance(w, int)]

    def bad(self):
        return [i for i, w in enumerate(self.want) if isinstance(w, int)]


def is_heavy(op, params, n_in):
    """wit_is_heavy: the instructions the device runs in the kernel with the generic big-integer code"""
    def is_p(ml):
        return value_of(ml) == P25519
    if op in (OP_NN_ADD, OP_NN_SUB):
        return not (is_p(params[1:9]) and params[0] <= 8 and n_in - params[0] <= 8)
    if op == OP_NN_MUL:
        return not (is_p(params[2:10]) and params[0] <= 8 and n_in - params[0] <= 8 and params[1] <= 9)
    if op == OP_NN_INV:
        return not (is_p(params[1:9]) and n_in <= 8 and params[0] <= 8)
    return op == OP_DIV_REM


def _nn_cases(rng):
    cases = []
    for tag, m, scale in (("p25519", P25519, 1), ("L", L25519, 0), ("secp", SECP, 0)):
        ml = limbs_of(m, 8)
        shapes = [(8, 8)] + ([(1, 8), (4, 8), (8, 4)] if scale else [(4, 8)])
        for na, nb in shapes:
            full = (na, nb) == (8, 8) and scale == 1
            pairs = nn_pairs(rng, m, na, nb, 160 if full else 48, full)
            if not scale:
                pairs = pairs[:150]
            tup = [limbs_of(a, na) + limbs_of(b, nb) for a, b in pairs]
            cases.append(Case("nn_add_%s_%dx%d" % (tag, na, nb), OP_NN_ADD, [na] + ml, na + nb, 9, tup))
            cases.append(Case("nn_sub_%s_%dx%d" % (tag, na, nb), OP_NN_SUB, [na] + ml, na + nb, 9, tup))
            for nover in ((8, 9) if (na, nb) == (8, 8) else (na + nb - 8,)):
                cases.append(Case("nn_mul_%s_%dx%d_q%d" % (tag, na, nb, nover), OP_NN_MUL, [na, nover] + ml, na + nb, 8 + nover, tup))
        for n in (8, 4, 1) if scale else (8, 4):
            xs = nn_edges(m, n) + [structured(rng, n) for _ in range(24 if scale else 8)] + \
                [rng.randrange(2**(32 * n)) for _ in range(40 if scale else 12)]
            if not scale:
                xs = xs[:44]
            cases.append(Case("nn_inv_%s_%d" % (tag, n), OP_NN_INV, [n] + ml, n, 2 * n, [limbs_of(x, n) for x in xs]))
    return cases


DIV_SHAPES = [(16, 8), (8, 8), (16, 3), (4, 2), (16, 1), (9, 8), (32, 8), (39, 20)]


def _div_operand(rng, n, kind):
    return structured(rng, n) if kind else rng.randrange(2**(32 * n))


def _div_cases(rng):
    """per shape: 200 pairs, 70 % structured; then, from 1 500 further structured draws, up to 48 that the model sends through the
    add-back (random operands take it with probability ~2^-31 per quotient limb)"""
    cases = []
    for la, lb in DIV_SHAPES:
        pairs = [(0, 0), (structured(rng, la), 0), (0, 1), (2**(32 * la) - 1, 2**(32 * lb) - 1), (2**(32 * la) - 1, 1),
                 (2**(32 * lb) - 1, 2**(32 * lb) - 1), (1 << (32 * la - 1), (1 << (32 * lb - 1)) + 1)]
        for k in range(200):
            s = k % 10 < 7
            a, b = _div_operand(rng, la, s), _div_operand(rng, lb, s or k % 10 == 7)
            if k % 25 == 0 and b:
                a = b * (a // b)                             # exact division: remainder 0
            pairs.append((a, b))
        extra = 0
        for _ in range(1500 if lb > 1 else 0):
            a, b = structured(rng, la), structured(rng, lb)
            if b and extra < 48 and "add_back" in divmod_model(a, b)[2]:
                pairs.append((a, b))
                extra += 1
        n_div = la - lb + 1
        cases.append(Case("div_rem_%dx%d" % (la, lb), OP_DIV_REM, [la, n_div, lb], la + lb, n_div + lb,
                          [limbs_of(a, la) + limbs_of(b, lb) for a, b in pairs]))
    return cases


def div_branch_counts(cases):
    """{branch: tuples taking it} over the OP_DIV_REM cases, by the model"""
    counts = dict.fromkeys(DIV_BRANCHES, 0)
    for c in cases:
        if c.op != OP_DIV_REM:
            continue
        la = c.params[0]
        for t in c.tuples:
            a, b = value_of(t[:la]), value_of(t[la:])
            if b:
                for k in divmod_model(a, b)[2]:
                    counts[k] += 1
    return counts


def _pt_add(p, q):
    (x1, y1), (x2, y2) = p, q
    t = D25519 * x1 * x2 * y1 * y2 % P25519
    return ((x1 * y2 + y1 * x2) * pow(1 + t, P25519 - 2, P25519) % P25519, (y1 * y2 + x1 * x2) * pow(1 - t, P25519 - 2, P25519) % P25519)


def _decompress_cases(rng):
    ys = [0, 1, 2, P25519 - 1, P25519, P25519 + 1, 2**255 - 20, 2**255 - 1, BASE_Y]
    base = (recover_x(BASE_Y, 0), BASE_Y)
    pt = base
    for _ in range(30):                                      # encodings of real points: k B, k = 1..30
        ys.append(pt[1])
        pt = _pt_add(pt, base)
    ys += [rng.getrandbits(255) for _ in range(40)]
    tup = []
    for y in ys:
        for sign in (0, 1):
            val = (sign << 255) | y
            tup.append([(val >> (255 - i)) & 1 for i in range(256)])
    return [Case("decompress", OP_DECOMPRESS, [], 256, 16, tup)]


CMP_SHAPES = [(16, 2), (8, 4), (4, 8), (2, 16), (1, 32), (6, 6), (5, 7)]


def _comparison_cases(rng):
    """x > y is an ordinary input of the gate (result bit 0, a negative most significant difference), not a failure: the most
    significant differing chunk gives |msd| < 2^chunk_bits, so 2^chunk_bits + msd < 2^(chunk_bits + 1) for EVERY pair and
    WIT_ERR_COMPARISON cannot be produced by any operand; the x > y pairs are checked against their full output lists"""
    cases = []
    for nc, cb in CMP_SHAPES:
        bits = nc * cb
        top, ones = 1 << (bits - 1), (1 << bits) - 1
        pairs = [(0, 0), (ones, ones), (0, ones), (ones, 0), (1, 0), (0, 1), (ones - 1, ones), (top - 1, top), (top, top - 1)]
        for _ in range(12):
            r = rng.getrandbits(bits)
            pairs += [(r, r), (r & ~1, r | 1), (r & ~top, r | top)]
            x, y = sorted((rng.getrandbits(bits), rng.getrandbits(bits)))
            pairs.append((x, y))
            if x != y:
                pairs.append((y, x))                         # x > y: result bit 0
            k = rng.randrange(nc)                            # equal above chunk k, random below
            lo = (1 << (cb * k)) - 1
            x, y = sorted(((r & ~lo) | (rng.getrandbits(bits) & lo), (r & ~lo) | (rng.getrandbits(bits) & lo)))
            pairs.append((x, y))
        cases.append(Case("comparison_%dx%d" % (nc, cb), OP_COMPARISON, [nc, cb], 2, 5 * nc + 1 + cb + 2, [list(p) for p in pairs]))
    # every g_inv_small(d), d = 1..64, and the first values past the switch to g_inv, with both signs of the chunk difference:
    # +d in the lowest 7-bit chunk, and -d there under a +1 in the chunk above
    pairs = []
    for d in range(1, 128):
        k = rng.randrange(128 - d)
        pairs += [(k, k + d), (k + d, (1 << 7) | k)]
    cases.append(Case("comparison_5x7_small_inverses", OP_COMPARISON, [5, 7], 2, 5 * 5 + 1 + 7 + 2, [list(p) for p in pairs]))
    return cases


def _field_vals(rng, n):
    return [rng.choice(DV.CANON) if rng.random() < 0.4 else rng.randrange(P) for _ in range(n)]


def _u32_cases(rng):
    cases = []
    r32 = lambda: rng.getrandbits(32)                        # noqa: E731
    mul = [[0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF],             # a b + c = p - 1 exactly: hi = 0xFFFFFFFF, third output 0
           [0xFFFFFFFF, B32, 0],                             # the same value with a 33-bit factor
           [0xFFFFFFFF, 0xFFFFFFFF, B32],                    # = p: fails
           [B32, B32, 0], [P - 1, P - 1, P - 1], [2**63, 2, 0], [2**63, 2, 1],     # >= 2^64: fail
           [0, 0, 0], [0, 0, P - 1], [1, P - 1, 0], [1, P - 1, 1], [0xFFFFFFFF, 0xFFFFFFFF, 0], [0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF]]
    mul += [[r32(), r32(), r32()] for _ in range(48)]
    cases.append(Case("u32_muladd", OP_U32_MULADD, [], 3, 35, mul))
    for n in (2, 3, 5, 16):
        # sums of exactly 16 2^32 - 1 (passes) and 16 2^32 (fails): n - 1 addends of 2^32 - 1 and one that completes the sum
        last = 16 * B32 - 1 - (n - 1) * 0xFFFFFFFF
        tup = [[0xFFFFFFFF] * n, [0] * n, [0xFFFFFFFF] * (n - 1) + [last], [0xFFFFFFFF] * (n - 1) + [last + 1]]
        tup += [[r32() for _ in range(n)] for _ in range(12)]
        cases.append(Case("add_many_%d" % n, OP_ADD_MANY, [], n, 20, tup))
    sub = [[x, y, b] for x in (0, 1, 0xFFFFFFFF) for y in (0, 1, 0xFFFFFFFF) for b in (0, 1)] + [[B32, 0, 0], [B32 + 5, 3, 1]]
    sub += [[r32(), r32(), rng.randrange(2)] for _ in range(16)]
    cases.append(Case("sub_u32", OP_SUB_U32, [], 3, 18, sub))
    for n in (1, 3):
        tup = [[0xFFFFFFFF] * n, [0] * n, [0xFFFFFFFF] * (n - 1) + [B32], [B32] + [0] * (n - 1), [P - 1] * n]
        tup += [[r32() for _ in range(n)] for _ in range(8)]
        cases.append(Case("range_check_%d" % n, OP_RANGE_CHECK, [], n, 16 * n, tup))
    cases.append(Case("interleave", OP_INTERLEAVE, [], 1, 33,
                      [[0], [0xFFFFFFFF], [B32], [P - 1], [0x55555555], [0xAAAAAAAA], [1], [0x80000000]] + [[r32()] for _ in range(12)]))
    for mode in (0, 1):
        tup = [[0], [P - 1], [0x5555555555555555], [0xAAAAAAAAAAAAAAAA], [0xFFFFFFFF], [0xFFFFFFFF00000000], [1], [2**63]]
        tup += [[rng.randrange(P)] for _ in range(16)]
        cases.append(Case("uninterleave_b32_%d" % mode, OP_UNINTERLEAVE, [mode], 1, 66, tup))
    return cases


def _digits(x, base):
    n = 0
    while x:
        x //= base
        n += 1
    return n


def _split_cases(rng):
    """per base: the limb counts that are exactly enough for p - 1 and for 2^32, and one fewer each; every x runs at every count,
    the reference says which fit"""
    cases = []
    for base in (2, 4, 16, 2**32, 2**63, 3, 7, 10):
        xs = [0, 1, P - 1, P - 2, 2**63, 2**32 - 1, 2**32, base - 1, base, base**2 % P] + [rng.randrange(P) for _ in range(6)] + \
            [rng.getrandbits(32) for _ in range(4)]
        for count in sorted({_digits(P - 1, base), _digits(P - 1, base) - 1, _digits(2**32, base), _digits(2**32, base) - 1} - {0}):
            cases.append(Case("split_base%d_x%d" % (base, count), OP_SPLIT, [base, count], 1, count, [[x] for x in xs]))
    return cases


def _base_cases(rng):
    cases = []
    for n in (1, 4, 32, 64):
        tup = [[1] * n, [0] * n, [P - 1] * n] + [[rng.randrange(2) for _ in range(n)] for _ in range(8)] + \
            [_field_vals(rng, n) for _ in range(16)]
        cases.append(Case("le_sum_%d" % n, OP_LE_SUM, [], n, 1, tup))
    for c0, c1 in ((1, 1), (P - 1, P - 1), (0, 1), (2**32, P - 2**32), (rng.randrange(P), rng.randrange(P))):
        tup = [[a, b, c] for a in (0, P - 1, 2**32) for b in (P - 1, 2**63) for c in (0, P - 1)] + [_field_vals(rng, 3) for _ in range(24)]
        cases.append(Case("arith_%d_%d" % (c0, c1), OP_ARITH, [c0, c1], 3, 1, tup))
    tup = [[a, b] for a in DV.CANON for b in DV.CANON] + [_field_vals(rng, 2) for _ in range(32)]
    tup += [[a, a] for a in _field_vals(rng, 16)]
    cases.append(Case("is_equal", OP_IS_EQUAL, [], 2, 2, tup))
    for bits in range(1, 7):
        n = 1 << bits
        tup = [[idx] + _field_vals(rng, n) for idx in (0, n - 1, n, n // 2, P - 1, 2**32) + tuple(rng.randrange(n) for _ in range(10))]
        cases.append(Case("random_access_%d" % bits, OP_RANDOM_ACCESS, [bits], 1 + n, 1 + bits, tup))
    return cases


def ext_values(rng):
    """the extension pairs of tests/test_gpu_devsim.py test_gl2_extension_ops"""
    comps = [0, 1, P - 1, P - 2, 2**32 - 1, 2**32, 2**63, P - 2**32]
    return [(0, 0), (1, 0), (0, 1), (P - 1, P - 1), (P - 1, 0)] + [(a, b) for a in comps[:4] for b in comps[4:]] + \
        [(rng.randrange(P), rng.randrange(P)) for _ in range(40)]


COSET_SHAPES = [(4, 6), (3, 4), (2, 3), (1, 2), (4, 5), (3, 2)]      # (4, 6) is what plonky2/recursion.py emits for arity 16; (3, 4),
# (2, 3) are its choices for arities 8 and 4


def _recursion_cases(rng):
    cases = []
    vals = ext_values(rng)
    flat = lambda es: [c for e in es for c in e]             # noqa: E731
    trip = [flat([a, rng.choice(vals), rng.choice(vals)]) for a in vals for _ in range(2)]
    for c0, c1 in ((1, 1), (P - 1, 2**32), (rng.randrange(P), rng.randrange(P))):
        cases.append(Case("ext_arith_%d" % c0, OP_EXT_ARITH, [c0, c1], 6, 2, trip))
    for c0 in (1, P - 1, rng.randrange(P)):
        cases.append(Case("ext_mul_%d" % c0, OP_EXT_MUL, [c0], 4, 2, [t[:4] for t in trip]))
    cases.append(Case("ext_inv", OP_EXT_INV, [], 2, 2, [list(e) for e in vals] + [[0, b] for b in DV.CANON] + [[a, 0] for a in DV.CANON]))
    for n in (1, 2, 64):
        tup = []
        for base in DV.CANON + [rng.randrange(P) for _ in range(8)]:
            for bits in ([1] * n, [0] * n, [rng.randrange(2) for _ in range(n)]):
                tup.append([base] + bits)
        cases.append(Case("exponentiation_%d" % n, OP_EXPONENTIATION, [], 1 + n, n + 1, tup))
    for ext, widths in ((False, (1, 2, 43)), (True, (1, 2, 32))):
        for n in widths:
            k = 4 + (2 * n if ext else n)
            tup = [flat([rng.choice(vals), rng.choice(vals)]) + _field_vals(rng, k - 4) for _ in range(24)]
            tup += [[P - 1] * k, [0] * k]
            cases.append(Case("reducing%s_%d" % ("_ext" if ext else "", n), OP_REDUCING_EXT if ext else OP_REDUCING, [n], k, 2 * n, tup))
    for sb, d in COSET_SHAPES:
        npts = 1 << sb
        k = 1 + 2 * npts + 2
        tup = [_field_vals(rng, k) for _ in range(12)] + [[P - 1] * k, [1] + [0] * (k - 1)]
        tup += [[0] + _field_vals(rng, k - 1)]               # zero shift: WIT_ERR_COSET_SHIFT
        tup = [[t[0] or 1] + t[1:] for t in tup[:-1]] + tup[-1:]
        cases.append(Case("coset_interp_%d_%d" % (sb, d), OP_COSET_INTERP, [sb, d] + barycentric_weights(sb), k,
                          2 + 4 * ((npts - 2) // (d - 1)) + 2, tup))
    tup = [[P - 1] * 24] + [[rng.choice(DV.CANON) for _ in range(24)] for _ in range(16)] + [_field_vals(rng, 24) for _ in range(16)] + \
        [[a] * 24 for a in DV.CANON]
    cases.append(Case("poseidon_mds", OP_POSEIDON_MDS, [], 24, 24, tup))
    return cases


def _poseidon_cases(rng):
    """the rows are the library's host function's (zklc_amd.plonky2.prover.poseidon_gate_rows) and must satisfy the oracle's gate:
    want = None for the tuples that have a row"""
    states = DV.poseidon_states(40, seed=11, loose=False) + [[rng.choice(DV.CANON) for _ in range(12)] for _ in range(12)]
    tup = []
    for i, s in enumerate(states):
        tup.append(list(s) + [i & 1])
    for _ in range(12):                                      # swap with the left half above / below the right half: the borrow of b - a
        lo, hi = sorted((rng.randrange(P), rng.randrange(P)))
        left_big = [hi] * 4 + [lo] * 4 + _field_vals(rng, 4)
        left_small = [lo] * 4 + [hi] * 4 + _field_vals(rng, 4)
        tup += [left_big + [1], left_small + [1], left_big + [0]]
    tup += [[P - 1] * 4 + [0] * 4 + [0] * 4 + [1], [0] * 4 + [P - 1] * 4 + [P - 1] * 4 + [1]]
    want = [None] * len(tup)
    tup += [list(states[3]) + [2], list(states[4]) + [P - 1]]
    want += [WIT_ERR_POSEIDON, WIT_ERR_POSEIDON]
    c12 = [list(s) for s in states[:3]]
    return [Case("poseidon", OP_POSEIDON, [], 13, 122, tup, want),
            Case("poseidon_12_inputs", OP_POSEIDON, [], 12, 122, c12, [WIT_ERR_POSEIDON] * len(c12))]


@functools.lru_cache(maxsize=None)
def table(seed=20):
    """every case of the table, built with a fixed seed"""
    rng = random.Random(seed)
    cases = []
    for f in (_nn_cases, _div_cases, _decompress_cases, _comparison_cases, _u32_cases, _split_cases, _base_cases, _recursion_cases,
              _poseidon_cases):
        cases += f(rng)
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


POSEIDON_OUT_COLS = [c for c in range(12, 135) if c != 24]      # the instruction's outputs: the row's wires 12..134 without the swap flag


def fill_poseidon(rows_fn):
    """want of the Poseidon tuples that have a row, from rows_fn(inputs [n, 12], swap [n]) -> rows [n, 135] (the caller passes
    zklc_amd.plonky2.prover.poseidon_gate_rows); -> [(tuple, full row)] for the check against the oracle's gate"""
    c = by_name("poseidon")
    idx = [i for i, w in enumerate(c.want) if not isinstance(w, int)]
    rows = rows_fn(np.array([c.tuples[i][:12] for i in idx], dtype=np.uint64), np.array([c.tuples[i][12] for i in idx], dtype=np.uint64))
    for i, row in zip(idx, rows):
        c.want[i] = [int(row[col]) for col in POSEIDON_OUT_COLS]
    return [(c.tuples[i], [int(x) for x in row]) for i, row in zip(idx, rows)]


def by_name(name):
    return next(c for c in table() if c.name == name)


def assert_coverage(cases):
    """the conditions the table is built to meet, checked on the model before any library call -> the counts, for the record"""
    div = div_branch_counts(cases)
    for k in ("qhat_corr", "qhat_big", "add_back"):
        assert div[k] >= 64, (k, div)
    assert div["lt"] >= 8 and div["one_limb"] >= 64, div
    dec = next(c for c in cases if c.op == OP_DECOMPRESS)
    frac = len(dec.good()) / len(dec.tuples)
    assert 0.25 <= frac <= 0.75, frac
    # non-native addition over p25519: a + b == p exactly (stays unreduced), and both outcomes of the overflow
    add = next(c for c in cases if c.name == "nn_add_p25519_8x8")
    eq_p = sum(1 for t in add.tuples if value_of(t[:8]) % P25519 + value_of(t[8:]) % P25519 == P25519)
    assert eq_p >= 8, eq_p
    # w25519_divmod: its loop of two conditional subtractions.  After the two folds R = r2 < 2^255 + 19 * 2^8, so R - p < p: the
    # second subtraction can never run, whatever the operands; the count is kept for the record (always 0) and the first one is
    # asserted in both outcomes
    second, first = 0, [0, 0]
    for c in cases:
        if c.op == OP_NN_MUL and value_of(c.params[2:10]) == P25519:
            for t in c.tuples:
                na = c.params[0]
                x = (value_of(t[:na]) % P25519) * (value_of(t[na:]) % P25519)
                r1 = 19 * (x >> 255) + (x & (2**255 - 1))
                r2 = 19 * (r1 >> 255) + (r1 & (2**255 - 1))
                second += r2 >= 2 * P25519
                first[r2 >= P25519] += 1
                assert r2 < 2**255 + 19 * 2**8
    assert min(first) >= 64 and second == 0, (first, second)
    # comparison: both inverse routes
    small = big = 0
    for c in cases:
        if c.op == OP_COMPARISON:
            nc, cb = c.params
            for t in c.tuples:
                for i in range(nc):
                    d = abs(((t[0] >> (cb * i)) & ((1 << cb) - 1)) - ((t[1] >> (cb * i)) & ((1 << cb) - 1)))
                    small += 1 <= d <= 64
                    big += d > 64
    assert small >= 64 and big >= 64, (small, big)
    codes = sorted({w for c in cases for w in c.want if isinstance(w, int)})
    return {"div": div, "decompress_decode_fraction": round(frac, 3), "nn_add_sum_equals_p": eq_p,
            "w25519_divmod_first_subtraction": first[1], "w25519_divmod_second_subtraction": second, "comparison_small_inverse_chunks": small, "comparison_g_inv_chunks": big,
            "error_codes": codes}


def tuples_per_opcode(cases):
    out = {}
    for c in cases:
        out[OP_NAMES[c.op]] = out.get(OP_NAMES[c.op], 0) + len(c.tuples)
    return out


# ------------------------------------------------------------------------------------------------ the device's launch plan
WIT_SMALL = 4096


def plan_launches(levels, W):
    """wit_plan of csrc/plonky2_witness_dev.hip on a list of levels, each a list of (opcode, heavy) -> [(kind, instructions)] with
    kind "step" (the single-workgroup stepping kernel over a run of levels), "light" (wit_level_kernel<false>) and "heavy"
    (wit_level_kernel<true>).  The rule: with Wp = the power of two >= W lanes per instruction, a level's instructions are sorted
    by (heavy, opcode) and every opcode group is padded to a multiple of 64 / Wp schedule slots; a level with no heavy instruction
    and at most 4096 lanes (slots x Wp) is "small", consecutive small levels share ONE stepping launch; any other level takes one
    light launch for its light slots and one heavy launch for its heavy slots."""
    Wp = 1
    while Wp < W:
        Wp *= 2
    G = 64 // Wp
    out, run, size = [], 0, 0

    def align(n):
        return -(-n // G) * G
    for lv in levels:
        start = size
        for h in (False, True):
            ops = [op for op, hv in lv if hv == h]
            for op in sorted(set(ops)):
                size = align(size) + ops.count(op)
            if not h:
                size = heavy_begin = align(size)
        count, heavy = size - start, size - heavy_begin
        if not heavy and count * Wp <= WIT_SMALL:
            run += 1
            continue
        if run:
            out.append(("step", run))
            run = 0
        if count > heavy:
            out.append(("light", count - heavy))
        if heavy:
            out.append(("heavy", heavy))
    if run:
        out.append(("step", run))
    return out
