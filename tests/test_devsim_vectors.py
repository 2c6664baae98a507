"""The operand sets of tests/test_gpu_devsim.py without a GPU: the vector builders, their big-integer branch classification and the
conditions that keep the device tests from being vacuous (every named branch of the reductions at every slot of every batch width,
mixed within every 64 lanes) are checked on every CPU run."""
import importlib.util
import os
import random

import pytest

import devsim_vectors as DV

P = DV.P
MUL_WIDTHS = [1, 2, 3, 4, 5, 6, 7, 8, 15]
RANGE_WIDTHS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16, 18]


def _gen():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("gen_gl_asm", os.path.join(root, "tools", "gen_gl_asm.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_uniform_operands_never_take_the_rare_branches():
    """why the constructed operands exist: 20 000 uniform products, no borrow and no TP >= p, about half of them carry"""
    rng = random.Random(5)
    got = [DV.mul_model(rng.randrange(P), rng.randrange(P)) for _ in range(20000)]
    assert sum(m[1] for m in got) == 0 and sum(m[3] for m in got) == 0
    assert 9000 < sum(m[2] for m in got) < 11000


def test_constructions_take_their_branch():
    rng = random.Random(6)
    for _ in range(500):
        b = rng.randrange(2**40, P)
        a = DV.borrow_partner(b, rng.choice([1, 2, 3, 5]))
        r, borrow, _, _ = DV.mul_model(a, b)
        assert borrow and r == a * b % P
    for b in [7**i for i in range(1, 12)] + [rng.randrange(2, 2**32) for _ in range(500)]:
        a = DV.ge_p_partner_small(b)
        r, _, carry, ge = DV.mul_model(a, b)
        assert ge and not carry and r == a * b % P
    for _ in range(20):
        b = rng.randrange(2**32, 2**40)
        a = DV.ge_p_partner(b)
        assert a is not None and DV.mul_model(a, b)[3]


@pytest.mark.parametrize("width", MUL_WIDTHS)
def test_mul_batch_vectors_cover_every_branch_at_every_slot(width):
    x, t, want, flags = DV.mul_batch_vectors(width)
    assert DV.N_TUPLES % 64 and DV.N_TUPLES > 128
    assert len(x) == len(t) == len(want) == DV.N_TUPLES * width and max(x + t) < P
    DV.assert_coverage(flags, DV.N_TUPLES, width, DV.MUL_BRANCHES)


@pytest.mark.parametrize("width", RANGE_WIDTHS)
def test_range4_vectors_cover_every_branch_at_every_slot(width):
    x, want, flags = DV.range4_vectors(width)
    assert len(x) == DV.N_TUPLES * width and max(x) < P
    DV.assert_coverage(flags, DV.N_TUPLES, width, DV.RANGE_BRANCHES)
    for v in (0, 1, 2, 3, 4, P - 1, P - 2):
        assert v in x


def test_the_carry_of_y_plus_2_has_exactly_two_operands():
    """The carry of y + 2 in range4_stream needs the LOOSE y = x (x - 3) to be 2^64 - 2 or 2^64 - 1, so x is a root of
    x^2 - 3 x = 2^32 - 3 or = 2^32 - 2 (mod p).  The search (square roots mod p, then the reduction's model on each root): one of
    the two discriminants is a square, its two roots both leave the representative ABOVE p -- exactly two canonical limbs take the
    branch, and the range vectors carry them at every slot."""
    cands = DV.add2_carry_candidates()
    assert sorted(cands) == [(709008753516580104, True), (17737735315898004220, True)]
    for x, _ in cands:
        y = DV.loose_mul_model(x, x - 3)[0]
        assert y in (2**64 - 2, 2**64 - 1) and y % P == x * (x - 3) % P


def test_models_agree_with_the_generator_simulator():
    """the classification model and the generator's instruction lists are the same arithmetic: the simulator's result equals the
    model's (bit for bit, loose values included) on constructed, edge and random operands"""
    gen = _gen()
    prog, _, _, _ = gen.build_mul(1)
    x, t, want, flags = DV.mul_batch_vectors(1, n=400)
    assert sum(flags["borrow"]) > 50 and sum(flags["ge_p"]) > 50
    for a, b, w in zip(x, t, want):
        R = gen.simulate(prog, {"a0l": a & DV.EPS, "a0h": a >> 32, "b0l": b & DV.EPS, "b0h": b >> 32})
        assert R["r0l"] | (R["r0h"] << 32) == w
    prog, _, _, _ = gen.build_range4(2)
    xs, want, flags = DV.range4_vectors(2, n=200)
    for k in range(0, len(xs), 2):
        regs = {}
        for q in range(2):
            regs["x%dl" % q], regs["x%dh" % q] = xs[k + q] & DV.EPS, xs[k + q] >> 32
        R = gen.simulate(prog, regs)
        for q in range(2):
            assert R["r%dl" % q] | (R["r%dh" % q] << 32) == DV.range4_model(xs[k + q])[0]


@pytest.mark.parametrize("g,dit,inverse,zp", [(g, d, i, 0) for g in (1, 2, 3, 4) for d in (0, 1) for i in (0, 1)] + [(3, 0, 0, 3), (4, 0, 0, 3)])
def test_ntt_group_vectors_take_the_borrow_in_the_table_multiplications(g, dit, inverse, zp):
    x, t, want, flags = DV.ntt_group_vectors(g, dit, inverse, zp, n=130)
    M = 1 << g
    assert len(x) == len(want) == 130 * M and len(t) == 130 * (M - 1) and max(x + t) < P
    assert sum(flags["borrow"]) >= 32, sum(flags["borrow"])
    if g == 2 and not zp:      # the reference is the definition: a 4-point transform of the natural-order input (DIF -> bit-reversed out)
        w = pow(7, (P - 1) // 4, P)
        if inverse:
            w = pow(w, P - 2, P)
        xs, ones = x[:4], [1, 1, 1]
        got = DV.ntt_group_ref(2, dit, inverse, xs if not dit else [xs[0], xs[2], xs[1], xs[3]], ones)[0]
        dft = [sum(xs[j] * pow(w, j * k, P) for j in range(4)) % P for k in range(4)]
        assert (got if dit else [got[0], got[2], got[1], got[3]]) == dft


def test_mutated_reduction_passes_random_and_fails_constructed_operands():
    """what the constructed operands buy, shown with the generator's simulator: drop the repair of TP >= p (no carry) from
    mulmod_canonical and the list still agrees with big integers on 5 000 uniform products -- and disagrees on the constructed ones"""
    gen = _gen()
    prog, _, _, _ = gen.build_mul(1)
    mutated = [ins for ins in prog if ins[0] != "sor"]          # the select then sees the carry flag alone
    assert len(mutated) == len(prog) - 1
    rng = random.Random(8)

    def run(p, a, b):
        R = gen.simulate(p, {"a0l": a & DV.EPS, "a0h": a >> 32, "b0l": b & DV.EPS, "b0h": b >> 32})
        return R["r0l"] | (R["r0h"] << 32)
    for _ in range(5000):
        a, b = rng.randrange(P), rng.randrange(P)
        assert run(mutated, a, b) == a * b % P
    pools = DV.mul_pools(rng)
    bad = sum(run(mutated, a, b) != a * b % P for a, b in pools["ge_p"])
    assert bad == len(pools["ge_p"]) >= 64
    assert all(run(prog, a, b) == a * b % P for a, b in pools["ge_p"] + pools["borrow"])
