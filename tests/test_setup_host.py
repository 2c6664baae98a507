"""The scalar stage of groth16.Setup on the host (zklc_groth16_setup_scalars_host: the lane functions of csrc/groth16_setup.cuh, g++)
against `oracle.groth16.key_scalars` on every system and toxic set of tests/setup_cases.py, every malformed call of include/zklc.h,
and `setup_host` -- the two host stages joined -- against the closed form of the key.  No GPU.  Exact equality of integers."""
import random

import numpy as np
import pytest

import groth16_size_cases as S
import setup_cases as C
from oracle import bn254 as B, groth16 as G
from zklc_amd import _lib, gnark_keys as GK, groth16_setup as GS
from zklc_amd.groth16 import setup_host, setup_scalars_host
from zklc_amd.r1cs import R1CS

R = G.R
INVALID = -1


def make_r1cs(name, ctx=None):
    sy = C.system(name)
    return R1CS.from_csr(sy["n_constraints"], sy["n_wires"], *sy["csr"], ctx=ctx)


@pytest.fixture(scope="module")
def systems():
    out = {name: make_r1cs(name) for name in C.SYSTEM_NAMES}
    yield out
    for s in out.values():
        s.close()


def test_the_cases_reach_every_path():
    """what the systems are chosen for, stated on the oracle's side: domains 2 and 4, live padding, a column longer than a segment
    (at least two segments), columns for 1, 8 and 64 lanes, empty columns, zero scalars, all three coefficient classes"""
    assert GS.SEG_TERMS <= 2048
    assert [C.system(n)["n"] for n in C.SYSTEM_NAMES] == [2, 4, 128, 4096, 8192, 8]
    assert C.system("chain4000")["n_constraints"] == 4000 < C.system("chain4000")["n"]
    lens = C.column_lengths("chain4000")
    assert lens[(2, 0)] == 4000 > GS.SEG_TERMS and C.expected_plan("chain4000", GS.SEG_TERMS)["segments"] >= 2
    assert all(c == R - 3 for row in C.system("chain4000")["rows"][2] for w, c in row if w == 0)
    total = [0] * 4
    for name in C.SYSTEM_NAMES:
        p = C.expected_plan(name, GS.SEG_TERMS)
        total = [a + b for a, b in zip(total, list(p.values())[:4])]
    assert all(total), "a lanes-per-column bin no system reaches: %r" % total
    # the bits system: short columns and columns for a wave (the constant and the public wires); the eight-lane bin is
    # chain100's (its public wires: 33 or 34 terms), the segments are chain4000's
    p = C.expected_plan("bits8192", GS.SEG_TERMS)
    assert p["cols_1_lane"] and p["cols_64_lanes"] and C.expected_plan("chain100", GS.SEG_TERMS)["cols_8_lanes"] == 3
    e = C.expected("bits8192", "base")
    assert sum(1 for a, b in zip(e["a_t"], e["b_t"]) if a == 0 and b == 0) >= 50
    coeffs = {c for M in C.system("bits8192")["rows"] for row in M for _, c in row}
    assert {1, R - 1} < coeffs and len(coeffs) > 10
    e = C.expected("hand5", "base")
    assert e["a_t"][4] == e["b_t"][4] == e["k"][4] == 0 and e["b_t"][1] == 0 and e["a_t"][3] != 0
    assert not any(C.expected("chain100", "tau_in_domain")["z"]) and any(C.expected("chain100", "tau_zero")["z"][:1])


def test_the_plan_function_counts_columns_like_the_oracle(systems):
    for name, sys_ in systems.items():
        assert GS.plan(sys_) == C.expected_plan(name, GS.SEG_TERMS), name


@pytest.mark.parametrize("system_name,toxic_name", C.CASES, ids=C.CASE_IDS)
def test_host_scalars_equal_the_oracle(systems, system_name, toxic_name):
    sy = C.system(system_name)
    want = C.expected_words(system_name, toxic_name)
    for nthreads in (1, 16):
        got = setup_scalars_host(systems[system_name], sy["n_public"], C.toxic(toxic_name, sy["n"]), nthreads=nthreads)
        for name, g, w in zip(("a_t", "b_t", "k", "z"), got, want):
            assert g.shape == w.shape and np.array_equal(g, w), "%s differs (%d threads)" % (name, nthreads)


def test_a_larger_domain_than_the_constraints_need(systems):
    """n is the caller's: 100 constraints on a domain of 256"""
    sy = C.system("chain100")
    assert sy["n"] == 128
    pad = tuple(list(M) + [{}] * 100 for M in sy["oracle_rows"])       # 200 constraints, the last 100 empty: the oracle's domain is 256
    want = G.key_scalars(pad, sy["n_public"], S.TOXIC)
    assert want["n"] == 256
    a_t, b_t, k, z = setup_scalars_host(systems["chain100"], sy["n_public"], S.TOXIC, n=256)
    assert S.ints_from_words(a_t) == want["a_t"] and S.ints_from_words(b_t) == want["b_t"]
    assert S.ints_from_words(k) == want["k_vk"] + want["k_pk"] and S.ints_from_words(z) == want["z"]


def _aligned(n_words, fill=0x99):
    """uint64 array of n_words whose address is a multiple of 16, filled with a pattern"""
    raw = np.full(n_words + 2, 0, dtype=np.uint64)
    off = (-raw.ctypes.data % 16) // 8
    a = raw[off:off + n_words]
    a.view(np.uint8)[:] = fill
    assert a.ctypes.data % 16 == 0
    return a


def test_malformed_calls_are_invalid_arguments(systems):
    lib = _lib.load()
    sy = C.system("chain3")
    s, npub, n, nw = systems["chain3"], sy["n_public"], sy["n"], sy["n_wires"]
    a_t, b_t, k, z = _aligned(4 * nw), _aligned(4 * nw), _aligned(4 * nw), _aligned(4 * (n - 1))
    good = GS.toxic_words(S.TOXIC)

    def call(sys_=s, toxic=good, n_public=npub, n_=n, outs=None):
        p = [x.ctypes.data if x is not None else None for x in (outs or (a_t, b_t, k, z))]
        h = sys_._handle() if sys_ is not None else None
        return lib.zklc_groth16_setup_scalars_host(h, toxic.ctypes.data if toxic is not None else None, n_public, n_, 1, *p)

    def with_toxic(i, v):
        t = list(S.TOXIC)
        t[i] = v
        return GS.toxic_words(t)
    bad = {
        "gamma = 0": dict(toxic=with_toxic(3, 0)), "gamma = r": dict(toxic=with_toxic(3, R)), "delta = 0": dict(toxic=with_toxic(4, 0)),
        "delta = 2 r": dict(toxic=with_toxic(4, 2 * R)), "n = 3": dict(n_=3), "n = 6": dict(n_=6), "n below the constraints": dict(n_=2),
        "n = 1": dict(n_=1), "n = 0": dict(n_=0), "n = 2^29": dict(n_=1 << 29), "n = 2^63": dict(n_=1 << 63),
        "n_public + 1 > n_wires": dict(n_public=nw), "n_public = 2^32 - 1": dict(n_public=(1 << 32) - 1), "no system": dict(sys_=None),
        "no toxic waste": dict(toxic=None),
    }
    for i, name in enumerate(("a_t", "b_t", "k", "z")):
        outs = [a_t, b_t, k, z]
        outs[i] = None
        bad["no " + name] = dict(outs=tuple(outs))
        outs = [a_t, b_t, k, z]
        outs[i] = outs[i][1:]                                       # 8 bytes further: not 16-byte aligned
        bad["misaligned " + name] = dict(outs=tuple(outs))
    for what, kw in bad.items():
        assert call(**kw) == INVALID, what
    for x in (a_t, b_t, k, z):
        assert (x.view(np.uint8) == 0x99).all(), "a refused call writes nothing"
    assert call(n_=1, sys_=systems["chain1"], n_public=2) == INVALID        # max(2, n_constraints) with one constraint
    assert lib.zklc_groth16_setup_workspace_bytes(s._handle(), 3) == 0 and lib.zklc_groth16_setup_workspace_bytes(None, 4) == 0
    assert lib.zklc_groth16_setup_workspace_bytes(s._handle(), 1 << 29) == 0 and lib.zklc_groth16_setup_workspace_bytes(s._handle(), 4) > 0
    assert lib.zklc_groth16_setup_plan(None, a_t.ctypes.data) == INVALID and lib.zklc_groth16_setup_plan(s._handle(), None) == INVALID
    assert call() == 0 and np.array_equal(a_t.reshape(-1, 4), C.expected_words("chain3", "base")[0])
    # toxic needs 8-byte alignment only (include/zklc.h): the same words at 8 mod 16 are a GOOD call with the same scalars
    shifted = _aligned(22)[1:21]
    shifted[:] = good.reshape(-1)
    assert shifted.ctypes.data % 16 == 8
    a_t[:] = 0
    z[:] = 0
    assert call(toxic=shifted) == 0 and np.array_equal(a_t.reshape(-1, 4), C.expected_words("chain3", "base")[0])
    assert np.array_equal(z.reshape(-1, 4), C.expected_words("chain3", "base")[3])
    with pytest.raises(_lib.ZklcError) as e:
        setup_scalars_host(s, npub, (S.TOXIC[0], 1, 1, R, 1))
    assert e.value.code == INVALID
    with pytest.raises(ValueError):
        setup_scalars_host(s, npub, (1, 2, 3, 4, 1 << 256))


@pytest.fixture(scope="module")
def host_key(systems):
    sy = C.system("chain100")
    pk, vk = setup_host(systems["chain100"], sy["n_public"], S.TOXIC, window_bits=8)
    return sy, pk, vk


def test_setup_host_gives_the_closed_form_verifying_key(host_key):
    sy, pk, vk = host_key
    sc = C.expected("chain100", "base")["scalars"]
    want = G.closed_form_vk(sc, S.TOXIC, sy["n_public"])
    assert {k: vk[k] for k in want} == want
    tau, alpha, beta, gamma, delta = S.TOXIC
    assert vk["beta1"] == B.mul(beta, B.G1) and vk["delta1"] == B.mul(delta, B.G1)
    assert GK.words_to_points(pk["alpha1_words"]) == [B.mul(alpha, B.G1)] and GK.words_to_points(pk["beta1_words"]) == [vk["beta1"]]
    assert GK.words_to_points(pk["delta1_words"]) == [vk["delta1"]]
    assert GK.words_to_points(pk["beta2_words"], g2=True) == [vk["beta2"]] and GK.words_to_points(pk["delta2_words"], g2=True) == [vk["delta2"]]


def test_setup_host_points_and_masks_are_the_scalars(host_key):
    """the masks are the zero scalars; per array the first, the last and three random points against B.mul / B.g2_mul (the arrays
    A / B1 / B2 are compacted: wire i is at the number of kept wires before it)"""
    sy, pk, vk = host_key
    e = C.expected("chain100", "base")
    sc = e["scalars"]
    assert pk["n"] == 128 and pk["n_public"] == 3
    assert pk["infinity_a"].tolist() == [x == 0 for x in e["a_t"]] and pk["infinity_b"].tolist() == [x == 0 for x in e["b_t"]]
    assert pk["infinity_a"].sum() >= 4 and pk["infinity_b"].sum() >= 4
    assert len(pk["A_words"]) == int((~pk["infinity_a"]).sum()) and len(pk["B1_words"]) == len(pk["B2_words"]) == int((~pk["infinity_b"]).sum())
    assert len(pk["K_words"]) == len(sc["k_pk"]) == sy["n_wires"] - 4 and len(pk["Z_words"]) == 127
    rng = random.Random(16)
    for name, scalars, g2 in (("A", e["a_t"], False), ("B1", e["b_t"], False), ("B2", e["b_t"], True), ("K", sc["k_pk"], False),
                              ("Z", sc["z"], False)):
        kept = [i for i, x in enumerate(scalars) if x] if name in ("A", "B1", "B2") else list(range(len(scalars)))
        assert len(kept) == len(pk[name + "_words"])
        picks = sorted({0, len(kept) - 1} | {rng.randrange(len(kept)) for _ in range(1 if g2 else 3)})
        got = GK.words_to_points(pk[name + "_words"][picks], g2=g2)
        for at, pt in zip(picks, got):
            x = scalars[kept[at]]
            want = (B.g2_mul(x, B.G2) if g2 else B.mul(x, B.G1)) if x else None
            assert pt == want, "%s[%d]" % (name, at)


def test_words_to_points_inverts_points_to_words():
    pts = [None, B.G1, B.mul(5, B.G1), None, B.mul(R - 1, B.G1)]
    assert GK.words_to_points(GK.points_to_words(pts)) == pts
    pts2 = [B.G2, None, B.g2_mul(7, B.G2)]
    assert GK.words_to_points(GK.points_to_words(pts2, g2=True), g2=True) == pts2
    assert GK.words_to_points(np.zeros((0, 8), dtype=np.uint64)) == [] and GK.words_to_points(np.zeros((2, 16), dtype=np.uint64), g2=True) == [None, None]


def test_the_key_survives_gnarks_file_format(host_key):
    """pk -> integer tuples -> pk_to_gnark_bytes -> pk_from_gnark_bytes: the same key, masks included"""
    sy, pk, vk = host_key
    as_points = {"n": pk["n"], "n_public": pk["n_public"], "infinity_a": pk["infinity_a"], "infinity_b": pk["infinity_b"]}
    for name in ("A", "B1", "K", "Z"):
        as_points[name] = GK.words_to_points(pk[name + "_words"])
    as_points["B2"] = GK.words_to_points(pk["B2_words"], g2=True)
    for name in ("alpha1", "beta1", "delta1"):
        as_points[name] = GK.words_to_points(pk[name + "_words"])[0]
    for name in ("beta2", "delta2"):
        as_points[name] = GK.words_to_points(pk[name + "_words"], g2=True)[0]
    data = GK.pk_to_gnark_bytes(as_points)
    back = GK.pk_from_gnark_bytes(data, pk["n_public"])
    assert back["n"] == pk["n"] and back["trailer"] == b""
    for name in ("A", "B1", "B2", "K", "Z", "alpha1", "beta1", "delta1", "beta2", "delta2"):
        assert back[name] == as_points[name], name
    assert back["infinity_a"].tolist() == pk["infinity_a"].tolist() and back["infinity_b"].tolist() == pk["infinity_b"].tolist()
    for name in ("A", "B1", "K", "Z"):
        assert np.array_equal(GK.points_to_words(back[name]), pk[name + "_words"]), name
    assert np.array_equal(GK.points_to_words(back["B2"], g2=True), pk["B2_words"])
    assert GK.vk_from_gnark_bytes(GK.vk_to_gnark_bytes(vk))["K"] == vk["K"]
