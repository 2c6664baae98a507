"""zklc_bn254_g{1,2}_decode_host and gnark_keys.load_pk on the host path (no GPU): the lane functions of csrc/gnark_points.cuh
compiled for the host against the point-by-point Python reader (tests/gnark_point_cases.py)."""
import ctypes

import numpy as np
import pytest

import gnark_point_cases as C
from oracle import bn254 as B, groth16 as G
from zklc_amd import _lib, gnark_keys as K
from zklc_amd.formats import ProofInvalid

COMBOS = [(False, False), (False, True), (True, False), (True, True)]       # (g2, compressed)
TAU = (0x1234567891, 0xabcdef12345, 0x777766665555, 0x3133731337, 0x42424242)


def _check(got, want, what):
    words, status, summary = got
    _, e_status, e_words, e_summary = want
    bad = np.nonzero(np.asarray(status) != e_status)[0]
    assert len(bad) == 0, "%s: status of slot %d is %d, expected %d" % (what, bad[0], status[bad[0]], e_status[bad[0]])
    assert np.array_equal(np.asarray(words), e_words), what + ": words"
    assert list(summary) == e_summary, what + ": summary"


@pytest.mark.parametrize("g2,compressed", COMBOS)
@pytest.mark.parametrize("n", [1, 65, 300])
def test_host_decoder_equals_the_python_reader(g2, compressed, n):
    for start in ((0, 7) if n == 1 else (n,)):
        want = C.array(g2, compressed, n, start=start)
        _check(K.decode_points_host(want[0], n, g2=g2, compressed=compressed, chunk_points=128), want, "n = %d" % n)


def test_every_class_occurs_in_the_cases():
    for g2, compressed in COMBOS:
        cs = C.cases(g2, compressed)
        assert {c[1] for c in cs} == {C.OK, C.INFINITY, C.BAD_ENCODING, C.NOT_ON_CURVE}
        if g2:
            assert sum(c[2] == C.NOT_IN_SUBGROUP for c in cs) >= 8


@pytest.mark.parametrize("compressed", [False, True])
def test_host_decoder_g2_membership(compressed):
    want = C.array(True, compressed, 300, check_subgroup=True)
    assert (want[1] == C.NOT_IN_SUBGROUP).any() and (want[1] == C.OK).any()
    _check(K.decode_points_host(want[0], 300, g2=True, compressed=compressed, check_subgroup=True), want, "checked")
    # the same bytes without the flag: the twist points outside G2 are OK
    want = C.array(True, compressed, 300)
    _check(K.decode_points_host(want[0], 300, g2=True, compressed=compressed, nthreads=3), want, "unchecked")


def test_membership_classes_agree_with_the_oracle():
    """the classes known by construction, a sample of 16 confirmed by [r] Q == O"""
    cs = [c for c in C.cases(True, False) if c[1] == C.OK]
    sample = [c for c in cs if c[2] == C.NOT_IN_SUBGROUP][:10] + [c for c in cs if c[2] == C.OK][:6]
    assert len(sample) == 16
    for c in sample:
        pt = K.read_g2(K._Reader(c[0]))
        in_g2 = B.g2_add(B.g2_mul(B.R - 1, pt), pt) is None
        assert in_g2 == (c[2] == C.OK), c[5]


@pytest.mark.parametrize("g2,compressed", COMBOS)
def test_all_infinity_and_all_rejected_arrays(g2, compressed):
    want = C.array(g2, compressed, 70, only={C.INFINITY})
    assert want[3] == [0, 70, 0, None]
    _check(K.decode_points_host(want[0], 70, g2=g2, compressed=compressed), want, "all infinity")
    want = C.array(g2, compressed, 70, only={C.BAD_ENCODING, C.NOT_ON_CURVE})
    assert want[3] == [0, 0, 70, 0]
    _check(K.decode_points_host(want[0], 70, g2=g2, compressed=compressed), want, "all rejected")
    _check(K.decode_points_host(b"", 0, g2=g2, compressed=compressed), C.array(g2, compressed, 0), "empty")


def test_bad_arguments_are_errors_of_the_call():
    lib = _lib.load()
    data, _, _, _ = C.array(False, False, 4)
    src = K._aligned_u8(len(data) + 16)
    src[:len(data)] = np.frombuffer(data, dtype=np.uint8)
    words, status, summary = K._aligned_u8(4 * 128 + 16), np.zeros(4, dtype=np.uint32), np.zeros(4, dtype=np.uint64)
    call = lambda fn, p, flags, w=0: fn(src.ctypes.data + p, 4, flags, 1, words.ctypes.data + w, status.ctypes.data, summary.ctypes.data)
    g1, g2 = lib.zklc_bn254_g1_decode_host, lib.zklc_bn254_g2_decode_host
    assert call(g1, 0, 0) == 0
    assert call(g1, 8, 0) == -1 and call(g1, 0, 0, w=8) == -1 and call(g2, 4, 0) == -1          # ZKLC_ERR_INVALID_ARG: misaligned
    assert call(g1, 0, 4) == -1 and call(g2, 0, 8) == -1                                         # unknown flag bits
    assert call(g1, 0, _lib.POINTS_CHECK_SUBGROUP) == -1                                         # G1 has cofactor 1
    assert call(g1, 0, _lib.POINTS_COMPRESSED) == 0
    assert g1(None, 4, 0, 1, words.ctypes.data, status.ctypes.data, summary.ctypes.data) == -1
    assert g1(src.ctypes.data, 4, 0, 1, words.ctypes.data, status.ctypes.data, None) == -1
    assert lib.zklc_strerror(-1).startswith(b"invalid")


# ------------------------------------------------------------------------------------------------ the key loader, host path
@pytest.fixture(scope="module")
def key20():
    r1cs, _ = G.square_chain_r1cs(20, n_public=2)
    pk, _ = G.setup(r1cs, 2, TAU)
    assert any(p is None for p in pk["A"]) or any(p is None for p in pk["B1"])
    return pk


def _b2_offset(data, pk, raw, trailer):
    n_wires = len(pk["A"])
    n_b2 = sum(p is not None for p in pk["B2"])
    stride = 128 if raw else 64
    return len(data) - len(trailer) - 24 - 2 * n_wires - n_b2 * stride, n_b2, stride


@pytest.mark.parametrize("raw", [True, False])
def test_loader_equals_the_python_reader(key20, raw, tmp_path):
    trailer = b"\x00\x00\x00\x02commitment keys"
    data = K.pk_to_gnark_bytes(key20, raw=raw, trailer=trailer)
    want = K.pk_from_gnark_bytes(data, 2, raw=raw)
    path = tmp_path / "pk.bin"
    path.write_bytes(data)
    for src in (data, str(path)):
        got = K.load_pk(src, 2, raw=raw, chunk_points=16)
        assert got["n"] == want["n"] and got["n_public"] == 2 and got["trailer"] == trailer
        assert np.array_equal(got["infinity_a"], want["infinity_a"]) and np.array_equal(got["infinity_b"], want["infinity_b"])
        for name in ("alpha1", "beta1", "delta1", "beta2", "delta2"):
            assert got[name] == want[name], name
        for name in ("A", "B1", "Z", "K", "B2"):
            assert name not in got and name + "_dev" not in got
            assert got[name + "_words"].dtype == np.uint64
            assert np.array_equal(got[name + "_words"], K.points_to_words(want[name], g2=name == "B2")), name
        assert len(got["Z_words"]) == want["n"] - 1


def test_loader_names_the_rejected_point(key20):
    data = bytearray(K.pk_to_gnark_bytes(key20, raw=True, trailer=b"tail"))
    off, n_b2, stride = _b2_offset(data, key20, True, b"tail")
    assert n_b2 > 3
    data[off + 3 * stride + 64 + 31] ^= 1                     # B2[3], Y.A1
    with pytest.raises(ProofInvalid, match=r"B2\[3\]: NOT_ON_CURVE"):
        K.load_pk(bytes(data), 2)
    with pytest.raises(ProofInvalid):
        K.pk_from_gnark_bytes(bytes(data), 2)


@pytest.mark.parametrize("raw", [True, False])
def test_loader_tests_b2_for_membership(key20, raw):
    data = bytearray(K.pk_to_gnark_bytes(key20, raw=raw))
    off, n_b2, stride = _b2_offset(data, key20, raw, b"")
    data[off + 2 * stride:off + 3 * stride] = K.write_g2(C.twist_point_outside_g2(), raw)
    with pytest.raises(ProofInvalid, match=r"B2\[2\]: NOT_IN_SUBGROUP"):
        K.load_pk(bytes(data), 2, raw=raw)
    got = K.load_pk(bytes(data), 2, raw=raw, check_subgroup=False)           # on the twist: accepted when the test is off
    assert got["B2_words"][2].any()
    K.pk_from_gnark_bytes(bytes(data), 2, raw=raw)                            # the Python reader makes no subgroup test


def test_loader_reports_mixed_encodings(key20):
    data = bytearray(K.pk_to_gnark_bytes(key20, raw=True))
    off = 8 + 5 * 32 + 3 * 64 + 4                                             # A[0]
    assert data[off] >> 6 == 0
    data[off] |= 0x80
    with pytest.raises(ProofInvalid, match=r"A\[0\]: BAD_ENCODING.*mixes point encodings.*pk_from_gnark_bytes"):
        K.load_pk(bytes(data), 2)


def test_loader_refuses_malformed_keys_like_the_python_reader():
    """the malformed proving keys of tests/test_gnark_keys.py::test_malformed_keys_are_refused (and a cut inside a point array):
    the same message from both readers"""
    r1cs, _ = G.square_chain_r1cs(12, n_public=2)
    pk, _ = G.setup(r1cs, 2, TAU)
    good = K.pk_to_gnark_bytes(pk)
    flipped = bytearray(good)
    flipped[7] ^= 1                                                           # cardinality no power of two
    header = bytearray(good)
    header[8 + 31] ^= 1                                                       # CardinalityInv
    for data, n_pub in [(bytes(flipped), 2), (good, 3), (good[:-3], 2), (good[:1000], 2), (bytes(header), 2), (good[:50], 2)]:
        with pytest.raises(ProofInvalid) as e1:
            K.pk_from_gnark_bytes(data, n_pub)
        with pytest.raises(ProofInvalid) as e2:
            K.load_pk(data, n_pub)
        assert str(e1.value) == str(e2.value)
    assert K.load_pk(good, 2)["trailer"] == b""
