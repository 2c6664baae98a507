"""zklc_bn254_g{1,2}_encode_host and gnark_keys.save_pk / save_vk on the host path (no GPU): the lane functions of
csrc/gnark_points_encode.cuh compiled for the host against the Python writer (tests/gnark_encode_cases.py), the round trip through
the decoder, key files against pk_to_gnark_bytes / vk_to_gnark_bytes byte for byte, and the stand-alone program of
tests/gnark_encode_host under the host sanitizers."""
import io
import os
import subprocess

import numpy as np
import pytest

import gnark_encode_cases as E
import groth16_size_cases as S
import setup_cases as SC
from conftest import ROOT
from zklc_amd import _lib, gnark_keys as K
from zklc_amd.formats import ProofInvalid
from zklc_amd.groth16 import save_pk, save_vk, setup_host
from zklc_amd.r1cs import R1CS

FORMS = [(False, False), (False, True), (True, False), (True, True)]       # (g2, compressed)
N = 2 * 256 + 77
ARRAYS = ("A", "B1", "Z", "K", "B2")
SINGLES = ("alpha1", "beta1", "delta1", "beta2", "delta2")


def test_every_class_and_every_ordering_edge_is_in_every_64_records():
    for g2 in (False, True):
        pat, bounds = E.pattern(g2), E.round_bounds(g2)
        assert len(bounds) == E.ROUNDS and all(0 < b - a <= E.ROUND_MAX for a, b in bounds)
        for validate, classes in ((False, {E.OK, E.INFINITY, E.BAD_ENCODING}), (True, {E.OK, E.INFINITY, E.BAD_ENCODING, E.NOT_ON_CURVE})):
            cls = [c for c, _ in E.expected_pattern(g2, False, validate)]
            assert [c for c, _ in E.expected_pattern(g2, True, validate)] == cls
            tiled = [(cls[i % len(pat)], pat[i % len(pat)][1]) for i in range(2 * len(pat) + E.WINDOW)]
            for first in range(2 * len(pat)):
                window = tiled[first:first + E.WINDOW]
                assert {c for c, _ in window} == classes, (g2, validate, first)
                assert set(E.edge_tags(g2)) <= {t for _, t in window}, (g2, first)
        tags = {t for _, t in pat}
        assert {"x = 0, y != 0", "only the last word non-zero", "multiple, -y", "multiple, one word changed", "infinity"} <= tags
        assert sum(t.startswith("coordinate ") for t in tags) == (12 if g2 else 6)        # p, p + 1, 2^256 - 1 in every position
        # the ordering edges fall on both sides, and both flags occur
        flags = {s[0] >> 6 for (c, s), (_, t) in zip(E.expected_pattern(g2, True, False), pat) if t.startswith("edge")}
        assert flags == {2, 3}
        by_tag = {t: c for (c, _), (_, t) in zip(E.expected_pattern(g2, False, True), pat)}
        assert by_tag["multiple"] == by_tag["multiple, -y"] == E.OK and by_tag["multiple, one word changed"] == E.NOT_ON_CURVE
        assert not g2 or by_tag["twist point outside G2"] == E.OK                           # no subgroup test


def _check(got, want, what):
    data, status, summary = got
    e_data, e_status, e_summary = want
    bad = np.nonzero(np.asarray(status) != e_status)[0]
    assert len(bad) == 0, "%s: status of record %d is %d, expected %d" % (what, bad[0], status[bad[0]], e_status[bad[0]])
    assert bytes(data) == e_data, what + ": bytes"
    assert list(summary) == e_summary, what + ": summary"


@pytest.mark.parametrize("g2,compressed", FORMS)
@pytest.mark.parametrize("validate", [False, True])
def test_host_encoder_equals_the_python_writer(g2, compressed, validate):
    for n, start, chunk in ((N, 3, 1 << 20), (N, 11, 100), (1, 0, 1 << 20), (1, 2, 1 << 20), (0, 0, 1 << 20)):
        got = K.encode_points_host(E.words(g2, n, start), n, g2=g2, compressed=compressed, validate=validate, chunk_points=chunk)
        _check(got, E.expected(g2, compressed, validate, n, start), "n = %d from %d in chunks of %d" % (n, start, chunk))


@pytest.mark.parametrize("g2,compressed", FORMS)
def test_decoding_the_encoders_bytes_gives_the_words_back(g2, compressed):
    """OK records come back word for word, infinity as zeros, and every 0xFF slot is BAD_ENCODING to the decoder"""
    words = E.words(g2, N, 5)
    data, status, _ = K.encode_points_host(words, N, g2=g2, compressed=compressed, validate=True)
    assert {int(s) for s in status} == {E.OK, E.INFINITY, E.BAD_ENCODING, E.NOT_ON_CURVE}
    back, d_status, _ = K.decode_points_host(data, N, g2=g2, compressed=compressed)
    ok, rejected = status == E.OK, status >= E.BAD_ENCODING
    assert np.array_equal(back[ok], words[ok]) and (d_status[ok] == _lib.POINT_OK).all()
    assert (d_status[status == E.INFINITY] == _lib.POINT_INFINITY).all()
    stride = len(data) // N
    assert all(bytes(data[i * stride:(i + 1) * stride]) == b"\xff" * stride for i in np.nonzero(rejected)[0])
    assert (d_status[rejected] == _lib.POINT_BAD_ENCODING).all() and not back[rejected].any()


def test_bad_arguments_are_errors_of_the_call():
    lib = _lib.load()
    words = K._aligned_u8(4 * 128 + 16)
    out, status, summary = K._aligned_u8(4 * 128 + 16), np.full(5, 0xA5A5A5A5, dtype=np.uint32), np.full(5, 7, dtype=np.uint64)
    out[:] = 0xA5
    call = lambda fn, flags, w=0, o=0, s=0, m=0: fn(words.ctypes.data + w, 4, flags, 1, out.ctypes.data + o, status.ctypes.data + s,
                                                    summary.ctypes.data + m)
    g1, g2 = lib.zklc_bn254_g1_encode_host, lib.zklc_bn254_g2_encode_host
    for fn in (g1, g2):
        assert call(fn, 0, w=8) == -1 and call(fn, 0, o=8) == -1 and call(fn, 0, s=2) == -1 and call(fn, 0, m=4) == -1   # misaligned
        assert call(fn, _lib.POINTS_CHECK_SUBGROUP) == -1 and call(fn, 8) == -1                      # no subgroup test; unknown bits
        assert fn(None, 4, 0, 1, out.ctypes.data, status.ctypes.data, summary.ctypes.data) == -1
        assert fn(words.ctypes.data, 4, 0, 1, None, status.ctypes.data, summary.ctypes.data) == -1
        assert fn(words.ctypes.data, 4, 0, 1, out.ctypes.data, None, summary.ctypes.data) == -1
        assert fn(words.ctypes.data, 4, 0, 1, out.ctypes.data, status.ctypes.data, None) == -1
        assert fn(words.ctypes.data, (1 << 31) + 1, 0, 1, out.ctypes.data, status.ctypes.data, summary.ctypes.data) == -1
    assert (out == 0xA5).all() and (status == 0xA5A5A5A5).all() and (summary == 7).all(), "a refused call writes nothing"
    assert call(g1, _lib.POINTS_COMPRESSED | _lib.POINTS_VALIDATE) == 0 and summary[:4].tolist() == [0, 4, 0, (1 << 64) - 1]
    assert _lib.POINTS_VALIDATE == 4


# ------------------------------------------------------------------------------------------------ key files, host path
@pytest.fixture(scope="module")
def key():
    """setup_host on the 100-constraint chain: (pk with *_words arrays, vk, the same pk as the integer tuples of the Python writer)"""
    sy = SC.system("chain100")
    r1cs = R1CS.from_csr(sy["n_constraints"], sy["n_wires"], *sy["csr"])
    try:
        pk, vk = setup_host(r1cs, sy["n_public"], S.TOXIC, window_bits=8)
    finally:
        r1cs.close()
    ints = {"n": pk["n"], "infinity_a": pk["infinity_a"], "infinity_b": pk["infinity_b"]}
    for name in ARRAYS:
        ints[name] = K.words_to_points(pk[name + "_words"], g2=name == "B2")
    for name in SINGLES:
        ints[name] = K.words_to_points(pk[name + "_words"], g2=name.endswith("2"))[0]
    assert pk["infinity_a"].any() or pk["infinity_b"].any()
    return pk, vk, ints, sy["n_public"]


@pytest.mark.parametrize("raw", [True, False])
def test_save_pk_equals_the_python_writer_and_loads_back(key, raw, tmp_path):
    pk, _, ints, n_public = key
    trailer = b"\x00\x00\x00\x02commitment keys"
    want = K.pk_to_gnark_bytes(ints, raw=raw, trailer=trailer)
    for chunk in (100, 1 << 20):                              # chunk seams inside A, B1, Z, K and B2; and one chunk per array
        path = tmp_path / ("pk_%d.bin" % chunk)
        assert save_pk(pk, str(path), raw=raw, chunk_points=chunk, trailer=trailer) == len(want)
        assert path.read_bytes() == want
    f = io.BytesIO()
    assert K.save_pk(pk, f, raw=raw, validate=False, nthreads=3, chunk_points=7, trailer=trailer) == len(want) and f.getvalue() == want
    loaded = K.load_pk(want, n_public, raw=raw)
    assert loaded["trailer"] == trailer and loaded["n"] == pk["n"]
    assert np.array_equal(loaded["infinity_a"], pk["infinity_a"]) and np.array_equal(loaded["infinity_b"], pk["infinity_b"])
    for name in ARRAYS:
        assert np.array_equal(loaded[name + "_words"], pk[name + "_words"]), name
    for name in SINGLES:
        assert loaded[name] == ints[name], name
    # a loaded key (single points as integer tuples) is written back to the same bytes
    f = io.BytesIO()
    K.save_pk(loaded, f, raw=raw, trailer=trailer)
    assert f.getvalue() == want


@pytest.mark.parametrize("raw", [True, False])
def test_save_vk_equals_the_python_writer(key, raw, tmp_path):
    _, vk, _, _ = key
    want = K.vk_to_gnark_bytes(vk, raw=raw, trailer=b"tail")
    path = tmp_path / "vk.bin"
    assert save_vk(vk, str(path), raw=raw, trailer=b"tail") == len(want) and path.read_bytes() == want
    f = io.BytesIO()
    K.save_vk(vk, f, raw=raw, chunk_points=2, trailer=b"tail")
    assert f.getvalue() == want
    back = K.vk_from_gnark_bytes(want, raw=raw)
    assert back.pop("trailer") == b"tail" and back == vk


def test_a_rejected_point_raises_and_leaves_no_file(key, tmp_path):
    pk, vk, _, _ = key
    bad = dict(pk)
    bad["K_words"] = pk["K_words"].copy()
    bad["K_words"][37, 5] ^= 1                                # K[37], y: off the curve
    path = tmp_path / "pk.bin"
    with pytest.raises(ProofInvalid, match=r"^K\[37\]: NOT_ON_CURVE$"):
        K.save_pk(bad, str(path), chunk_points=16)
    assert not path.exists()
    assert K.save_pk(bad, str(path), validate=False) > 0 and path.exists()        # canonical words: written when nobody asks
    bad["B2_words"] = pk["B2_words"].copy()
    bad["B2_words"][3, 8:12] = np.array(E._int_words(E.P), dtype=np.uint64)        # B2[3], X.A1 = p
    with pytest.raises(ProofInvalid, match=r"^B2\[3\]: BAD_ENCODING$"):
        K.save_pk({**bad, "K_words": pk["K_words"]}, str(path), validate=False)
    assert not path.exists()
    f = io.BytesIO()
    with pytest.raises(ProofInvalid, match=r"^delta1\[0\]: NOT_ON_CURVE$"):
        K.save_pk({**pk, "delta1_words": pk["delta1_words"] ^ np.uint64(2)}, f)
    bad_vk = dict(vk)
    bad_vk["K"] = list(vk["K"])
    bad_vk["K"][1] = (vk["K"][1][0], (vk["K"][1][1] + 1) % E.P)
    with pytest.raises(ProofInvalid, match=r"^K\[1\]: NOT_ON_CURVE$"):
        K.save_vk(bad_vk, str(tmp_path / "vk.bin"))
    assert not (tmp_path / "vk.bin").exists()


# ------------------------------------------------------------------------------------------------ the sanitizers
def _write_batches(path):
    """every form with and without validation at n = 0, 1, 255, 256, 257 (the host path's task is 256 points)"""
    batches = [(g2, compressed, validate, n) for g2, compressed in FORMS for validate in (False, True) for n in (0, 1, 255, 256, 257)]
    with open(path, "wb") as f:
        f.write(np.array([len(batches)], dtype=np.uint64).tobytes())
        for g2, compressed, validate, n in batches:
            data, status, summary = E.expected(g2, compressed, validate, n, start=n % 5)
            flags = (_lib.POINTS_COMPRESSED if compressed else 0) | (_lib.POINTS_VALIDATE if validate else 0)
            f.write(np.array([g2, flags, n], dtype=np.uint64).tobytes() + E.words(g2, n, start=n % 5).tobytes())
            f.write(np.array(summary[:3] + [E.ALL_ONES if summary[3] is None else summary[3]], dtype=np.uint64).tobytes())
            f.write(status.tobytes() + bytes(-4 * n % 8) + data)


def test_the_host_file_links_alone_and_is_clean_under_the_sanitizers(tmp_path):
    """csrc/gnark_points_encode_host.cpp + tests/gnark_encode_host/gnark_encode_host_main.cpp and nothing else, g++
    -fsanitize=address,undefined, as a child process: every malformed call, then output buffers of exactly n x stride bytes"""
    case = str(tmp_path / "batches.bin")
    _write_batches(case)
    exe = str(tmp_path / "gnark_encode_host_main")
    src = [os.path.join(ROOT, "tests", "gnark_encode_host", "gnark_encode_host_main.cpp"),
           os.path.join(ROOT, "zk-light-client-implementation_amd", "csrc", "gnark_points_encode_host.cpp")]
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                         "-pthread", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"] + src + ["-o", exe],
                        capture_output=True, text=True, timeout=600)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe, case], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "gnark encode host: ok" in run.stdout, (run.stdout + run.stderr)[-3000:]
