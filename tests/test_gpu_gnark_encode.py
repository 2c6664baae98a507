"""zklc_bn254_g{1,2}_encode_dev (csrc/gnark_points_encode.hip) and gnark_keys.save_pk / save_vk with a context: the kernels against the
expectation of tests/gnark_encode_cases.py (the Python writer) and against the host path, byte for byte; the round trip through the
decoding kernels; a key made by `Setup` written on the GPU, read back on the GPU, and proved and verified under."""
import io

import numpy as np
import pytest
import torch

import gnark_encode_cases as E
import groth16_size_cases as S
import setup_cases as SC
from oracle import groth16 as G
from zklc_amd import _lib, gnark_keys as K
from zklc_amd.groth16 import Groth16Prover, Groth16Verifier, Setup, save_pk, save_vk
from zklc_amd.r1cs import R1CS

pytestmark = pytest.mark.gpu

FORMS = [(False, False), (False, True), (True, False), (True, True)]       # (g2, compressed)
N = 2 * 256 + 77                    # two whole workgroups and a tail that ends inside a wave
INVALID = -1


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _run(zctx, g2, compressed, validate, n, start, **kw):
    words = E.words(g2, n, start)
    want = E.expected(g2, compressed, validate, n, start)
    data, status, summary = K.encode_points_dev(zctx, words, n, g2=g2, compressed=compressed, validate=validate, **kw)
    assert data.is_cuda and status.is_cuda
    data, status = _host(data, np.uint8), _host(status, np.uint32)
    what = "g2 = %s, compressed = %s, validate = %s, n = %d" % (g2, compressed, validate, n)
    bad = np.nonzero(status != want[1])[0]
    assert len(bad) == 0, "%s: status of record %d is %d, expected %d" % (what, bad[0], status[bad[0]], want[1][bad[0]])
    assert data.tobytes() == want[0], what + ": bytes"
    assert list(summary) == want[2], what + ": summary"
    h_data, h_status, h_summary = K.encode_points_host(words, n, g2=g2, compressed=compressed, validate=validate)
    assert data.tobytes() == h_data.tobytes() and status.tobytes() == h_status.tobytes() and list(summary) == list(h_summary), \
        what + ": the kernels and the host path differ"


@pytest.mark.parametrize("g2,compressed", FORMS)
def test_device_encoder_equals_the_python_writer_and_the_host_path(zctx, g2, compressed):
    for validate in (False, True):
        _run(zctx, g2, compressed, validate, N, 3)
    _run(zctx, g2, compressed, True, N, 9, chunk_points=256)          # three calls: the summary adds up, the index counts from 0


@pytest.mark.parametrize("g2,compressed", FORMS)
def test_one_point_and_no_point(zctx, g2, compressed):
    pat = E.pattern(g2)
    for start in range(0, len(pat), 5):                                # a lone lane of every kind of record
        _run(zctx, g2, compressed, True, 1, start)
    _run(zctx, g2, compressed, False, 0, 0)
    # n = 0 through the entry itself: the summary is initialised, nothing else is touched
    dev = torch.device("cuda", zctx.device_id)
    summary = torch.full((4,), 7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    zctx.bn254_points_encode_dev(None, 0, None, None, summary, group=2 if g2 else 1, flags=_lib.POINTS_COMPRESSED if compressed else 0,
                                 stream=zctx.stream_ptr())
    zctx.synchronize()
    assert summary.cpu().tolist() == [0, 0, 0, -1]


def test_malformed_calls_are_invalid_arguments_and_launch_nothing(zctx):
    dev = torch.device("cuda", zctx.device_id)
    lib = _lib.load()
    n = 4
    words = torch.from_numpy(E.words(True, n + 1).view(np.int64)).to(dev)
    out = torch.full((n * 128 + 16,), 0xA5, dtype=torch.uint8, device=dev)
    status = torch.full((n + 1,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    summary = torch.full((5,), 7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    for fn in (lib.zklc_bn254_g1_encode_dev, lib.zklc_bn254_g2_encode_dev):
        call = lambda flags=0, w=0, o=0, s=0, m=0, count=n, ctx=zctx._h: fn(ctx, zctx.stream_ptr(), words.data_ptr() + w, count, flags,
                                                                            out.data_ptr() + o, status.data_ptr() + s, summary.data_ptr() + m)
        assert call(w=8) == INVALID and call(o=8) == INVALID and call(s=2) == INVALID and call(m=4) == INVALID       # misaligned
        assert call(flags=_lib.POINTS_CHECK_SUBGROUP) == INVALID and call(flags=8) == INVALID                        # unknown here
        assert call(count=(1 << 31) + 1) == INVALID and call(ctx=None) == INVALID
        assert fn(zctx._h, zctx.stream_ptr(), None, n, 0, out.data_ptr(), status.data_ptr(), summary.data_ptr()) == INVALID
        assert fn(zctx._h, zctx.stream_ptr(), words.data_ptr(), n, 0, None, status.data_ptr(), summary.data_ptr()) == INVALID
        assert fn(zctx._h, zctx.stream_ptr(), words.data_ptr(), n, 0, out.data_ptr(), None, summary.data_ptr()) == INVALID
        assert fn(zctx._h, zctx.stream_ptr(), words.data_ptr(), n, 0, out.data_ptr(), status.data_ptr(), None) == INVALID
    zctx.synchronize()
    assert bool((out == 0xA5).all()) and bool((status == 0x5A5A5A5A).all()) and bool((summary == 7).all()), "a refused call launched"
    # the decoding entries still refuse the new flag
    assert lib.zklc_bn254_g1_decode_dev(zctx._h, zctx.stream_ptr(), out.data_ptr(), n, _lib.POINTS_VALIDATE, words.data_ptr(),
                                        status.data_ptr(), summary.data_ptr()) == INVALID
    # a good call writes n slots and not a byte behind them
    assert lib.zklc_bn254_g2_encode_dev(zctx._h, zctx.stream_ptr(), words.data_ptr(), n, 0, out.data_ptr(), status.data_ptr(),
                                        summary.data_ptr()) == 0
    zctx.synchronize()
    assert _host(out, np.uint8)[:n * 128].tobytes() == E.expected(True, False, False, n)[0]
    assert bool((out[n * 128:] == 0xA5).all()) and int(status[n]) == 0x5A5A5A5A and int(summary[4]) == 7


@pytest.mark.parametrize("g2,compressed", FORMS)
def test_decoding_kernels_give_the_encoded_words_back(zctx, g2, compressed):
    words = E.words(g2, N, 5)
    data, status, _ = K.encode_points_dev(zctx, words, N, g2=g2, compressed=compressed, validate=True)
    status = _host(status, np.uint32)
    back, d_status, _ = K.decode_points_dev(zctx, _host(data, np.uint8), N, g2=g2, compressed=compressed)
    back, d_status = _host(back, np.uint64), _host(d_status, np.uint32)
    ok, rejected = status == E.OK, status >= E.BAD_ENCODING
    assert ok.sum() > 50 and rejected.sum() > 50
    assert np.array_equal(back[ok], words[ok]) and (d_status[ok] == _lib.POINT_OK).all()
    assert (d_status[status == E.INFINITY] == _lib.POINT_INFINITY).all()
    assert (d_status[rejected] == _lib.POINT_BAD_ENCODING).all() and not back[rejected].any()


def test_a_key_from_setup_is_written_read_back_and_proved_under(zctx, tmp_path):
    """`Setup` on the smallest system of tests/setup_cases.py -> save_pk / save_vk on the GPU -> load_pk on the GPU -> a proof"""
    sy = SC.system(SC.SYSTEM_NAMES[0])
    assert sy["n"] == min(SC.system(name)["n"] for name in SC.SYSTEM_NAMES) == 2
    r1cs, wit = G.square_chain_r1cs(sy["n_constraints"])
    n_public = sy["n_public"]
    sys_ = R1CS.from_csr(sy["n_constraints"], sy["n_wires"], *sy["csr"], ctx=zctx)
    try:
        pk, vk = Setup(zctx, sys_, n_public, S.TOXIC)
        ints = {"n": pk["n"], "infinity_a": pk["infinity_a"], "infinity_b": pk["infinity_b"]}
        for name in ("A", "B1", "Z", "K", "B2"):
            ints[name] = K.words_to_points(_host(pk[name + "_dev"], np.uint64), g2=name == "B2")
        for name in ("alpha1", "beta1", "delta1", "beta2", "delta2"):
            ints[name] = K.words_to_points(pk[name + "_words"], g2=name.endswith("2"))[0]
        pubs = [11, 22][:n_public]
        w = wit(pubs, 5)
        for raw in (True, False):
            want = K.pk_to_gnark_bytes(ints, raw=raw, trailer=b"tail")
            path = str(tmp_path / ("pk_%d.bin" % raw))
            assert save_pk(pk, path, raw=raw, ctx=zctx, trailer=b"tail") == len(want)
            assert open(path, "rb").read() == want
            f = io.BytesIO()
            K.save_pk(pk, f, raw=raw, ctx=zctx, chunk_points=1, trailer=b"tail")      # every point a chunk of its own: both buffers in turn
            assert f.getvalue() == want
            f = io.BytesIO()
            save_vk(vk, f, raw=raw, ctx=zctx)
            assert f.getvalue() == K.vk_to_gnark_bytes(vk, raw=raw)
            loaded = K.load_pk(path, n_public, raw=raw, ctx=zctx)
            assert loaded["trailer"] == b"tail"
            for name in ("A", "B1", "Z", "K", "B2"):
                assert loaded[name + "_dev"].is_cuda and torch.equal(loaded[name + "_dev"], pk[name + "_dev"]), name
            prover = Groth16Prover(zctx, loaded, sys_)
            try:
                proof = prover.prove_witness(w, 12345, 67890)
            finally:
                prover.close()
            ver = Groth16Verifier(zctx, K.vk_from_gnark_bytes(f.getvalue(), raw=raw))
            assert ver.verify(proof, pubs) is True
            assert ver.verify(proof, [pubs[0] + 1] + pubs[1:]) is False
        # a rejected point: named, and no file left
        bad = dict(pk)
        bad["Z_dev"] = pk["Z_dev"].clone()
        bad["Z_dev"][0, 4] ^= 1
        path = tmp_path / "bad.bin"
        with pytest.raises(K.ProofInvalid, match=r"^Z\[0\]: NOT_ON_CURVE$"):
            K.save_pk(bad, str(path), ctx=zctx)
        assert not path.exists()
    finally:
        sys_.close()
