"""zklc_bn254_g{1,2}_decode_dev (csrc/gnark_points.hip) and gnark_keys.load_pk with a context: the kernels against the expectation
of tests/gnark_point_cases.py (the point-by-point Python reader) and against the host path, byte for byte; a prover built from the
device tensors of a loaded key against the oracle prover."""
import numpy as np
import pytest

import gnark_point_cases as C
from oracle import groth16 as G
from zklc_amd import gnark_keys as K
from zklc_amd.groth16 import Groth16Prover

pytestmark = pytest.mark.gpu

W = C.WORKGROUP
SIZES = [1, W + 1, 3 * W + 1]        # the tail guard alone, a second workgroup of one lane, the sum over several workgroups


def _run(zctx, g2, compressed, n, check_subgroup=False, **kw):
    want = C.array(g2, compressed, n, check_subgroup=check_subgroup, start=n % 7, **kw)
    words, status, summary = K.decode_points_dev(zctx, want[0], n, g2=g2, compressed=compressed, check_subgroup=check_subgroup)
    words, status = words.cpu().numpy().view(np.uint64), status.cpu().numpy().view(np.uint32)
    what = "g2 = %s, compressed = %s, n = %d" % (g2, compressed, n)
    bad = np.nonzero(status != want[1])[0]
    assert len(bad) == 0, "%s: status of slot %d is %d, expected %d" % (what, bad[0], status[bad[0]], want[1][bad[0]])
    assert np.array_equal(words, want[2]), what + ": words"
    assert list(summary) == want[3], what + ": summary"
    h_words, h_status, h_summary = K.decode_points_host(want[0], n, g2=g2, compressed=compressed, check_subgroup=check_subgroup)
    assert words.tobytes() == h_words.tobytes() and status.tobytes() == h_status.tobytes() and list(summary) == list(h_summary), \
        what + ": the kernels and the host path differ"


@pytest.mark.parametrize("g2,compressed", [(False, False), (False, True), (True, False), (True, True)])
def test_device_decoder_equals_the_python_reader_and_the_host_path(zctx, g2, compressed):
    for n in SIZES:
        _run(zctx, g2, compressed, n)


@pytest.mark.parametrize("compressed", [False, True])
def test_device_decoder_g2_membership(zctx, compressed):
    for n in SIZES:
        _run(zctx, True, compressed, n, check_subgroup=True)


def test_device_decoder_uniform_arrays_and_chunks(zctx):
    _run(zctx, False, False, W + 1, only={C.INFINITY})
    _run(zctx, True, True, W + 1, only={C.BAD_ENCODING, C.NOT_ON_CURVE})
    # several chunks: the summary is the sum over the calls, the first rejected index counts from the start of the array
    want = C.array(False, True, 2 * W + 5, only={C.OK})
    tail = C.array(False, True, 3, only={C.NOT_ON_CURVE})
    words, status, summary = K.decode_points_dev(zctx, want[0] + tail[0], 2 * W + 8, compressed=True, chunk_points=W)
    assert summary == [2 * W + 5, 0, 3, 2 * W + 5]
    assert np.array_equal(words.cpu().numpy().view(np.uint64), np.concatenate([want[2], tail[2]]))


def test_loaded_key_proves_like_the_oracle(zctx):
    """the 128-row key of test_gpu_groth16: written raw and compressed, loaded on the GPU, proved from the device tensors"""
    n_con, n_pub = 100, 3
    r1cs, wit = G.square_chain_r1cs(n_con, n_public=n_pub)
    pk, vk = G.setup(r1cs, n_pub, (0x1234567891, 0xabcdef12345, 0x777766665555, 0x3133731337, 0x42424242))
    assert pk["n"] == 128
    r, s = 0x1111222233334444, 0x5555666677778888
    pubs = [11, 22, 33]
    w = wit(pubs, 7)
    abc = G.abc_evaluations(r1cs, w, pk["n"])
    want = G.proof_to_uint256x8(G.prove(pk, r1cs, w, r, s))
    for raw in (True, False):
        data = K.pk_to_gnark_bytes(pk, raw=raw)
        loaded = K.load_pk(data, n_pub, raw=raw, ctx=zctx, chunk_points=100)
        for name in ("A", "B1", "Z", "K", "B2"):
            assert loaded[name + "_dev"].is_cuda and name + "_words" not in loaded
        prover = Groth16Prover(zctx, loaded)
        got = prover.prove(w, abc, r, s)
        prover.close()
        assert got == want, "the proof from the loaded key differs from the oracle prover's"
        python_read = Groth16Prover(zctx, K.pk_from_gnark_bytes(data, n_pub, raw=raw))
        assert python_read.prove(w, abc, r, s) == got
        python_read.close()
        assert G.verify(vk, ((got[0], got[1]), ((got[3], got[2]), (got[5], got[4])), (got[6], got[7])), pubs)
