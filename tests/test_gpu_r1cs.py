"""A w, B w, C w of a resident constraint system on the GPU (zklc_r1cs_abc_dev: csrc/r1cs_eval.hip) against Python integers and
the host twin (tests/r1cs_cases.py), byte for byte; and `Groth16Prover.prove_witness`: from the solved witness to the proof words of
oracle/groth16.py, or to the index of the violated constraint."""
import numpy as np
import pytest
import torch

import r1cs_cases as C
from oracle import groth16 as G
from zklc_amd.groth16 import Groth16Prover, UnsatisfiedConstraint
from zklc_amd.r1cs import R1CS, summary_tuple

pytestmark = pytest.mark.gpu

FF = -1               # int64 with every bit set


def _dev_eval(zctx, sys_, w, n, check=True):
    """the kernels into buffers filled with 0xFF -> (a, b, c as uint64 arrays, summary)"""
    dev = torch.device("cuda", zctx.device_id)
    d_w = torch.from_numpy(C.witness_words(w).view(np.int64)).to(dev)
    a, b, c = (torch.full((n, 4), FF, dtype=torch.int64, device=dev) for _ in range(3))
    d_sum = torch.full((2,), 7, dtype=torch.int64, device=dev) if check else None
    torch.cuda.current_stream(dev).synchronize()
    sys_.enqueue(zctx, d_w, n, a, b, c, d_sum)
    zctx.synchronize()
    h = lambda t: t.cpu().numpy().view(np.uint64)
    return h(a), h(b), h(c), (summary_tuple(h(d_sum)) if check else None)


def _equal(got, want, what):
    for name, g, w in zip("abc", got[:3], want[:3]):
        bad = np.nonzero((g != w).any(axis=1))[0]
        assert len(bad) == 0, "%s: row %d of %s is %s, expected %s" % (what, bad[0], name, g[bad[0]], w[bad[0]])
        assert g.tobytes() == w.tobytes()
    assert got[3] == want[3], what + ": summary"


def test_kernels_equal_python_and_the_host_twin_on_the_edge_system(zctx):
    s = C.edge_system()
    n = 2 * C.domain_size(s.n_constraints)
    _, w, *want = C.expected_cached("edge", 0, n)
    sys_ = R1CS.from_csr(*s.csr(), ctx=zctx)
    got = _dev_eval(zctx, sys_, w, n)
    _equal(got, want, "kernels against Python")
    _equal(got, sys_.abc_host(C.witness_words(w), n, check=True), "kernels against the host twin")
    # without the check: the same words; n = n_constraints: no padding kernel
    _equal(_dev_eval(zctx, sys_, w, n, check=False) + (), want[:3] + [None], "unchecked")
    _, _, *want0 = C.expected_cached("edge", 0, s.n_constraints)
    _equal(_dev_eval(zctx, sys_, w, s.n_constraints), want0, "n = n_constraints")
    sys_.close()


@pytest.mark.parametrize("nc", [1, 65, 3 * 256 + 1])
def test_kernels_equal_python_on_random_systems(zctx, nc):
    """the tail guard alone, a second wave, several workgroups"""
    s = C.random_system(nc)
    n = C.domain_size(nc) + 3
    _, w, *want = C.expected_cached("random", nc, n)
    sys_ = R1CS.from_csr(*s.csr(), ctx=zctx)
    got = _dev_eval(zctx, sys_, w, n)
    _equal(got, want, "nc = %d" % nc)
    _equal(got, sys_.abc_host(C.witness_words(w), n, check=True), "nc = %d, host twin" % nc)
    # abc_dev: the same through the allocating wrapper
    dev = torch.device("cuda", zctx.device_id)
    a, b, c, d_sum = sys_.abc_dev(zctx, torch.from_numpy(C.witness_words(w).view(np.int64)).to(dev), n, check=True)
    zctx.synchronize()
    h = lambda t: t.cpu().numpy().view(np.uint64)
    _equal((h(a), h(b), h(c), summary_tuple(h(d_sum))), want, "abc_dev")
    sys_.close()


def test_unreduced_witness_words_are_reduced_on_the_device(zctx):
    s = C.random_system(65)
    n = 128
    _, w, *want = C.expected_cached("random", 65, n)
    _equal(_dev_eval(zctx, R1CS.from_csr(*s.csr(), ctx=zctx), [x + G.R if i % 2 else x for i, x in enumerate(w)], n), want, "witness + r")


@pytest.mark.parametrize("kind,arg", [("edge", 0), ("random", 3 * 256 + 1)])
def test_summaries_of_broken_witnesses_from_the_device(zctx, kind, arg):
    s = C.edge_system() if kind == "edge" else C.random_system(arg)
    nc = s.n_constraints
    n = C.domain_size(nc)
    sys_ = R1CS.from_csr(*s.csr(), ctx=zctx)
    fresh = [j for j in range(nc) if any(w == s.fresh_wire(j) for w, _ in s.rows[2 * nc + j])]
    for broken in [(), (0,), (nc - 1,), (0, nc - 1), tuple(fresh[1:-1:3])]:
        _, w, *want = C.expected_cached(kind, arg, n, broken)
        assert want[3] == (len(broken), broken[0] if broken else None)
        _equal(_dev_eval(zctx, sys_, w, n), want, "broken at %s" % (broken,))
    sys_.close()


def test_malformed_device_calls_are_rejected(zctx):
    from zklc_amd import ZklcError
    s = C.random_system(65)
    dev = torch.device("cuda", zctx.device_id)
    sys_ = R1CS.from_csr(*s.csr(), ctx=zctx)
    host_only = R1CS.from_csr(*s.csr())
    d_w = torch.from_numpy(C.witness_words(s.witness).view(np.int64)).to(dev)
    n = 128
    buf = torch.zeros((3, n + 1, 4), dtype=torch.int64, device=dev)
    ws = torch.zeros(sys_.workspace_bytes() + 32, dtype=torch.uint8, device=dev)
    d_sum = torch.zeros(2, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    lib = sys_._lib
    a, b, c = (buf[i].data_ptr() for i in range(3))

    def call(handle=sys_._s, w=d_w.data_ptr(), n=n, a=a, b=b, c=c, flags=1, summary=d_sum.data_ptr(), wsp=ws.data_ptr(), wsb=ws.numel() - 32):
        return lib.zklc_r1cs_abc_dev(zctx._h, zctx.stream_ptr(), handle, w, n, a, b, c, flags, summary, wsp, wsb)
    assert call() == 0
    assert call(n=64) == -1                                   # n < n_constraints
    assert call(flags=3) == -1                                # unknown flag bits
    assert call(summary=None) == -1                           # check without a summary
    assert call(w=None) == -1 and call(b=None) == -1 and call(wsp=None) == -1
    assert call(w=d_w.data_ptr() + 8) == -1 and call(c=c + 8) == -1 and call(wsp=ws.data_ptr() + 8) == -1
    assert call(wsb=sys_.workspace_bytes() - 1) == -1         # short workspace
    assert call(handle=host_only._s) == -1                    # a system created without a context
    zctx.synchronize()
    with pytest.raises(ZklcError):
        host_only.abc_dev(zctx, d_w, n)
    zctx.synchronize()


RS = (0x1111222233334444, 0x5555666677778888)


@pytest.fixture(scope="module")
def chain(zctx):
    """the 100-constraint square chain under the key of tests/test_gpu_groth16.py (domain 128) with its constraint system resident,
    one satisfying witness and the oracle's proof words for it -- the oracle's setup and proof are minutes of Python integers
    together with nothing to spare, so they are made ONCE and shared by the tests below"""
    n_pub = 3
    r1cs, wit = G.square_chain_r1cs(100, n_public=n_pub)
    pk, _ = G.setup(r1cs, n_pub, (0x1234567891, 0xabcdef12345, 0x777766665555, 0x3133731337, 0x42424242))
    assert pk["n"] == 128
    good = wit([11, 22, 33], 7)
    want = G.proof_to_uint256x8(G.prove(pk, r1cs, good, *RS))
    sys_ = R1CS.from_rows(*r1cs, pk["n_wires"], ctx=zctx)
    prover = Groth16Prover(zctx, pk, sys_)
    yield r1cs, pk, prover, good, want
    prover.close()
    sys_.close()


def test_prove_witness_equals_the_oracle_and_prove(zctx, chain):
    r1cs, pk, prover, good, want = chain
    assert prover.prove_witness(good, *RS) == want, "prove_witness differs from the oracle prover"
    print("groth16 prove_witness (n = 128): ms", prover.last_ms)
    assert prover.last_ms["r1cs_eval_device"] > 0 and prover.last_ms["r1cs_check"] is True
    assert prover.prove_witness(good, *RS, check=False) == want
    assert prover.prove(good, G.abc_evaluations(r1cs, good, pk["n"]), *RS) == want
    assert "r1cs_eval_device" not in prover.last_ms


def test_a_broken_witness_raises_and_the_prover_recovers(zctx, chain):
    r1cs, pk, prover, good, want = chain
    base = 1 + 3
    for j, count in [(99, 1), (0, 2), (41, 2)]:
        w = list(good)
        w[base + j + 1] = (w[base + j + 1] + 1) % G.R          # x_(j+1): the output of constraint j and the input of j + 1
        with pytest.raises(UnsatisfiedConstraint) as e:
            prover.prove_witness(w, *RS)
        assert (e.value.index, e.value.count) == (j, count)
        assert isinstance(e.value, ValueError)
        # the same object proves the next valid witness: the three streams were drained before the exception left
        assert prover.prove_witness(good, *RS) == want
    # without the check the broken witness is proven as it is, like `prove` does
    assert prover.prove_witness(w, 5, 6, check=False) == prover.prove(w, G.abc_evaluations(r1cs, w, pk["n"]), 5, 6)
    bare = Groth16Prover(zctx, pk)
    with pytest.raises(ValueError):
        bare.prove_witness(good, 1, 2)
    bare.close()
