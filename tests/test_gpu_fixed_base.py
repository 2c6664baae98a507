"""The batched fixed-base multiplication on the GPU (zklc_bn254_g{1,2}_fixed_mul_dev over a table the GPU built:
csrc/bn254_fixed_mul.hip) against the host twin and against oracle/bn254.py's Python integers (tests/fixed_base_cases.py), word for
word: the edge scalars of every window width, zero scalars at every place of the groups that share an inversion, sizes around a
group, a wave and a workgroup of either stage, and the c = 16 table through single-digit scalars.  No tolerance anywhere."""
import ctypes

import numpy as np
import pytest
import torch

import fixed_base_cases as C
from zklc_amd import fixed_base as FB

pytestmark = pytest.mark.gpu

INVALID = -1
FF = -1               # int64 with every bit set
WINDOWS = (5, 13, 16)
SIZES = (1, 63, 64, 65, 257, 4099)       # 4099: a second workgroup of the inversion stage (257 groups)


@pytest.fixture(scope="module")
def dev_tables(zctx):
    t = {(g, c): FB.FixedBase(zctx, g, None, c) for g in (C.G1, C.G2) for c in WINDOWS}
    yield t
    for x in t.values():
        x.close()


@pytest.fixture(scope="module")
def host_tables():
    """no c = 16 table on the host: the c = 13 one gives the same words"""
    t = {(g, c): FB.FixedBase(None, g, None, 13 if c == 16 else c) for g in (C.G1, C.G2) for c in WINDOWS if c != 13}
    for g in (C.G1, C.G2):
        t[g, 13] = t[g, 16]
    yield t
    for x in set(t.values()):
        x.close()


def _dev_mul(zctx, t, scalars):
    """the kernels into buffers filled with 0xFF -> (words as a uint64 array, summary)"""
    dev = torch.device("cuda", zctx.device_id)
    n = len(scalars)
    d_s = torch.from_numpy(C.scalar_words(scalars).view(np.int64)).to(dev)
    words = torch.full((n, t.width), FF, dtype=torch.int64, device=dev)
    summary = torch.full((2,), 7, dtype=torch.int64, device=dev)
    ws = torch.empty(t.workspace_bytes(n), dtype=torch.uint8, device=dev)
    torch.cuda.current_stream(dev).synchronize()
    t.enqueue(d_s, words, summary, ws)
    zctx.synchronize()
    return words.cpu().numpy().view(np.uint64), FB.summary_tuple(summary.cpu().numpy().view(np.uint64))


def _rows_equal(got, want, what):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, "%s: point %d is %s, expected %s" % (what, bad[0], got[bad[0]], want[bad[0]])
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("c", WINDOWS)
@pytest.mark.parametrize("group", [C.G1, C.G2])
def test_kernels_equal_the_host_twin_and_the_oracle_on_the_edge_scalars(zctx, dev_tables, host_tables, group, c):
    mine = C.edge_scalars(c) + C.random_scalars(24, 7)
    scalars = mine + C.oracle_scalars(group)
    got, summary = _dev_mul(zctx, dev_tables[group, c], scalars)
    want, host_summary = host_tables[group, c].mul_host(C.scalar_words(scalars))
    _rows_equal(got, want, "kernels against the host twin, c = %d" % c)
    _rows_equal(got[len(mine):], C.expected_words(group, scalars[len(mine):]), "kernels against the oracle, c = %d" % c)
    assert summary == host_summary == C.expected_summary(scalars)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("group", [C.G1, C.G2])
def test_zero_scalars_inside_the_inversion_groups(zctx, dev_tables, host_tables, group, n):
    scalars = C.zero_placements(group, n)
    want = C.expected_words(group, scalars)
    host, host_summary = host_tables[group, 5].mul_host(C.scalar_words(scalars))
    _rows_equal(host, want, "host twin, n = %d" % n)
    for c in WINDOWS:
        got, summary = _dev_mul(zctx, dev_tables[group, c], scalars)
        _rows_equal(got, want, "n = %d, c = %d" % (n, c))
        assert summary == host_summary == C.expected_summary(scalars) and summary[0] >= 1
    if n == 1:
        got, summary = _dev_mul(zctx, dev_tables[group, 16], [C.R - 1])
        _rows_equal(got, C.expected_words(group, [C.R - 1]), "one scalar")
        assert summary == (0, None)


@pytest.mark.parametrize("group", [C.G1, C.G2])
def test_the_table_the_gpu_built_at_c_16(zctx, dev_tables, group):
    """entry (k, d) = d 2^(16 k) G is what the single-digit scalar d 2^(16 k) reads and nothing else"""
    probes = C.table_probes()
    assert {(0, 1), (0, 0xffff), (15, 1)} <= set(probes) and max(k for k, _ in probes) == C.rows(16) - 1
    scalars = [d << (16 * k) for k, d in probes]
    for (k, d), s in zip(probes, scalars):
        assert s < C.R and [(i, v) for i, v in enumerate(C.digits(s, 16)) if v] == [(k, d)]
    got, summary = _dev_mul(zctx, dev_tables[group, 16], scalars)
    _rows_equal(got, C.expected_words(group, scalars), "c = 16 table")
    assert summary == (0, None)


@pytest.mark.parametrize("group", [C.G1, C.G2])
def test_all_zero_and_empty_batches_and_the_allocating_wrapper(zctx, dev_tables, group):
    t = dev_tables[group, 13]
    got, summary = _dev_mul(zctx, t, [0, C.R] * 40)
    assert not got.any() and summary == (80, 0)
    dev = torch.device("cuda", zctx.device_id)
    words, d_sum, _ = t.mul_dev(torch.zeros((0, 4), dtype=torch.int64, device=dev))
    zctx.synchronize()
    assert words.shape == (0, t.width) and FB.summary_tuple(d_sum.cpu().numpy().view(np.uint64)) == (0, None)
    scalars = [1, 0, C.R - 1, 2]
    words, d_sum, _ = t.mul_dev(torch.from_numpy(C.scalar_words(scalars).view(np.int64)).to(dev))
    zctx.synchronize()
    _rows_equal(words.cpu().numpy().view(np.uint64), C.expected_words(group, scalars), "mul_dev")
    assert FB.summary_tuple(d_sum.cpu().numpy().view(np.uint64)) == (1, 1)


@pytest.mark.parametrize("group", [C.G1, C.G2])
def test_a_base_that_is_not_the_generator(zctx, group):
    base = np.array(C.point_words(group, C.base_point(group, False)), dtype=np.uint64)
    with FB.FixedBase(zctx, group, base, 5) as t:
        got, summary = _dev_mul(zctx, t, C.other_base_scalars(group))
    _rows_equal(got, np.array(C.other_base_points(group), dtype=np.uint64), "base %d x the generator" % C.BASE_MULT[group])
    assert summary == (1, 0)


def test_malformed_device_calls_are_refused_without_a_launch(zctx, dev_tables, host_tables):
    dev = torch.device("cuda", zctx.device_id)
    for group in (C.G1, C.G2):
        t = dev_tables[group, 5]
        n = 20
        d_s = torch.from_numpy(C.scalar_words([3] * (n + 1)).view(np.int64)).to(dev)
        words = torch.full((n + 1, t.width), FF, dtype=torch.int64, device=dev)
        summary = torch.full((2,), 7, dtype=torch.int64, device=dev)
        ws = torch.empty(t.workspace_bytes(n) + 16, dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        need = t.workspace_bytes(n)
        call = lambda tbl, s, k, w, sm, wsp, wsb: t._mul_dev(zctx._h, zctx.stream_ptr(), tbl, s, k, w, sm, wsp, wsb)
        args = (t._t, d_s.data_ptr(), n, words.data_ptr(), summary.data_ptr(), ws.data_ptr(), need)
        bad = [
            args[:6] + (need - 1,),                                            # short workspace
            args[:1] + (d_s.data_ptr() + 8,) + args[2:],                       # misaligned pointers
            args[:3] + (words.data_ptr() + 8,) + args[4:],
            args[:5] + (ws.data_ptr() + 8, need),
            args[:4] + (summary.data_ptr() + 4,) + args[5:],
            args[:1] + (None,) + args[2:],                                     # missing pointers
            args[:3] + (None,) + args[4:],
            args[:4] + (None,) + args[5:],
            args[:5] + (None, need),
            (None,) + args[1:],                                                # no table
            (dev_tables[1 - group, 5]._t,) + args[1:],                         # a table of the other group
            (host_tables[group, 5]._t,) + args[1:],                            # a table built without a context
            args[:2] + ((1 << 30) + 1,) + args[3:],                            # too many scalars
        ]
        for a in bad:
            assert call(*a) == INVALID, a
        assert t._mul_dev(None, zctx.stream_ptr(), *args) == INVALID           # no context
        zctx.synchronize()
        assert (words.cpu().numpy() == FF).all() and summary.cpu().tolist() == [7, 7], "a refused call launched"
        assert call(*args) == 0
        zctx.synchronize()
        assert (words[n].cpu().numpy() == FF).all() and summary.cpu().tolist() == [0, -1]
        _rows_equal(words[:n].cpu().numpy().view(np.uint64), host_tables[group, 5].mul_host(C.scalar_words([3] * n))[0], "3 G")
    h = ctypes.c_void_p(1)
    lib = dev_tables[C.G1, 5]._lib
    zero = np.zeros(16, dtype=np.uint64)
    for group, base, c in ((2, None, 8), (C.G1, None, 3), (C.G2, None, 17), (C.G1, zero.ctypes.data, 5), (C.G2, zero.ctypes.data, 5)):
        assert lib.zklc_bn254_fixed_base_create(zctx._h, group, base, c, ctypes.byref(h)) == INVALID and not h.value
        h.value = 1
