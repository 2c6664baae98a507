"""zklc_bn254_fixed_base_create without a context and zklc_bn254_g{1,2}_fixed_mul_host (no GPU): the host twin of the batched
fixed-base multiplication -- the lane functions of csrc/bn254_fixed_mul.cuh compiled for the host -- against oracle/bn254.py's
double-and-add in Python integers (tests/fixed_base_cases.py), word for word.  Every expected point is exact: no tolerance."""
import ctypes
import os

import numpy as np
import pytest

import fixed_base_cases as C
from conftest import ROOT
from zklc_amd import _lib
from zklc_amd import fixed_base as FB

INVALID = -1          # ZKLC_ERR_INVALID_ARG
WINDOWS = (5, 13)


@pytest.fixture(scope="module")
def tables():
    t = {(g, c): FB.FixedBase(None, g, None, c) for g in (C.G1, C.G2) for c in WINDOWS}
    yield t
    for x in t.values():
        x.close()


def _rows_equal(got, want, what):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, "%s: point %d is %s, expected %s" % (what, bad[0], got[bad[0]], want[bad[0]])
    assert got.tobytes() == want.tobytes()


def test_constants_are_the_library_s():
    src = open(os.path.join(ROOT, "zk-light-client-implementation_amd", "csrc", "bn254_fixed_mul.cuh")).read()
    assert "#define FBM_INV_GROUP %du" % C.INV_GROUP in src and C.INV_GROUP == FB.INV_GROUP
    assert "#define FBM_SCALAR_BITS %du" % C.SCALAR_BITS in src
    lib = _lib.load()
    for g, rec, limbs in ((C.G1, 64, 10), (C.G2, 128, 20)):
        for c in (4, 5, 13, 16):
            assert lib.zklc_bn254_fixed_base_table_bytes(g, c) == C.rows(c) * ((1 << c) - 1) * rec
        assert lib.zklc_bn254_fixed_mul_workspace_bytes(g, 1000) == 5 * limbs * 4 * 1000
        assert lib.zklc_bn254_fixed_mul_workspace_bytes(g, (1 << 30) + 1) == 0
    assert lib.zklc_bn254_fixed_base_table_bytes(2, 8) == 0 and lib.zklc_bn254_fixed_base_table_bytes(0, 17) == 0
    assert lib.zklc_bn254_fixed_base_table_bytes(C.G1, 16) == 67107840 and lib.zklc_bn254_fixed_base_table_bytes(C.G2, 16) == 134215680


@pytest.mark.parametrize("c", [4, 5, 13, 16])
def test_edge_scalars_have_every_case(c):
    e = C.edge_scalars(c)
    n, top = C.rows(c), (1 << c) - 1
    assert {0, 1, 2, C.R - 1, C.R - 2, C.R, C.R + 1, (1 << 256) - 1} <= set(e)
    d = [C.digits(s, c) for s in e]
    for k in range(1, n):
        assert any(x[k] == 1 and sum(x) == 1 for x in d), "2^(c k) alone, window %d" % k
        assert any(all(v == top for v in x[:k]) and not any(x[k:]) for x in d), "a borrow out of window %d" % k
    for k in range(n - 1):
        assert any(x[k] == top and sum(x) == top for x in d), "the largest digit alone in window %d" % k
    assert any(x[n - 1] == (C.R - 1) >> (c * (n - 1)) and not any(x[:n - 1]) for x in d)
    for s in e:
        assert sum(v << (c * k) for k, v in enumerate(C.digits(s, c))) == s % C.R


@pytest.mark.parametrize("group", [C.G1, C.G2])
def test_host_twin_equals_the_oracle_and_itself_across_windows(tables, group):
    """every edge scalar of both windows and random ones through BOTH tables: the digits differ, the words must not; the oracle's
    points for its share of them (its budget); the summary counts 0 and r"""
    scalars = C.edge_scalars(5) + C.edge_scalars(13) + C.random_scalars(24, 7) + C.oracle_scalars(group)
    w5, s5 = tables[group, 5].mul_host(C.scalar_words(scalars), nthreads=3)
    w13, s13 = tables[group, 13].mul_host(C.scalar_words(scalars))
    _rows_equal(w5, w13, "c = 5 against c = 13")
    assert s5 == s13 == C.expected_summary(scalars)
    k = len(scalars) - len(C.oracle_scalars(group))
    _rows_equal(w13[k:], C.expected_words(group, scalars[k:]), "c = 13 against the oracle")
    # the same scalar gives the same words wherever it stands and whatever shares its inversion
    w1, _ = tables[group, 5].mul_host(C.scalar_words(scalars[::-1]), nthreads=1)
    _rows_equal(w1[::-1].copy(), w5, "reversed batch")


@pytest.mark.parametrize("group", [C.G1, C.G2])
@pytest.mark.parametrize("n", C.PLACEMENT_SIZES)
def test_zero_scalars_inside_the_inversion_groups(tables, group, n):
    scalars = C.zero_placements(group, n)
    for c in WINDOWS:
        w, summary = tables[group, c].mul_host(C.scalar_words(scalars), nthreads=2)
        _rows_equal(w, C.expected_words(group, scalars), "n = %d, c = %d" % (n, c))
        assert summary == C.expected_summary(scalars) and summary[0] >= 1
    if n == 1:
        w, summary = tables[group, 5].mul_host(C.scalar_words([C.R - 1]))
        _rows_equal(w, C.expected_words(group, [C.R - 1]), "one scalar")
        assert summary == (0, None)


@pytest.mark.parametrize("group", [C.G1, C.G2])
def test_all_zero_batch_and_empty_batch(tables, group):
    w, summary = tables[group, 5].mul_host(C.scalar_words([0, C.R] * 20))
    assert not w.any() and summary == (40, 0)
    w, summary = tables[group, 5].mul_host(np.zeros((0, 4), dtype=np.uint64))
    assert w.shape[0] == 0 and summary == (0, None)


@pytest.mark.parametrize("group", [C.G1, C.G2])
def test_a_base_that_is_not_the_generator(group):
    base = np.array(C.point_words(group, C.base_point(group, False)), dtype=np.uint64)
    with FB.FixedBase(None, group, base, 5) as t:
        w, summary = t.mul_host(C.scalar_words(C.other_base_scalars(group)))
    want = np.array(C.other_base_points(group), dtype=np.uint64)
    _rows_equal(w, want, "base %d x the generator" % C.BASE_MULT[group])
    assert summary == (1, 0)
    # the generator handed over as words is the NULL base
    gen = np.array(C.point_words(group, C.base_point(group)), dtype=np.uint64)
    with FB.FixedBase(None, group, gen, 5) as t:
        w, _ = t.mul_host(C.scalar_words([1, 2, C.R - 1]))
    _rows_equal(w, C.expected_words(group, [1, 2, C.R - 1]), "the generator as words")


def test_outputs_are_written_in_full_and_malformed_calls_are_refused(tables):
    lib = _lib.load()
    scalars = C.scalar_words([0, 1, C.R, 2])
    for group, fn in ((C.G1, lib.zklc_bn254_g1_fixed_mul_host), (C.G2, lib.zklc_bn254_g2_fixed_mul_host)):
        t = tables[group, 5]
        width = t.width
        words = np.full((5, width), (1 << 64) - 1, dtype=np.uint64)
        summary = np.full(2, 7, dtype=np.uint64)
        assert fn(t._t, scalars.ctypes.data, 4, 1, words.ctypes.data, summary.ctypes.data) == 0
        _rows_equal(words[:4], C.expected_words(group, [0, 1, C.R, 2]), "0xFF-filled output")
        assert (words[4] == (1 << 64) - 1).all() and summary.tolist() == [2, 0]
        before = words.copy()
        call = lambda *a: fn(*a)
        assert call(None, scalars.ctypes.data, 4, 1, words.ctypes.data, summary.ctypes.data) == INVALID           # no table
        assert call(tables[1 - group, 5]._t, scalars.ctypes.data, 4, 1, words.ctypes.data, summary.ctypes.data) == INVALID   # other group
        assert call(t._t, None, 4, 1, words.ctypes.data, summary.ctypes.data) == INVALID                           # missing pointers
        assert call(t._t, scalars.ctypes.data, 4, 1, None, summary.ctypes.data) == INVALID
        assert call(t._t, scalars.ctypes.data, 4, 1, words.ctypes.data, None) == INVALID
        assert call(t._t, scalars.ctypes.data + 8, 3, 1, words.ctypes.data, summary.ctypes.data) == INVALID        # misaligned
        assert call(t._t, scalars.ctypes.data, 4, 1, words.ctypes.data + 8, summary.ctypes.data) == INVALID
        assert call(t._t, scalars.ctypes.data, (1 << 30) + 1, 1, words.ctypes.data, summary.ctypes.data) == INVALID
        assert words.tobytes() == before.tobytes(), "a refused call wrote"


def test_malformed_tables_are_refused():
    lib = _lib.load()
    h = ctypes.c_void_p(1)
    create = lambda group, base, c: lib.zklc_bn254_fixed_base_create(None, group, base, c, ctypes.byref(h))
    for group, c in ((2, 8), (C.G1, 3), (C.G1, 17), (C.G2, 0)):
        assert create(group, None, c) == INVALID and not h.value
        h.value = 1
    zero = np.zeros(16, dtype=np.uint64)
    assert create(C.G1, zero.ctypes.data, 5) == INVALID and not h.value             # the point at infinity
    assert create(C.G2, zero.ctypes.data, 5) == INVALID
    assert lib.zklc_bn254_fixed_base_create(None, C.G1, None, 5, None) == INVALID
    with pytest.raises(ValueError):
        FB.FixedBase(None, C.G1, np.zeros(16, dtype=np.uint64), 5)                  # G2 words for a G1 table: Python's check
    t = FB.FixedBase(None, C.G1, None, 4)
    t.close()
    with pytest.raises(ValueError):
        t.mul_host(C.scalar_words([1]))
    lib.zklc_bn254_fixed_base_destroy(None)
