"""The lean arithmetic forms (ZKLC_LEAN_ARITH, on by default; csrc/goldilocks_ntt_group.cuh, csrc/plonky2_perm_terms.cuh) on the GPU,
against the oracle's C restatement: transforms whose last (DIF) or first (DIT) group is the unit-twiddle group of every size,
the single-group case where that group is also the first one, two-pass transforms, extensions down to 2^0 -> 2^3 (one group that
is zero-aware and unit at once), and proof bytes under both settings of the switch."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import devsim_vectors as DV
from oracle import cport
from oracle import goldilocks as gl

pytestmark = pytest.mark.gpu

P = gl.P
INV, IN_BR, OUT_BR = 1, 2, 4


def _operands(rng, shape):
    """uniform field elements with the canonical edge operands of tests/devsim_vectors.py sprinkled in (a quarter of the positions)"""
    a = rng.integers(0, 2**64, size=shape, dtype=np.uint64)
    a = np.where(a >= np.uint64(P), a - np.uint64(P), a)
    edge = np.array(DV.CANON, dtype=np.uint64)
    pick = rng.integers(0, 4 * len(edge), size=shape)
    return np.where(pick < len(edge), edge[pick % len(edge)], a)


def _bitrev(n):
    bits = n.bit_length() - 1
    return np.array([int(format(i, "0%db" % bits)[::-1], 2) if bits else 0 for i in range(n)])


_NTT_CASES = {}


def _ntt_case(log_n):
    """operands and the oracle's forward and inverse transforms, computed once per size"""
    if log_n not in _NTT_CASES:
        a = _operands(np.random.default_rng(700 + log_n), (3, 1 << log_n))
        a[0, :] = np.uint64(P - 1)                                   # a row of one edge value
        _NTT_CASES[log_n] = (a, cport.gl_ntt(a, nthreads=4), cport.gl_ntt(a, inverse=True, nthreads=4), _bitrev(1 << log_n))
    return _NTT_CASES[log_n]


@pytest.mark.parametrize("flags", [0, INV, IN_BR, OUT_BR, INV | IN_BR, INV | OUT_BR])
@pytest.mark.parametrize("log_n", [1, 2, 3, 4, 5, 6, 13, 14])
def test_ntt_matches_the_oracle(zctx, log_n, flags):
    a, fwd, inv, br = _ntt_case(log_n)
    want = inv if flags & INV else fwd
    got = zctx.gl_ntt(a[:, br] if flags & IN_BR else a, flags=flags)
    assert got.max() < P
    assert np.array_equal(got, want[:, br] if flags & OUT_BR else want)


@pytest.mark.parametrize("out_br", [False, True])
@pytest.mark.parametrize("log_n,rate_bits", [(0, 3), (1, 3), (2, 3), (5, 3), (10, 3), (11, 3)])
def test_lde_matches_the_oracle(zctx, log_n, rate_bits, out_br):
    c = _operands(np.random.default_rng(800 + log_n), (3, 1 << log_n))
    want = cport.gl_lde(c, rate_bits, 7, nthreads=4)
    got = zctx.gl_lde(c, rate_bits, 7, flags=OUT_BR if out_br else 0)
    assert got.max() < P
    assert np.array_equal(got, want[:, _bitrev(1 << (log_n + rate_bits))] if out_br else want)


def partial_chunk_circuit():
    """2^5 rows of the recursion gate mix over the standard 135-wire configuration with 77 routed wires instead of 80: the
    configuration leaves the number free, and 77 = 9 * 8 + 5 makes the last chunk of the permutation argument a partial one"""
    from zklc_amd.plonky2 import synthetic as SY, standard_recursion_config
    cfg = standard_recursion_config()
    cfg["num_routed_wires"] = 77
    assert cfg["num_routed_wires"] % cfg["max_quotient_degree_factor"] != 0
    return SY.synthetic_circuit(5, cfg, SY.recursion_shape_mix(cfg), num_public_inputs=8, seed=7)


_CHILD = r'''
import hashlib, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import zklc_amd
from zklc_amd.plonky2 import HASH_GL
from test_gpu_plonky2 import _synthetic
from test_gpu_lean_arith import partial_chunk_circuit
with zklc_amd.Context(0) as ctx:
    for name, (data, wires, pis) in (("ed25519", _synthetic("ed25519", 13, seed=5, npi=16)), ("partial", partial_chunk_circuit())):
        prover = data.prover(ctx, HASH_GL)
        print("DIGEST %%s %%s" %% (name, hashlib.sha256(prover.prove_bytes(wires, pis)).hexdigest()))
        prover.close()
'''


def test_proof_bytes_equal_the_c_prover_under_both_settings():
    """The library reads ZKLC_LEAN_ARITH once per process: one fresh child per setting, one after the other, proves the 2^13 x 234
    slice of the Ed25519 shape and the tiny circuit with a partial last chunk; every digest must be the C prover's."""
    from test_gpu_plonky2 import _synthetic
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    want = {}
    for name, (data, wires, pis) in (("ed25519", _synthetic("ed25519", 13, seed=5, npi=16)), ("partial", partial_chunk_circuit())):
        want[name] = hashlib.sha256(cport.plonky2_prove(data, wires, pis)[0]).hexdigest()
    code = _CHILD % {"root": root, "tests": os.path.join(root, "tests")}
    for setting in (None, "0"):
        env = {k: v for k, v in os.environ.items() if k != "ZKLC_LEAN_ARITH"}
        if setting is not None:
            env["ZKLC_LEAN_ARITH"] = setting
        run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=root, timeout=900)
        assert run.returncode == 0, (setting, run.stderr[-2000:])
        got = dict(ln.split()[1:3] for ln in run.stdout.splitlines() if ln.startswith("DIGEST "))
        assert got == want, "proof bytes under ZKLC_LEAN_ARITH=%r differ from the C prover's" % (setting,)
