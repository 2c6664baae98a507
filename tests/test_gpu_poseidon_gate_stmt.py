"""ZKLC_P2_POSEIDON_GATE=stmt on the device: the evaluator of the Poseidon gate built from generated statements
(p2_eval_poseidon_stmt: the hash kernel's full-round statements and the statement of the lazy partial block with the wires as
operands).  Part 1: the gate alone, one row per lane in a kernel of its own (tests/poseidon_gate_dev), against the oracle's evaluator
and against the `loose` form on the device.  Part 2: proof bytes -- one child process per setting (the switches are read once per
process) proves the 2^13 x 234 slice of the Ed25519 shape and a recursion-shaped 2^12 x 135 circuit in which Poseidon gates are most
of the rows and share their selector with other gates; every setting must give the C prover's bytes."""
import ctypes
import hashlib
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import poseidon_gate_vectors as PV
from oracle import plonky2_gates as OG

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STMT, LOOSE = 120, 110


@pytest.fixture(scope="module")
def dev():
    import zklc_amd  # noqa: F401  (first: the package's hardware-queue setting applies to this process)
    b = importlib.import_module("zk-light-client-implementation_amd.build")
    if os.path.exists(b.HIPCC) and not b.poseidon_gate_dev_is_current():
        b.build_poseidon_gate_dev(verbose=False)
    if not os.path.exists(b.PGD_LIB):
        pytest.fail("tests/poseidon_gate_dev/libposeidon_gate_dev.so is missing and there is no hipcc to build it: run __graft_entry__.build()")
    lib = ctypes.CDLL(b.PGD_LIB)
    lib.pgd_eval.restype = ctypes.c_int
    lib.pgd_eval.argtypes = [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32]
    return lib


@pytest.fixture(scope="module")
def gate_rows():
    rows = PV.rows(extra=6)
    assert len(rows) == 150 and len(rows) % 64      # the last wave is partly filled
    return rows


def _eval(dev, code, rows, alphas):
    wa = np.ascontiguousarray(np.array([r for _, r in rows], dtype=np.uint64).reshape(-1))
    aa = np.array(alphas, dtype=np.uint64)
    out = np.zeros(len(rows) * len(alphas), dtype=np.uint64)
    rc = dev.pgd_eval(code, wa.ctypes.data, aa.ctypes.data, len(alphas), out.ctypes.data, len(rows))
    assert rc == 0, "pgd_eval: HIP error %d" % rc
    return [[int(v) for v in out[len(alphas) * i:len(alphas) * (i + 1)]] for i in range(len(rows))]


@pytest.mark.parametrize("pair", [0, 1], ids=["random_alphas", "alpha_p_minus_1_and_2_pow_32"])
def test_gate_alone_against_the_oracle_and_the_loose_form(dev, gate_rows, pair):
    from zklc_amd.plonky2 import gates as G
    og = OG.gate_from_id(G.PoseidonGate().id())
    alphas = PV.alphas()[pair]
    got = _eval(dev, STMT, gate_rows, alphas)
    assert got == _eval(dev, LOOSE, gate_rows, alphas)
    for i, (expect, r) in enumerate(gate_rows):
        cs = og.eval(OG.BaseK, [], r, [0] * 4)
        assert got[i] == [OG.reduce_with_powers(OG.BaseK, cs, a) for a in alphas], i
        if expect:
            assert (got[i] == [0, 0]) == (expect == 1), i


def test_gate_alone_with_one_challenge(dev, gate_rows):
    """nch = 1: the evaluator feeds both accumulators whatever nch is; only the first is read"""
    a = PV.alphas()[0][:1]
    one = _eval(dev, STMT, gate_rows, a)
    assert one == _eval(dev, LOOSE, gate_rows, a)
    assert one == [g[:1] for g in _eval(dev, STMT, gate_rows, PV.alphas()[0])]


# ------------------------------------------------------------------------------------------------ proof bytes
SETTINGS = [{}, {"ZKLC_P2_POSEIDON_GATE": "stmt"}, {"ZKLC_P2_POSEIDON_GATE": "loose"},
            {"ZKLC_P2_POSEIDON_GATE": "stmt", "ZKLC_P2_QUOTIENT": "fused"}]


def circuits():
    """the Ed25519 slice of test_every_quotient_evaluator_variant_gives_the_same_proof_bytes, and the recursion shape with the
    Poseidon gate's share of the rows raised to two thirds (selector groups as in the reference's recursion circuits)"""
    from zklc_amd.plonky2 import synthetic as SY, gates as G, standard_recursion_config, wide_ecc_config
    ecc = wide_ecc_config()
    ed = SY.synthetic_circuit(13, ecc, SY.ed25519_shape_mix(ecc), num_public_inputs=16, seed=5)
    cfg = standard_recursion_config()
    mix = [(g, 120 if isinstance(g, G.PoseidonGate) else w) for g, w in SY.recursion_shape_mix(cfg)]
    rec = SY.synthetic_circuit(12, cfg, mix, num_public_inputs=11, seed=8)
    assert ed[1].shape == (234, 1 << 13) and rec[1].shape == (135, 1 << 12)
    return [("ed25519_2p13x234", ed), ("recursion_2p12x135", rec)]


_CHILD = r'''
import hashlib, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import zklc_amd
from zklc_amd.plonky2 import HASH_GL
from test_gpu_poseidon_gate_stmt import circuits
with zklc_amd.Context(0) as ctx:
    for name, (data, wires, pis) in circuits():
        prover = data.prover(ctx, HASH_GL)
        print("DIGEST " + name + " " + hashlib.sha256(prover.prove_bytes(wires, pis)).hexdigest())
        prover.close()
'''


def test_every_setting_gives_the_c_provers_bytes(zctx):
    from oracle import cport
    code = _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    keys = sorted({k for s in SETTINGS for k in s})
    procs = []
    for s in SETTINGS:       # four children: with this process five of the processes that may have the GPU open at once
        env = {k: v for k, v in os.environ.items() if k not in keys}
        env.update(s)
        procs.append((s, subprocess.Popen([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env,
                                          cwd=ROOT)))
    try:
        want = {}            # the C prover's bytes, computed on the host while the children prove
        for name, (data, wires, pis) in circuits():
            raw, _ = cport.plonky2_prove(data, wires, pis)
            want[name] = hashlib.sha256(raw).hexdigest()
        for s, p in procs:
            so, se = p.communicate(timeout=600)
            assert p.returncode == 0, (s, se[-2000:])
            got = dict(ln.split()[1:3] for ln in so.splitlines() if ln.startswith("DIGEST "))
            assert got == want, "proof bytes under %r differ from the C prover's" % (s,)
    finally:
        for _, p in procs:   # nothing is left running when an assertion or the host prover fails
            if p.poll() is None:
                p.kill()
                p.wait()
