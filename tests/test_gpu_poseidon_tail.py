"""The Poseidon-Goldilocks hash kernels with a four-row last MDS layer (csrc/poseidon_gl.cuh: poseidon_gl_permute_keep, the sponge's
rule, two_to_one; p2_pow_kernel): every level of a tree against the oracle's C restatement at the widths that take each branch of
the sponge's rule -- 5 (final permutation only), 8 (exactly one chunk), 9 (full then one element), 15 (partial then final), 16, 17,
24 and the two widths of a block, 135 and 234 -- on 2^6 and 2^9 leaves, cap heights 0 and 4.  Trees of this size are cooperative
by default, so the per-level plan (ZKLC_NO_COOP_POSEIDON: lane-per-leaf and gl_merkle_level_kernel) and the tail plan
(ZKLC_MERKLE_TAIL=full: lane-per-leaf and gl_merkle_tail_kernel) run in one child process each; the switches are read once per
process.  Proof bytes and the proof-of-work witness of a 2^13 x 234 and a 2^12 x 135 circuit against the C prover, under the default
and under ZKLC_PGL_TAIL=0."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cport

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = [5, 8, 9, 15, 16, 17, 24, 135, 234]
SHAPES = [(w, log_leaves, cap) for log_leaves in (6, 9) for cap in (0, 4) for w in WIDTHS]
PROOFS = [("ed25519", 13), ("recursion", 12)]


def _matrix(width, log_leaves):
    """random words with a column of p - 1, a column of zeros and, in every other leaf, a last word of p - 1"""
    mat = np.random.default_rng(77 * width + log_leaves).integers(0, P, size=(width, 1 << log_leaves), dtype=np.uint64)
    mat[0, :] = P - 1
    mat[width // 2, :] = 0
    mat[width - 1, 1::2] = P - 1
    return mat


def _digests(levels):
    return [hashlib.sha256(np.ascontiguousarray(l).tobytes()).hexdigest() for l in levels]


@pytest.fixture(scope="module")
def oracle_levels():
    """every level of every shape from the C restatement, computed once"""
    return {s: _digests(cport.gl_merkle_commit(_matrix(s[0], s[1]), s[2], nthreads=4)) for s in SHAPES}


@pytest.mark.parametrize("log_leaves,cap", [(6, 0), (6, 4), (9, 0), (9, 4)])
def test_every_level_matches_the_oracle_default_plan(zctx, oracle_levels, log_leaves, cap):
    for w in WIDTHS:
        _, levels = zctx.gl_merkle_commit(_matrix(w, log_leaves), cap)
        assert len(levels) == log_leaves - cap + 1
        assert _digests(levels) == oracle_levels[(w, log_leaves, cap)], (w, log_leaves, cap)


_MERKLE_CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import zklc_amd
from test_gpu_poseidon_tail import SHAPES, _matrix, _digests
with zklc_amd.Context(0) as ctx:
    for width, log_leaves, cap in SHAPES:
        _, levels = ctx.gl_merkle_commit(_matrix(width, log_leaves), cap)
        print("LEVELS %%d %%d %%d %%s" %% (width, log_leaves, cap, " ".join(_digests(levels))))
'''


@pytest.mark.parametrize("plan,env", [("per-level", {"ZKLC_NO_COOP_POSEIDON": "1"}), ("tail", {"ZKLC_MERKLE_TAIL": "full"}),
                                      ("per-level, whole permutations", {"ZKLC_NO_COOP_POSEIDON": "1", "ZKLC_PGL_TAIL": "0"})])
def test_every_level_matches_the_oracle_lane_plans(oracle_levels, plan, env):
    """lane-per-leaf hashing of every width (the sponge's rule on the device) with the per-level kernel, then with the tail kernel
    (from 64 leaves; 2^9 leaves: one workgroup of 256 down to 16 parents, then cooperative); the third child runs the forms that
    ZKLC_PGL_TAIL=0 selects.  One child per setting, every level of every shape."""
    drop = ("ZKLC_NO_COOP_POSEIDON", "ZKLC_MERKLE_TAIL", "ZKLC_PGL_TAIL")
    child_env = dict({k: v for k, v in os.environ.items() if k not in drop}, **env)
    code = _MERKLE_CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=child_env, cwd=ROOT, timeout=600)
    assert run.returncode == 0, (plan, run.stderr[-2000:])
    got = {tuple(int(x) for x in ln.split()[1:4]): ln.split()[4:] for ln in run.stdout.splitlines() if ln.startswith("LEVELS ")}
    assert sorted(got) == sorted(SHAPES)
    for shape in SHAPES:
        assert got[shape] == oracle_levels[shape], (plan, shape)


_PROOF_CHILD = r'''
import hashlib, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import zklc_amd
from zklc_amd.plonky2 import HASH_GL, serialization as S
from test_gpu_plonky2 import _synthetic
with zklc_amd.Context(0) as ctx:
    for shape, degree_bits in %(proofs)r:
        data, wires, pis = _synthetic(shape, degree_bits, seed=5, npi=16)
        prover = data.prover(ctx, HASH_GL)
        raw = prover.prove_bytes(wires, pis)
        pow_witness = S.proof_from_bytes(raw, data.common_data(), HASH_GL)["proof"]["opening_proof"]["pow_witness"]
        print("PROOF %%s %%s %%d" %% (shape, hashlib.sha256(raw).hexdigest(), pow_witness))
        prover.close()
'''


@pytest.fixture(scope="module")
def oracle_proofs():
    """digest of the C prover's bytes and its proof-of-work witness (the lowest one: it scans upwards from zero), computed once"""
    from zklc_amd.plonky2 import HASH_GL, serialization as S
    from test_gpu_plonky2 import _synthetic
    want = {}
    for shape, degree_bits in PROOFS:
        data, wires, pis = _synthetic(shape, degree_bits, seed=5, npi=16)
        raw = cport.plonky2_prove(data, wires, pis)[0]
        want[shape] = (hashlib.sha256(raw).hexdigest(), S.proof_from_bytes(raw, data.common_data(), HASH_GL)["proof"]["opening_proof"]["pow_witness"])
    return want


@pytest.mark.parametrize("setting", [None, "0"], ids=["default", "ZKLC_PGL_TAIL=0"])
def test_proof_bytes_and_pow_witness_equal_the_c_prover(oracle_proofs, setting):
    env = {k: v for k, v in os.environ.items() if k != "ZKLC_PGL_TAIL"}
    if setting is not None:
        env["ZKLC_PGL_TAIL"] = setting
    code = _PROOF_CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "proofs": PROOFS}
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, timeout=900)
    assert run.returncode == 0, (setting, run.stderr[-2000:])
    got = {ln.split()[1]: (ln.split()[2], int(ln.split()[3])) for ln in run.stdout.splitlines() if ln.startswith("PROOF ")}
    assert sorted(got) == sorted(oracle_proofs)
    for shape, (digest, witness) in oracle_proofs.items():
        assert got[shape][1] == witness, "proof-of-work witness of %s under ZKLC_PGL_TAIL=%r is not the C prover's (the lowest)" % (shape, setting)
        assert got[shape][0] == digest, "proof bytes of %s under ZKLC_PGL_TAIL=%r differ from the C prover's" % (shape, setting)
