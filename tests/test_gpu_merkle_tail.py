"""The tail of a Goldilocks Merkle tree, one lane per permutation (gl_merkle_tail_kernel, csrc/gl_merkle_plan.h): every level of
the tree against the oracle's C restatement at the shapes where the plan changes kernels or launches.  The switch is read once per
process, so the other settings run in child processes: ZKLC_MERKLE_TAIL=full (the tail kernel down to 16 parents, lane-per-leaf
from 64 leaves: all shapes), =coop (the cooperative kernels only: two shapes), and proof bytes under all three."""
import hashlib
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from oracle import cport

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (width, log_leaves, cap): no-op leaves and no level at all; a single level; trees smaller than one workgroup (512 digests);
# exactly one workgroup and two workgroups joined by a second launch; the cap reached in the middle of a launch; the hand-over
# from the per-level kernel at 2^15, 2^16 and 2^17 leaves (the only launches of the tail kernel by default: three levels, then
# the cooperative subtrees).  The last three rows: 256, 512 and 1024 children down to the root (half a workgroup, one, two).
SHAPES = [(3, 6, 0), (5, 6, 6), (5, 7, 0), (9, 9, 8), (9, 10, 4), (135, 11, 4), (9, 13, 4), (9, 14, 0), (5, 15, 4), (5, 16, 0), (5, 17, 4),
          (9, 8, 0), (9, 9, 0), (9, 10, 0)]
COOP_SHAPES = [(9, 10, 4), (5, 15, 4)]


def _matrix(width, log_leaves):
    return np.random.default_rng(1000 * width + log_leaves).integers(0, P, size=(width, 1 << log_leaves), dtype=np.uint64)


def _assert_levels(got, want, what):
    assert len(got) == len(want), what
    for l, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), "%s: level %d differs" % (what, l)


@pytest.mark.parametrize("width,log_leaves,cap", SHAPES)
def test_every_level_matches_the_oracle(zctx, width, log_leaves, cap):
    mat = _matrix(width, log_leaves)
    cap_gpu, levels = zctx.gl_merkle_commit(mat, cap)
    want = cport.gl_merkle_commit(mat, cap, nthreads=4)
    assert len(want) == log_leaves - cap + 1
    _assert_levels(levels, want, (width, log_leaves, cap))
    assert np.array_equal(cap_gpu, want[-1])


@pytest.mark.parametrize("log_leaves", [9, 13])
@pytest.mark.parametrize("width,cap", [(5, 0), (9, 4)])
def test_edge_leaves(zctx, log_leaves, width, cap):
    """the alphabet of test_merkle_commit_edge_leaves: devsim_vectors.CANON, a column of p - 1, zeros in every other leaf's last word"""
    import devsim_vectors as DV
    rng = random.Random(width * 7 + cap + log_leaves)
    mat = np.array([[rng.choice(DV.CANON) for _ in range(1 << log_leaves)] for _ in range(width)], dtype=np.uint64)
    mat[0, :] = P - 1
    mat[width - 1, 1::2] = 0
    _, levels = zctx.gl_merkle_commit(mat, cap)
    _assert_levels(levels, cport.gl_merkle_commit(mat, cap, nthreads=4), (width, log_leaves, cap))


_MERKLE_CHILD = r'''
import hashlib, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import zklc_amd
from test_gpu_merkle_tail import _matrix
with zklc_amd.Context(0) as ctx:
    for width, log_leaves, cap in %(shapes)r:
        _, levels = ctx.gl_merkle_commit(_matrix(width, log_leaves), cap)
        print("LEVELS %%d %%d %%d %%s" %% (width, log_leaves, cap, " ".join(hashlib.sha256(l.tobytes()).hexdigest() for l in levels)))
'''


@pytest.mark.parametrize("setting,shapes", [("full", SHAPES), ("coop", COOP_SHAPES)])
def test_the_other_forms_stay_selectable(setting, shapes):
    """ZKLC_MERKLE_TAIL=full runs the tail kernel down to 16 parents (partly filled waves, a second launch of one workgroup, the cap in
    the middle of a launch) and hashes leaves one lane each from 64 leaves; =coop restores the cooperative kernels for everything
    of <= 2^14 nodes.  One child per setting, every level of every shape."""
    env = dict(os.environ, ZKLC_MERKLE_TAIL=setting)
    code = _MERKLE_CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "shapes": shapes}
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    got = {tuple(int(x) for x in ln.split()[1:4]): ln.split()[4:] for ln in run.stdout.splitlines() if ln.startswith("LEVELS ")}
    assert sorted(got) == sorted(shapes)
    for shape in shapes:
        want = cport.gl_merkle_commit(_matrix(shape[0], shape[1]), shape[2], nthreads=4)
        assert got[shape] == [hashlib.sha256(l.tobytes()).hexdigest() for l in want], (setting, shape)


def test_proof_bytes_equal_the_c_prover_under_every_setting():
    """One child per setting (the library reads ZKLC_MERKLE_TAIL once per process), all three at once: the 2^13 x 234 slice of the
    Ed25519 shape, and the 2^5-row circuit, every tree of which is smaller than a workgroup and whose row-major FRI leaves
    (leaf_stride != 1) go through the lane-per-leaf kernel under `full`.  Every digest must be the C prover's."""
    from test_gpu_plonky2 import _synthetic
    from test_gpu_lean_arith import _CHILD, partial_chunk_circuit
    want = {}
    for name, (data, wires, pis) in (("ed25519", _synthetic("ed25519", 13, seed=5, npi=16)), ("partial", partial_chunk_circuit())):
        want[name] = hashlib.sha256(cport.plonky2_prove(data, wires, pis)[0]).hexdigest()
    code = _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    procs = []
    for setting in (None, "full", "coop"):
        env = {k: v for k, v in os.environ.items() if k != "ZKLC_MERKLE_TAIL"}
        if setting is not None:
            env["ZKLC_MERKLE_TAIL"] = setting
        procs.append((setting, subprocess.Popen([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                                                env=env, cwd=ROOT)))
    for setting, p in procs:
        so, se = p.communicate(timeout=900)
        assert p.returncode == 0, (setting, se[-2000:])
        got = dict(ln.split()[1:3] for ln in so.splitlines() if ln.startswith("DIGEST "))
        assert got == want, "proof bytes under ZKLC_MERKLE_TAIL=%r differ from the C prover's" % (setting,)
