"""The Poseidon-BN254 Merkle tree kernels of csrc/poseidon_bn254.hip against the oracle's C tree builder
(oracle/c/poseidon_bn254_oracle.c, pinned to oracle/poseidon_bn254.py and the golden proofs by tests/test_oracle_c_bn254.py):
every digest of every level, at the sizes where the dispatch changes kernels -- the wrap's own trees of 2^15 leaves among them,
which the one-lane leaf kernel hashes -- for every width residue, under every ZKLC_BN254_COOP setting, with edge-valued leaves
and with a strided input.  The cases and the restated dispatch rule are in tests/bn254_merkle_cases.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bn254_merkle_cases as MC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300


@pytest.mark.parametrize("case,leaf_kernel,lane_levels", MC.THRESHOLD_CASES, ids=lambda v: MC.name(v) if isinstance(v, MC.Case) else None)
def test_full_trees_at_the_dispatch_thresholds(zctx, case, leaf_kernel, lane_levels):
    """default dispatch.  Which kernels a case reaches follows from the rule (item count against 2^14), asserted here beside the
    table of bn254_merkle_cases.py: (4, 15, 4) takes the one-lane leaf kernel and four-lane level kernels only, (4, 16, 4) one
    one-lane level."""
    assert os.environ.get("ZKLC_BN254_COOP") is None, "the threshold cases are meant for the default dispatch"
    n = 1 << case.log_leaves
    assert leaf_kernel == ("coop" if n <= 1 << 14 else "lane")
    assert lane_levels == sum(1 for l in range(case.log_leaves - case.cap) if (n >> (l + 1)) > 1 << 14)
    assert MC.dispatch(case) == (leaf_kernel, ["lane"] * lane_levels + ["coop"] * (case.log_leaves - case.cap - lane_levels))
    cap, levels = zctx.bn254_merkle_commit(MC.matrix(case), case.cap)
    diff = MC.first_difference(case, levels, MC.reference(case))
    assert diff is None, diff
    assert cap.shape == (1 << case.cap, 4)


@pytest.mark.parametrize("case", MC.STRIDED_CASES, ids=MC.name)
def test_strided_input_gives_the_packed_tree(zctx, case):
    """zklc_bn254_merkle_commit_dev with a column stride of 2^log_leaves + 24 words and 0xFF bytes between the columns: the tree of
    the packed call, which is the oracle's"""
    import torch
    n, stride = 1 << case.log_leaves, (1 << case.log_leaves) + MC.STRIDE_PAD
    mat = MC.matrix(case)
    padded = np.full((case.width, stride), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    padded[:, :n] = mat
    d_mat = torch.from_numpy(padded.view(np.int64)).cuda()
    words = zctx.gl_merkle_tree_words(case.log_leaves, case.cap)
    d_tree = torch.zeros(words, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()          # the upload and the fill are done before the context's own stream reads and writes
    zctx.bn254_merkle_commit_dev(d_mat, stride, case.log_leaves, case.width, case.cap, d_tree)
    zctx.synchronize()
    got = MC.split_levels(case, d_tree.cpu().numpy().view(np.uint64))
    _, packed = zctx.bn254_merkle_commit(mat, case.cap)
    diff = MC.first_difference(case, got, packed)
    assert diff is None, "strided against packed: " + diff
    diff = MC.first_difference(case, got, MC.reference(case))
    assert diff is None, diff


def test_width_and_dispatch_sweep_in_child_processes(tmp_path):
    """The library reads ZKLC_BN254_COOP once per process: one child per setting -- the default, 0 (one lane per permutation for
    everything) and 3 (the switch to four lanes happens inside a tree, at 8 items) -- builds every tree of MC.CHILD_CASES (widths
    1..28, 32, 36, 85, 135; widths 4 and 10 at every height from a single leaf on, with a cap of height 0 and one as tall as the
    tree; leaves of all P - 1, all 0 and the cycled edge alphabet) and writes the whole trees to a file; every level of every tree
    is the oracle's."""
    for s in MC.SETTINGS[1:]:       # what the settings are meant to reach, from the restated rule
        kinds = {k for c in MC.CHILD_CASES for k in [MC.dispatch(c, s)[0]] + MC.dispatch(c, s)[1]}
        assert kinds == ({"lane"} if s == "0" else {"lane", "coop"})
    assert all(MC.dispatch(c)[0] == "coop" and set(MC.dispatch(c)[1]) <= {"coop"} for c in MC.CHILD_CASES)
    want = {MC.name(c): MC.reference(c) for c in MC.CHILD_CASES}
    procs = []
    try:
        for s in MC.SETTINGS:       # three children: with this process four of the processes that may have the GPU open at once
            out = str(tmp_path / ("trees_%s.npz" % ("default" if s is None else s)))
            env = {k: v for k, v in os.environ.items() if k != "ZKLC_BN254_COOP"}
            if s is not None:
                env["ZKLC_BN254_COOP"] = s
            code = MC.CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "out": out}
            procs.append((s, out, subprocess.Popen([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                                   text=True, env=env, cwd=ROOT)))
        problems = []
        for s, out, p in procs:
            # a child that faults, aborts or runs into its time limit ends the test here: nothing more is started on the GPU, and
            # `finally` ends the children that still run
            so, se = p.communicate(timeout=CHILD_TIMEOUT)
            assert p.returncode == 0, ("ZKLC_BN254_COOP=%r" % s, p.returncode, se[-2000:])
            assert "DONE %d" % len(MC.CHILD_CASES) in so, (s, so[-500:])
            with np.load(out) as trees:
                assert sorted(trees.files) == sorted(want)
                for c in MC.CHILD_CASES:
                    diff = MC.first_difference(c, MC.split_levels(c, trees[MC.name(c)]), want[MC.name(c)])
                    if diff:
                        problems.append("ZKLC_BN254_COOP=%r (leaves %s, levels %s): %s" % ((s,) + MC.dispatch(c, s) + (diff,)))
        assert not problems, "\n".join(problems[:20] + ["%d trees differ" % len(problems)])
    finally:
        for _, _, p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
