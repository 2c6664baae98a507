"""The lean arithmetic forms of the prover (ZKLC_LEAN_ARITH, on by default) on the host, no GPU: tests/lean_arith_host/lean_arith_main.cpp
-- a stand-alone program over csrc/goldilocks_ntt_group.cuh and csrc/plonky2_perm_terms.cuh, never loaded into Python -- compares

  * the unit-twiddle and canonical-shift NTT groups with gl_ntt_group_plain at J = 0 (G = 1..4, DIF and DIT, forward and inverse,
    and the zero-aware first group ZP = 3 that is also the unit group),
  * the permutation-argument chunk function with the chain it replaces, chunks of 0..8 wires,
  * the batched FRI denominators with gl2_inv per element, batches with one zero, a zero in each set, and all zero,

on the canonical edge operands of tests/devsim_vectors.py and on random ones.  Built plainly and once more under the sanitizers."""
import os
import subprocess

import pytest

import devsim_vectors as DV
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "lean_arith_host", "lean_arith_main.cpp")
CXX = ["g++", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"]


@pytest.mark.parametrize("name,flags", [("plain", ["-O2"]),
                                        ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                       "-fno-omit-frame-pointer"])])
def test_lean_forms_equal_the_forms_they_replace(tmp_path, name, flags):
    exe = str(tmp_path / ("lean_arith_main_" + name))
    cc = subprocess.run(CXX + flags + [SRC, "-o", exe], capture_output=True, text=True, timeout=600)
    assert cc.returncode == 0, cc.stderr[-3000:]
    assert all(0 <= v < DV.P for v in DV.CANON)
    run = subprocess.run([exe, "20261018"] + [str(v) for v in DV.CANON], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "lean arith: ok" in run.stdout, (run.stdout + run.stderr)[-3000:]
