"""csrc/gl_ntt_plan.h, goldilocks.cuh, goldilocks_ntt_group.cuh + tests/ntt_plan_host/ntt_plan_host_main.cpp and nothing else, as child
processes on the CPU: built once plainly and once with g++ -fsanitize=address,undefined.  The program checks the conditions the pass
kernels rely on for the plan of every transform of 2^1 .. 2^24 elements (both tiles, zero-padded inputs, the radix-2 form), and runs
the plan on the CPU -- an emulation of the shift-twiddle pass kernel over the shared index maps and table layout -- against a plain
radix-2 transform: 2^1 .. 2^16 forward and inverse in both orders, the 8x LDE shapes with and without the zero-aware first group, lean
arithmetic on and off.  Three-pass plans: 2^21 under a pinned 2^12 tile in both builds, and in the plain build 2^23, the smallest
size whose default plan has three passes (about 6 s of the plain run, so no smaller substitute was needed)."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "ntt_plan_host", "ntt_plan_host_main.cpp")
INC = os.path.join(ROOT, "zk-light-client-implementation_amd", "csrc")


@pytest.mark.parametrize("sanitize", [False, True])
def test_the_plan_holds_at_every_size_and_runs_on_the_cpu(tmp_path, sanitize):
    exe = str(tmp_path / "ntt_plan_host_main")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra"] + flags + ["-I", INC, SRC, "-o", exe],
                        capture_output=True, text=True, timeout=600)
    assert cc.returncode == 0 and not cc.stderr.strip(), cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "ntt plan host: ok" in run.stdout, (run.stdout + run.stderr)[-3000:]
