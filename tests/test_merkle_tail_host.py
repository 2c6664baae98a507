"""csrc/gl_merkle_plan.h + tests/merkle_tail_host/merkle_tail_host_main.cpp and nothing else, as child processes on the CPU: built once
plainly and once with g++ -fsanitize=address,undefined.  The program walks the launch plan of every tree of 2^0 .. 2^24 leaves, every
cap height, every tail workgroup size and every mode: each level produced exactly once and in order, at the layout's offsets, by
grids that cover all children, with no empty launch."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "merkle_tail_host", "merkle_tail_host_main.cpp")
INC = os.path.join(ROOT, "zk-light-client-implementation_amd", "csrc")


@pytest.mark.parametrize("sanitize", [False, True])
def test_the_plan_covers_every_tree(tmp_path, sanitize):
    exe = str(tmp_path / "merkle_tail_host_main")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra"] + flags + ["-I", INC, SRC, "-o", exe],
                        capture_output=True, text=True, timeout=600)
    assert cc.returncode == 0 and not cc.stderr.strip(), cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "merkle tail host: ok" in run.stdout, (run.stdout + run.stderr)[-3000:]
