"""csrc/groth16_setup_host.cpp + csrc/r1cs_eval_host.cpp + tests/setup_host/setup_host_main.cpp and nothing else,
g++ -fsanitize=address,undefined, as a child process on the CPU: every malformed call (arrays exactly as long as they claim), then
systems and toxic sets of tests/setup_cases.py against the oracle's words -- the domains 2, 4 and 8, the 100-constraint chain with
every toxic set, and the 4000-constraint chain (the column of 4000 terms; 16 tasks of Lagrange values with an inversion each)."""
import os
import subprocess

import numpy as np

import setup_cases as C
from conftest import ROOT

CASES = [("chain1", t) for t in C.TOXIC_NAMES] + [("chain3", t) for t in C.TOXIC_NAMES] + [("hand5", t) for t in C.TOXIC_NAMES] \
    + [("chain100", t) for t in C.TOXIC_NAMES] + [("chain4000", "base"), ("chain4000", "tau_in_domain")]


def _toxic_words(toxic):
    return np.array([[(int(x) >> (64 * i)) & ((1 << 64) - 1) for i in range(4)] for x in toxic], dtype=np.uint64)


def _write_cases(path):
    with open(path, "wb") as f:
        f.write(np.array([len(CASES)], dtype=np.uint64).tobytes())
        for system_name, toxic_name in CASES:
            sy = C.system(system_name)
            row_ptr, wires, cids, coeffs = sy["csr"]
            f.write(np.array([sy["n_constraints"], sy["n_wires"], len(wires), len(coeffs), sy["n_public"], sy["n"]], dtype=np.uint64).tobytes())
            f.write(row_ptr.tobytes() + wires.astype(np.uint64).tobytes() + cids.astype(np.uint64).tobytes() + coeffs.tobytes())
            f.write(_toxic_words(C.toxic(toxic_name, sy["n"])).tobytes())
            for w in C.expected_words(system_name, toxic_name):
                f.write(w.tobytes())


def test_the_host_files_link_alone_and_are_clean_under_the_sanitizers(tmp_path):
    case = str(tmp_path / "cases.bin")
    _write_cases(case)
    exe = str(tmp_path / "setup_host_main")
    csrc = os.path.join(ROOT, "zk-light-client-implementation_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "setup_host", "setup_host_main.cpp"), os.path.join(csrc, "groth16_setup_host.cpp"),
           os.path.join(csrc, "r1cs_eval_host.cpp")]
    # -g1: line tables for the sanitizers' reports without the variable tracking that dominates the compile time of the inlined field
    # arithmetic; the three files are compiled side by side
    flags = ["-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
             "-pthread", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"]
    objs = [str(tmp_path / ("o%d.o" % i)) for i in range(len(src))]
    jobs = [subprocess.Popen(["g++"] + flags + ["-c", s, "-o", o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            for s, o in zip(src, objs)]
    for j in jobs:
        out = j.communicate(timeout=600)[0]
        assert j.returncode == 0, out[-3000:]
    cc = subprocess.run(["g++"] + flags + objs + ["-o", exe], capture_output=True, text=True, timeout=600)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe, case], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "setup host: ok" in run.stdout, (run.stdout + run.stderr)[-3000:]
