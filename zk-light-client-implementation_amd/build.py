"""Build libzklc_mi355.so (hipcc, gfx950 only) in-tree.

    python -m zklc_amd.build            # or: python zk-light-client-implementation_amd/build.py

Every csrc/*.hip is compiled to build/<name>.o (re-used while its sources and
headers are older than the object) and linked into lib/libzklc_mi355.so.  The
.so is git-ignored but travels to the GPU box with the gpurun snapshot.
"""
import concurrent.futures as cf
import glob
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
BUILD = os.path.join(HERE, "build")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libzklc_mi355.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function"]


def _newest(paths):
    return max((os.path.getmtime(p) for p in paths), default=0.0)


HOST_CXX = os.environ.get("CXX", "g++")
HOST_FLAGS = ["-O3", "-funroll-loops", "-std=c++17", "-fPIC", "-pthread", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"]


def _compile(src, obj, log):
    # *.hip = device + host code for gfx950 (hipcc); *.cpp = host-only helpers (transcript), plain C++
    cmd = ([HIPCC] + FLAGS if src.endswith(".hip") else [HOST_CXX] + HOST_FLAGS) + ["-c", src, "-o", obj]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s:\n%s\n%s" % (src, r.stdout, r.stderr))
    if log:
        print("[zklc build] compiled", os.path.basename(src), file=sys.stderr)
    return obj


def build(verbose=True, force=False):
    os.makedirs(BUILD, exist_ok=True)
    os.makedirs(LIBDIR, exist_ok=True)
    srcs = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.cpp")))
    hdrs = glob.glob(os.path.join(CSRC, "*.cuh")) + glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(
        os.path.join(CSRC, "*.inc")) + glob.glob(os.path.join(HERE, "..", "include", "*.h"))
    dep_time = _newest(hdrs + [os.path.abspath(__file__)])
    jobs, objs = [], []
    for s in srcs:
        o = os.path.join(BUILD, os.path.basename(s).replace(".", "_") + ".o")
        objs.append(o)
        if force or not os.path.exists(o) or os.path.getmtime(o) < max(os.path.getmtime(s), dep_time):
            jobs.append((s, o))
    if jobs:
        with cf.ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 4)) as ex:
            list(ex.map(lambda so: _compile(so[0], so[1], verbose), jobs))
    if jobs or not os.path.exists(LIB) or os.path.getmtime(LIB) < _newest(objs):
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread", "-o", LIB] + objs
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("link failed:\n%s\n%s" % (r.stdout, r.stderr))
        if verbose:
            print("[zklc build] linked", LIB, file=sys.stderr)
    return LIB


DEVSIM_DIR = os.path.join(HERE, "..", "tests", "devsim")
DEVSIM_SRC = os.path.join(DEVSIM_DIR, "devsim.hip")
DEVSIM_LIB = os.path.join(DEVSIM_DIR, "libdevsim.so")


def devsim_sources():
    return [DEVSIM_SRC, os.path.abspath(__file__)] + [p for ext in ("*.cuh", "*.h", "*.inc") for p in glob.glob(os.path.join(CSRC, ext))]


def devsim_is_current():
    return os.path.exists(DEVSIM_LIB) and os.path.getmtime(DEVSIM_LIB) >= _newest(devsim_sources())


def build_devsim(verbose=True, force=False):
    """tests/devsim/libdevsim.so: the arithmetic headers behind one-lane-per-tuple test kernels (test infrastructure, the device twin
    of tests/hostsim; never part of libzklc_mi355.so).  Same compiler, same FLAGS as the library, so the lane functions are lowered
    the way the product's are."""
    if force or not devsim_is_current():
        r = subprocess.run([HIPCC] + FLAGS + ["-shared", DEVSIM_SRC, "-o", DEVSIM_LIB], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed for %s:\n%s\n%s" % (DEVSIM_SRC, r.stdout, r.stderr))
        if verbose:
            print("[zklc build] built", DEVSIM_LIB, file=sys.stderr)
    return DEVSIM_LIB


PGD_DIR = os.path.join(HERE, "..", "tests", "poseidon_gate_dev")
PGD_SRC = os.path.join(PGD_DIR, "poseidon_gate_dev.hip")
PGD_LIB = os.path.join(PGD_DIR, "libposeidon_gate_dev.so")


def poseidon_gate_dev_is_current():
    deps = [PGD_SRC, os.path.abspath(__file__)] + [p for ext in ("*.cuh", "*.h", "*.inc") for p in glob.glob(os.path.join(CSRC, ext))]
    return os.path.exists(PGD_LIB) and os.path.getmtime(PGD_LIB) >= _newest(deps)


def build_poseidon_gate_dev(verbose=True, force=False):
    """tests/poseidon_gate_dev/libposeidon_gate_dev.so: the evaluators of the Poseidon gate behind a one-row-per-lane kernel (test
    infrastructure for tests/test_gpu_poseidon_gate_stmt.py; the library's compiler and FLAGS; a few seconds)."""
    if force or not poseidon_gate_dev_is_current():
        r = subprocess.run([HIPCC] + FLAGS + ["-Wno-inline-asm", "-shared", PGD_SRC, "-o", PGD_LIB], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed for %s:\n%s\n%s" % (PGD_SRC, r.stdout, r.stderr))
        if verbose:
            print("[zklc build] built", PGD_LIB, file=sys.stderr)
    return PGD_LIB


FCD_DIR = os.path.join(HERE, "..", "tests", "fri_coeff_dev")
FCD_SRC = os.path.join(FCD_DIR, "fri_coeff_dev.hip")
FCD_CASES = os.path.join(FCD_DIR, "fri_coeff_dev_cases.cpp")
FCD_LIB = os.path.join(FCD_DIR, "libfri_coeff_dev.so")


def fri_coeff_dev_is_current():
    deps = [FCD_SRC, FCD_CASES, os.path.join(HERE, "..", "tests", "fri_coeff_host", "fri_coeff_cases.h"), os.path.abspath(__file__)]
    deps += [p for ext in ("*.cuh", "*.h", "*.inc") for p in glob.glob(os.path.join(CSRC, ext))]
    return os.path.exists(FCD_LIB) and os.path.getmtime(FCD_LIB) >= _newest(deps)


def build_fri_coeff_dev(verbose=True, force=False):
    """tests/fri_coeff_dev/libfri_coeff_dev.so: the coefficient-form FRI combination kernel over the cases of
    tests/fri_coeff_host (test infrastructure for tests/test_gpu_fri_coeff.py; the kernel with the library's compiler and FLAGS, the
    cases and their Horner sums as plain host C++; a few seconds)."""
    if force or not fri_coeff_dev_is_current():
        obj, kobj = os.path.join(FCD_DIR, "fri_coeff_dev_cases.o"), os.path.join(FCD_DIR, "fri_coeff_dev.o")
        for cmd in ([HOST_CXX, "-O2", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-c", FCD_CASES, "-o", obj],
                    [HIPCC] + FLAGS + ["-c", FCD_SRC, "-o", kobj],
                    [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", FCD_LIB, kobj, obj]):
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError("%s failed for %s:\n%s\n%s" % (cmd[0], FCD_DIR, r.stdout[-4000:], r.stderr[-4000:]))
        if verbose:
            print("[zklc build] built", FCD_LIB, file=sys.stderr)
    return FCD_LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    build_devsim(force="--force" in sys.argv)
    build_poseidon_gate_dev(force="--force" in sys.argv)
    build_fri_coeff_dev(force="--force" in sys.argv)
