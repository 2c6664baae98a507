#!/usr/bin/env python3
"""Code size and register count of the Poseidon-Goldilocks hash kernels and of the Goldilocks NTT pass kernels, read from the gfx950
code objects in build/*.o.  Needs no GPU.

The symbol size of each kernel's function: the 64 KB instruction cache is the condition the leaf kernel's single looped copy of the
full-round statement exists for.  The VGPR / scratch figures of the kernel descriptor's metadata: above 128 VGPRs a SIMD holds three
waves instead of four, and the forward-order shift-twiddle NTT pass sits at exactly 128.

    python tools/kernel_code_size.py [build-dir]      # one line per kernel: code bytes, VGPRs, scratch bytes, mangled name
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "zk-light-client-implementation_amd", "build")
LLVM = "/opt/rocm/lib/llvm/bin"
KERNELS = {"goldilocks_hip.o": ("gl_hash_leaves_kernel", "gl_merkle_level_kernel", "gl_merkle_tail_kernel", "gl_ntt_pass_"),
           "plonky2_prover_hip.o": ("p2_pow_kernel",)}


def kernels(obj):
    """-> {mangled name: (code bytes, vgprs, scratch bytes)} of the gfx950 code object embedded in `obj`"""
    with tempfile.TemporaryDirectory() as d:
        tmp = os.path.join(d, os.path.basename(obj))
        os.symlink(obj, tmp)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", tmp], capture_output=True, cwd=d, check=True)
        co = os.path.join(d, [f for f in os.listdir(d) if "gfx950" in f][0])
        syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-sW", co], capture_output=True, text=True, check=True).stdout
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    size = {}
    for ln in syms.splitlines():          # .symtab and .dynsym list each function once
        m = re.match(r"\s*\d+:\s+[0-9a-f]+\s+(\d+)\s+FUNC\s+\S+\s+\S+\s+\S+\s+(\S+)", ln)
        if m:
            size[m.group(2)] = int(m.group(1))
    out = {}
    for blk in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        out[name] = (size.get(name, 0), int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)),
                     int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)))
    return out


def main():
    build = sys.argv[1] if len(sys.argv) > 1 else BUILD
    print("%8s %6s %8s  %s" % ("code", "vgprs", "scratch", "kernel"))
    for obj, names in KERNELS.items():
        for name, (code, vgprs, scratch) in sorted(kernels(os.path.join(build, obj)).items()):
            if any(n in name for n in names):
                print("%8d %6d %8d  %s" % (code, vgprs, scratch, name))


if __name__ == "__main__":
    sys.exit(main())
