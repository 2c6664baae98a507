"""Batched fixed-base scalar multiplication in BN254 G1 / G2 (zklc_bn254_fixed_base_* and zklc_bn254_g{1,2}_fixed_mul_* of
include/zklc.h, csrc/bn254_fixed_mul.{cuh,hip}, csrc/bn254_fixed_mul_host.cpp): words[i] = scalars[i] * P for one
base P -- gnark-crypto's `BatchScalarMultiplicationG1` / `G2`, by which `groth16.Setup` (gnark-plonky2-verifier/cmd/compile.go:40)
turns a key's scalars into its point arrays.

No CPU fallback for the device path: `mul_dev` is kernel launches through the C ABI over a table the GPU built; `mul_host` is the
library's host twin (the same lane functions, g++) over a table built by host threads."""
import ctypes

import numpy as np

from . import _lib

G1, G2 = 0, 1
R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
INV_GROUP = 16          # points that share one inversion (csrc/bn254_fixed_mul.cuh: FBM_INV_GROUP): point p is in group p % ceil(n / 16)
_M64 = (1 << 64) - 1
_NONE = (1 << 64) - 1


def scalar_words(scalars):
    """integers below 2^256 -> uint64 [n, 4], regular form"""
    return np.array([[(int(s) >> (64 * i)) & _M64 for i in range(4)] for s in scalars], dtype=np.uint64).reshape(-1, 4)


def summary_tuple(words):
    """two u64 of the library -> (points at infinity, index of the first one | None)"""
    count, first = int(words[0]) & _M64, int(words[1]) & _M64
    return count, (None if first == _NONE else first)


class FixedBase:
    """The table of one base: ceil(254 / window_bits) rows of 2^window_bits - 1 affine points.  With a Context it is built by and
    resident on that context's GPU (`mul_dev`); without one it is built by host threads (`mul_host`).  base_words: uint64 [8] / [16]
    in gnark-crypto's memory layout, None = the generator; a finite point of order r."""

    def __init__(self, ctx, group, base_words=None, window_bits=16):
        self._lib = _lib.load()
        self._t = None
        self.ctx, self.group, self.window_bits = ctx, int(group), int(window_bits)
        self.width = 16 if self.group == G2 else 8
        base = None
        if base_words is not None:
            base = np.ascontiguousarray(base_words, dtype=np.uint64).reshape(-1)
            if base.size != self.width:
                raise ValueError("fixed base: %d words for a point of %d" % (base.size, self.width))
        h = ctypes.c_void_p()
        rc = self._lib.zklc_bn254_fixed_base_create(ctx._h if ctx is not None else None, self.group,
                                                    base.ctypes.data if base is not None else None, self.window_bits, ctypes.byref(h))
        if rc != 0:
            raise _lib.ZklcError(rc, "zklc_bn254_fixed_base_create")
        self._t = h
        self._mul_dev = self._lib.zklc_bn254_g2_fixed_mul_dev if self.group == G2 else self._lib.zklc_bn254_g1_fixed_mul_dev
        self._mul_host = self._lib.zklc_bn254_g2_fixed_mul_host if self.group == G2 else self._lib.zklc_bn254_g1_fixed_mul_host

    def close(self):
        t, self._t = getattr(self, "_t", None), None
        if t:
            self._lib.zklc_bn254_fixed_base_destroy(t)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _handle(self):
        if self._t is None:
            raise ValueError("fixed-base table is closed")
        return self._t

    def table_bytes(self):
        return int(self._lib.zklc_bn254_fixed_base_table_bytes(self.group, self.window_bits))

    def workspace_bytes(self, n):
        return int(self._lib.zklc_bn254_fixed_mul_workspace_bytes(self.group, int(n)))

    def enqueue(self, d_scalars, d_words, d_summary, d_ws, stream=None):
        """zklc_bn254_g{1,2}_fixed_mul_dev on `stream` (default: the context's own) into the caller's device tensors: d_scalars
        int64 [n, 4], d_words int64 [n, 8 | 16], d_summary int64 [2], d_ws at least workspace_bytes(n) bytes.  Enqueue only."""
        n = d_scalars.numel() // 4
        if d_scalars.numel() * d_scalars.element_size() != n * 32 or not d_scalars.is_contiguous():
            raise ValueError("fixed base: the scalars must be n x 32 contiguous bytes")
        if d_words.numel() * d_words.element_size() != n * self.width * 8 or not d_words.is_contiguous():
            raise ValueError("fixed base: the output must be %d x %d contiguous bytes" % (n, self.width * 8))
        if d_summary.numel() * d_summary.element_size() != 16:
            raise ValueError("fixed base: the summary is two 64-bit words")
        rc = self._mul_dev(self.ctx._h, self.ctx.stream_ptr() if stream is None else stream, self._handle(), d_scalars.data_ptr(), n,
                           d_words.data_ptr(), d_summary.data_ptr(), d_ws.data_ptr(), d_ws.numel() * d_ws.element_size())
        self.ctx._check(rc)

    def mul_dev(self, d_scalars, stream=None):
        """d_scalars: device tensor int64 [n, 4], regular form -> (words int64 [n, 8 | 16], summary int64 [2], workspace uint8): device
        tensors; the work is enqueued on `stream` (default: the context's own), synchronise it before reading.  The workspace holds
        the multiples until the caller clears or drops it."""
        import torch
        dev = d_scalars.device
        n = d_scalars.numel() // 4
        words = torch.empty((n, self.width), dtype=torch.int64, device=dev)
        summary = torch.empty(2, dtype=torch.int64, device=dev)
        ws = torch.empty(max(self.workspace_bytes(n), 16), dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()      # torch hands blocks out on ITS stream; the kernels run on the context's
        self.enqueue(d_scalars, words, summary, ws, stream)
        return words, summary, ws

    def mul_host(self, scalars, nthreads=0):
        """the host twin: scalars uint64 [n, 4] (regular form) -> (words uint64 [n, 8 | 16], (infinities, first | None))"""
        s = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        n = s.shape[0]
        words = np.empty((n, self.width), dtype=np.uint64)
        summary = np.zeros(2, dtype=np.uint64)
        rc = self._mul_host(self._handle(), s.ctypes.data if n else None, n, int(nthreads), words.ctypes.data if n else None,
                            summary.ctypes.data)
        if rc != 0:
            raise _lib.ZklcError(rc, "zklc_bn254_fixed_mul_host")
        return words, summary_tuple(summary)
