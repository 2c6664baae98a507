"""The constraint system of `groth16.Prove(r1cs, pk, witness)` (gnark-plonky2-verifier/cmd/web-api.go:77) resident on the GPU: the
per-constraint vectors a = A w, b = B w, c = C w from the solved witness, and the test a_j b_j = c_j (zklc_r1cs_* of include/zklc.h,
csrc/r1cs_eval.{cuh,hip}, csrc/r1cs_eval_host.cpp).

The three matrices are ONE CSR of 3 n_constraints rows (row m n_constraints + j = row j of matrix m; A, B, C = 0, 1, 2) over a
dictionary of coefficients in gnark-crypto's Montgomery layout -- what a cgo shim can hand over from gnark's `constraint.R1CS`
(INTEGRATION.md).  Solving the system (gnark's hints) and reading `r1cs.bin` stay on the Go side.  No CPU fallback for the device
path: `abc_dev` is kernel launches through the C ABI; `abc_host` is the library's host twin (the same lane functions, g++)."""
import ctypes

import numpy as np

from . import _lib

R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
_M64 = (1 << 64) - 1
_NONE = (1 << 64) - 1
R1CS_CHECK = 1
# rows of at most BIN_LIMITS[0] terms are summed by one lane, of at most BIN_LIMITS[1] by eight lanes, longer ones by a wave of 64
# (csrc/r1cs_eval.cuh: R1CS_BIN0_MAX, R1CS_BIN1_MAX)
BIN_LIMITS = (4, 64)


class UnsatisfiedConstraint(ValueError):
    """the witness does not satisfy the system: `index` = the first constraint with a_j b_j != c_j, `count` = how many there are
    (gnark's solver: "constraint #index is not satisfied")"""

    def __init__(self, index, count):
        self.index, self.count = int(index), int(count)
        super().__init__("constraint #%d is not satisfied (%d unsatisfied in all)" % (self.index, self.count))


def _mont_words(x):
    m = (x % R) * (1 << 256) % R
    return tuple((m >> (64 * i)) & _M64 for i in range(4))


def summary_tuple(words):
    """two u64 of the library -> (number of unsatisfied constraints, index of the first one | None)"""
    count, first = int(words[0]) & _M64, int(words[1]) & _M64
    return count, (None if first == _NONE else first)


class R1CS:
    """One constraint system, validated and held by the library; with a Context also resident on that context's GPU."""

    def __init__(self, ctx, n_constraints, n_wires, row_ptr, term_wire, term_coeff, coeffs):
        self._lib = _lib.load()
        self._s = None
        self.ctx = ctx
        self.n_constraints, self.n_wires = int(n_constraints), int(n_wires)
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint64).reshape(-1)
        term_wire = np.ascontiguousarray(term_wire, dtype=np.uint32).reshape(-1)
        term_coeff = np.ascontiguousarray(term_coeff, dtype=np.uint32).reshape(-1)
        coeffs = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(-1, 4)
        # the C ABI cannot see the lengths of its arrays: they are compared here, in Python integers, with the sizes it is told
        if self.n_constraints < 0 or row_ptr.size != 3 * self.n_constraints + 1 or term_wire.size != term_coeff.size:
            raise ValueError("r1cs: row_ptr has %d entries for %d constraints, %d wires and %d coefficient ids"
                             % (row_ptr.size, self.n_constraints, term_wire.size, term_coeff.size))
        self.nnz, self.n_coeff = int(term_wire.size), int(coeffs.shape[0])
        h = ctypes.c_void_p()
        rc = self._lib.zklc_r1cs_create(ctx._h if ctx is not None else None, self.n_constraints, self.n_wires, row_ptr.ctypes.data,
                                        term_wire.ctypes.data, term_coeff.ctypes.data, self.nnz, coeffs.ctypes.data, self.n_coeff,
                                        ctypes.byref(h))
        if rc != 0:
            raise _lib.ZklcError(rc, "zklc_r1cs_create")
        self._s = h
        self._ws = None

    @classmethod
    def from_csr(cls, n_constraints, n_wires, row_ptr, term_wire, term_coeff, coeffs, ctx=None):
        """numpy arrays as the C ABI takes them: row_ptr uint64 [3 n_constraints + 1], term_wire / term_coeff uint32 [nnz], coeffs
        uint64 [n_coeff, 4] (Montgomery)"""
        return cls(ctx, n_constraints, n_wires, row_ptr, term_wire, term_coeff, coeffs)

    @classmethod
    def from_rows(cls, A, B, C, n_wires, ctx=None):
        """A, B, C: lists of rows {wire: coefficient} (integers; the form of oracle/groth16.py) -> the CSR over a dictionary without
        duplicates"""
        if not len(A) == len(B) == len(C):
            raise ValueError("r1cs: the three matrices have %d, %d and %d rows" % (len(A), len(B), len(C)))
        ids, row_ptr, wires, cids = {}, [0], [], []
        for M in (A, B, C):
            for row in M:
                for wire, coef in row.items():
                    wires.append(int(wire))
                    cids.append(ids.setdefault(int(coef) % R, len(ids)))
                row_ptr.append(len(wires))
        coeffs = np.array([_mont_words(v) for v in ids], dtype=np.uint64).reshape(-1, 4)
        return cls(ctx, len(A), n_wires, np.array(row_ptr, dtype=np.uint64), np.array(wires, dtype=np.uint32),
                   np.array(cids, dtype=np.uint32), coeffs)

    def close(self):
        s, self._s = getattr(self, "_s", None), None
        if s:
            self._lib.zklc_r1cs_destroy(s)
        self._ws = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if self._s is None:
            raise ValueError("r1cs is closed")
        return self._s

    def workspace_bytes(self):
        return int(self._lib.zklc_r1cs_workspace_bytes(self._handle()))

    def enqueue(self, ctx, d_w_regular, n, d_a, d_b, d_c, d_summary=None, stream=None):
        """zklc_r1cs_abc_dev on `stream` (default: ctx's own) into the caller's device tensors; with d_summary (int64 [2]) the
        satisfaction check runs behind the evaluation.  Enqueue only: the caller waits for the stream.  The workspace is this
        object's, so one evaluation of a system is in flight at a time."""
        import torch
        if self._ws is None or self._ws.device != d_w_regular.device:
            self._ws = torch.empty(max(self.workspace_bytes(), 16), dtype=torch.uint8, device=d_w_regular.device)
        if d_w_regular.numel() * d_w_regular.element_size() != self.n_wires * 32 or not d_w_regular.is_contiguous():
            raise ValueError("r1cs: the witness must be %d x 32 contiguous bytes" % self.n_wires)
        for t in (d_a, d_b, d_c):
            if t.numel() * t.element_size() != int(n) * 32 or not t.is_contiguous():
                raise ValueError("r1cs: an output must be %d x 32 contiguous bytes" % int(n))
        if d_summary is not None and d_summary.numel() * d_summary.element_size() != 16:
            raise ValueError("r1cs: the summary is two 64-bit words")
        rc = self._lib.zklc_r1cs_abc_dev(ctx._h, ctx.stream_ptr() if stream is None else stream, self._handle(), d_w_regular.data_ptr(),
                                         int(n), d_a.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), R1CS_CHECK if d_summary is not None else 0,
                                         d_summary.data_ptr() if d_summary is not None else None, self._ws.data_ptr(), self._ws.numel())
        ctx._check(rc)

    def abc_dev(self, ctx, d_w_regular, n, check=False, stream=None):
        """d_w_regular: device tensor int64 [n_wires, 4], the witness in regular form; n: the domain size (>= n_constraints).
        -> (a, b, c, summary): device tensors int64 [n, 4] in gnark's Montgomery layout (rows from n_constraints on are zero) and,
        with check, int64 [2] = (unsatisfied constraints, index of the first | all-ones), else None.  The work is enqueued on
        `stream` (default: ctx's own); synchronise it before reading."""
        import torch
        dev = d_w_regular.device
        a, b, c = (torch.empty((int(n), 4), dtype=torch.int64, device=dev) for _ in range(3))
        d_summary = torch.empty(2, dtype=torch.int64, device=dev) if check else None
        torch.cuda.current_stream(dev).synchronize()      # torch hands blocks out on ITS stream; the kernels run on the context's
        self.enqueue(ctx, d_w_regular, n, a, b, c, d_summary, stream)
        return a, b, c, d_summary

    def abc_host(self, w_reg, n, check=False, nthreads=0):
        """the host twin: w_reg uint64 [n_wires, 4] (regular form) -> (a, b, c, summary): uint64 [n, 4] arrays and, with check,
        (unsatisfied constraints, index of the first | None), else None"""
        w = np.ascontiguousarray(w_reg, dtype=np.uint64).reshape(-1, 4)
        if w.shape[0] != self.n_wires:
            raise ValueError("r1cs: %d witness words for %d wires" % (w.shape[0], self.n_wires))
        n = int(n)
        a, b, c = (np.empty((max(n, 0), 4), dtype=np.uint64) for _ in range(3))
        summary = np.zeros(2, dtype=np.uint64)
        rc = self._lib.zklc_r1cs_abc_host(self._handle(), w.ctypes.data, n, a.ctypes.data, b.ctypes.data, c.ctypes.data,
                                          R1CS_CHECK if check else 0, int(nthreads), summary.ctypes.data if check else None)
        if rc != 0:
            raise _lib.ZklcError(rc, "zklc_r1cs_abc_host")
        return a, b, c, (summary_tuple(summary) if check else None)
