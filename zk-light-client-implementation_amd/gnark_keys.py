"""Readers / writers of gnark's Groth16 key files for BN254: `pk.bin` / `vk.bin` as `SaveVerifierCircuitGroth` writes them
(`pk.WriteRawTo`, `vk.WriteRawTo`: gnark-plonky2-verifier/verifier/util.go:172-216) and `LoadGroth16ProverData` /
`LoadGroth16VerifierKey` read them (`pk.ReadFrom`, `vk.ReadFrom`: util.go:337-389).  The result feeds `groth16.Groth16Prover` /
`groth16.Groth16Verifier` directly (the `*_words` arrays are gnark-crypto's in-memory layout, little-endian Montgomery limbs).

PARITY UNPINNED.  The byte layout lives in un-vendored dependencies (gnark v0.9.1 backend/groth16/bn254/marshal.go, gnark-crypto
v0.12.2 ecc/bn254/marshal.go and fr/fft/domain.go; go.mod:8-9) and the reference ships no pk.bin / vk.bin to check against (the
keys are ~GB files produced by its trusted setup run).  What IS pinned by the reference: the uncompressed point encoding (32-byte
big-endian coordinates, G2 as X.A1 | X.A0 | Y.A1 | Y.A0) through the 256 proof bytes that cmd/web-api.go:90-98 slices into the
eight words Verifier.sol consumes (tests/test_formats.py).  The rest -- field order, slice length prefixes, the 2-bit point flags,
the domain header -- is restated from the published marshal code; everything after the last field this module understands
(Pedersen commitment keys: the reference's circuit has none, Verifier.sol carries no commitment terms) is kept as an opaque
trailer and reported, not interpreted.  Tests: round trips and structure only (tests/test_gnark_keys.py).

`load_pk` (end of this module) reads the same layout with the point arrays decoded and validated by the library -- one lane per
point on the GPU, or the same lane functions on host threads (include/zklc.h zklc_bn254_g{1,2}_decode_{dev,host}) -- so that the
reader is not the bottleneck of a start-up; it pins nothing: read_g1 / read_g2 below stay the specification of those kernels.
`save_pk` / `save_vk` are the writing direction (zklc_bn254_g{1,2}_encode_{dev,host}): a key in that memory layout, as `Setup` or
`load_pk` leave it, to the file; write_g1 / write_g2 and pk_to_gnark_bytes / vk_to_gnark_bytes stay their specification.
"""
import struct

import numpy as np

from .formats import P_BN254 as P, ProofInvalid
from .groth16 import fp_to_mont_words

R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
_FLAG_MASK, _UNCOMPRESSED, _INFINITY, _SMALLEST, _LARGEST = 0xC0, 0x00, 0x40, 0x80, 0xC0
_HALF_P = (P - 1) // 2


class _Reader:
    def __init__(self, data, copy=True):
        # copy=False: a view of the caller's buffer (a memory-mapped key file: load_pk)
        self.b, self.o = memoryview(bytes(data) if copy else data), 0

    def take(self, n):
        if self.o + n > len(self.b):
            raise ProofInvalid("key file truncated at byte %d (+%d)" % (self.o, n))
        v = self.b[self.o:self.o + n]
        self.o += n
        return v

    def u32(self):
        return struct.unpack(">I", self.take(4))[0]

    def u64(self):
        return struct.unpack(">Q", self.take(8))[0]

    def fr(self):
        v = int.from_bytes(self.take(32), "big")
        if v >= R:
            raise ProofInvalid("scalar field element not reduced")
        return v


def _sqrt_fp(a):
    x = pow(a, (P + 1) // 4, P)
    if x * x % P != a % P:
        raise ProofInvalid("compressed point: x is not on the curve")
    return x


def _fp2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def _fp2_sqrt(a):
    """a square root of a in Fp2 = Fp[i] / (i^2 + 1) (complex method); raises if a is not a square"""
    a0, a1 = a
    if a1 == 0:
        try:
            return (_sqrt_fp(a0), 0)
        except ProofInvalid:
            return (0, _sqrt_fp((P - a0) % P))
    d = _sqrt_fp((a0 * a0 + a1 * a1) % P)
    for dd in (d, (P - d) % P):
        h = (a0 + dd) * pow(2, P - 2, P) % P
        x0 = pow(h, (P + 1) // 4, P)
        if x0 * x0 % P != h or x0 == 0:
            continue
        x1 = a1 * pow(2 * x0, P - 2, P) % P
        if _fp2_mul((x0, x1), (x0, x1)) == (a0 % P, a1 % P):
            return (x0, x1)
    raise ProofInvalid("compressed point: x is not on the twist curve")


_B2 = None


def _twist_b():
    global _B2
    if _B2 is None:
        inv = pow(82, P - 2, P)
        _B2 = (27 * inv % P, (P - 3 * inv % P) % P)                   # 3 / (9 + i)
    return _B2


def _g1_lex_largest(y):
    return y > _HALF_P


def _g2_lex_largest(y):
    """gnark-crypto E2.LexicographicallyLargest: compares A1 first, A0 when A1 = 0"""
    return y[1] > _HALF_P if y[1] else y[0] > _HALF_P


def read_g1(rd):
    """one G1Affine as gnark-crypto's decoder accepts it: uncompressed (64 bytes) or compressed (32 bytes), by the flag bits"""
    first = rd.take(32)
    flag = first[0] & _FLAG_MASK
    x = int.from_bytes(first, "big") & ((1 << 254) - 1)
    if flag == _INFINITY:
        # compressed infinity is 32 bytes; the uncompressed form has 32 more zero bytes: gnark's writers never mix the two in a
        # file, so the caller says which one it expects (read_g1_raw)
        if x:
            raise ProofInvalid("infinity flag with a non-zero coordinate")
        return None
    if x >= P:
        raise ProofInvalid("G1 x not reduced")
    if flag == _UNCOMPRESSED:
        y = int.from_bytes(rd.take(32), "big")
        if y >= P:
            raise ProofInvalid("G1 y not reduced")
        if x == 0 and y == 0:
            return None
        if (y * y - x * x * x - 3) % P:
            raise ProofInvalid("G1 point not on the curve")
        return (x, y)
    y = _sqrt_fp((x * x * x + 3) % P)
    if _g1_lex_largest(y) != (flag == _LARGEST):
        y = (P - y) % P
    return (x, y)


def read_g2(rd):
    first = rd.take(64)
    flag = first[0] & _FLAG_MASK
    x1 = int.from_bytes(first[:32], "big") & ((1 << 254) - 1)
    x0 = int.from_bytes(first[32:], "big")
    if flag == _INFINITY:
        if x0 or x1:
            raise ProofInvalid("infinity flag with a non-zero coordinate")
        return None
    if x0 >= P or x1 >= P:
        raise ProofInvalid("G2 x not reduced")
    x = (x0, x1)
    rhs = _fp2_mul(_fp2_mul(x, x), x)
    b = _twist_b()
    rhs = ((rhs[0] + b[0]) % P, (rhs[1] + b[1]) % P)
    if flag == _UNCOMPRESSED:
        raw = rd.take(64)
        y = (int.from_bytes(raw[32:], "big"), int.from_bytes(raw[:32], "big"))
        if y[0] >= P or y[1] >= P:
            raise ProofInvalid("G2 y not reduced")
        if x == (0, 0) and y == (0, 0):
            return None
        if _fp2_mul(y, y) != rhs:
            raise ProofInvalid("G2 point not on the twist curve")
        return (x, y)
    y = _fp2_sqrt(rhs)
    if _g2_lex_largest(y) != (flag == _LARGEST):
        y = ((P - y[0]) % P, (P - y[1]) % P)
    return (x, y)


def _read_points(rd, one, raw_inf_pad):
    n = rd.u32()
    out = []
    for _ in range(n):
        start = rd.o
        pt = one(rd)
        if pt is None and raw_inf_pad and rd.o - start == raw_inf_pad:
            rd.take(raw_inf_pad)                           # RawBytes of infinity: the flag byte + zeros over the full uncompressed width
        out.append(pt)
    return out


def write_g1(pt, raw=True):
    if pt is None:
        return bytes([_INFINITY]) + bytes(63 if raw else 31)
    x, y = pt
    if raw:
        return x.to_bytes(32, "big") + y.to_bytes(32, "big")
    b = bytearray(x.to_bytes(32, "big"))
    b[0] |= _LARGEST if _g1_lex_largest(y) else _SMALLEST
    return bytes(b)


def write_g2(pt, raw=True):
    if pt is None:
        return bytes([_INFINITY]) + bytes(127 if raw else 63)
    (x0, x1), (y0, y1) = pt
    if raw:
        return b"".join(v.to_bytes(32, "big") for v in (x1, x0, y1, y0))
    b = bytearray(x1.to_bytes(32, "big") + x0.to_bytes(32, "big"))
    b[0] |= _LARGEST if _g2_lex_largest((y0, y1)) else _SMALLEST
    return bytes(b)


def _points(pts, one, raw):
    return struct.pack(">I", len(pts)) + b"".join(one(p, raw) for p in pts)


def _padded(rd, raw):
    """readers of single points: the raw (uncompressed) form of infinity is padded to the full width"""
    def g1():
        s = rd.o
        pt = read_g1(rd)
        if pt is None and raw and rd.o - s == 32:
            rd.take(32)
        return pt

    def g2():
        s = rd.o
        pt = read_g2(rd)
        if pt is None and raw and rd.o - s == 64:
            rd.take(64)
        return pt
    return g1, g2, (32 if raw else 0), (64 if raw else 0)


# ---------------------------------------------------------------------------------------------- verifying key
def vk_to_gnark_bytes(vk, raw=True, trailer=b""):
    """vk: dict alpha1, beta1, delta1 (G1), beta2, gamma2, delta2 (G2), K (G1 list).  gnark order: [alpha]1, [beta]1, [beta]2,
    [gamma]2, [delta]1, [delta]2, uint32 len(K), K..."""
    return (write_g1(vk["alpha1"], raw) + write_g1(vk["beta1"], raw) + write_g2(vk["beta2"], raw) + write_g2(vk["gamma2"], raw)
            + write_g1(vk["delta1"], raw) + write_g2(vk["delta2"], raw) + _points(vk["K"], write_g1, raw) + trailer)


def vk_from_gnark_bytes(data, raw=True):
    """-> dict as above + "trailer" (bytes after K: commitment fields, uninterpreted).  raw: the file was written by WriteRawTo
    (only matters for points at infinity, whose raw form is padded to the uncompressed width)."""
    rd = _Reader(data)
    g1, g2, pad1, pad2 = _padded(rd, raw)
    vk = {"alpha1": g1(), "beta1": g1(), "beta2": g2(), "gamma2": g2(), "delta1": g1(), "delta2": g2()}
    vk["K"] = _read_points(rd, read_g1, pad1)
    vk["trailer"] = bytes(rd.b[rd.o:])
    return vk


# ---------------------------------------------------------------------------------------------- proving key
def _domain_bytes(n):
    """fft.Domain.WriteTo: Cardinality (uint64), CardinalityInv, Generator, GeneratorInv, FrMultiplicativeGen, FrMultiplicativeGenInv
    (32-byte big-endian regular form)"""
    log_n = n.bit_length() - 1
    assert 1 << log_n == n and log_n <= 28
    gen = pow(5, (R - 1) >> log_n, R)
    vals = [pow(n, R - 2, R), gen, pow(gen, R - 2, R), 5, pow(5, R - 2, R)]
    return struct.pack(">Q", n) + b"".join(v.to_bytes(32, "big") for v in vals)


def pk_to_gnark_bytes(pk, raw=True, trailer=b""):
    """pk: the dict of oracle.groth16.setup / Groth16Prover (integer tuples, None = infinity; A, B1, B2 complete or compacted with
    infinity_a / infinity_b).  gnark order: domain, [alpha]1, [beta]1, [delta]1, A, B1, Z, K, [beta]2, [delta]2, B2, nbWires,
    NbInfinityA, NbInfinityB, InfinityA, InfinityB (one byte per bool)."""
    inf_a, inf_b = pk.get("infinity_a"), pk.get("infinity_b")
    A, B1, B2 = pk["A"], pk["B1"], pk["B2"]
    if inf_a is None:
        inf_a = [p is None for p in A]
        A = [p for p in A if p is not None]
    if inf_b is None:
        inf_b = [p is None for p in B1]
        assert [p is None for p in B2] == list(inf_b)
        B1 = [p for p in B1 if p is not None]
        B2 = [p for p in B2 if p is not None]
    out = [_domain_bytes(int(pk["n"])), write_g1(pk["alpha1"], raw), write_g1(pk["beta1"], raw), write_g1(pk["delta1"], raw),
           _points(A, write_g1, raw), _points(B1, write_g1, raw), _points(pk["Z"], write_g1, raw), _points(pk["K"], write_g1, raw),
           write_g2(pk["beta2"], raw), write_g2(pk["delta2"], raw), _points(B2, write_g2, raw),
           struct.pack(">QQQ", len(inf_a), int(sum(bool(x) for x in inf_a)), int(sum(bool(x) for x in inf_b))),
           bytes(1 if x else 0 for x in inf_a), bytes(1 if x else 0 for x in inf_b), trailer]
    return b"".join(out)


def _read_domain(rd):
    """the fft.Domain header -> the domain size"""
    n = rd.u64()
    if n == 0 or n & (n - 1):
        raise ProofInvalid("domain size is not a power of two")
    card_inv, gen = rd.fr(), rd.fr()
    rd.fr(), rd.fr(), rd.fr()
    if card_inv * n % R != 1 or pow(gen, n, R) != 1 or (n > 1 and pow(gen, n // 2, R) == 1):
        raise ProofInvalid("domain header inconsistent")
    return n


def _read_tail(rd, lens, n, n_public):
    """what follows B2: wire counts, infinity masks, trailer, checked against the lengths of the five point arrays
    -> (infinity_a, infinity_b, trailer)"""
    n_wires, n_inf_a, n_inf_b = rd.u64(), rd.u64(), rd.u64()
    if n_wires > (1 << 32):
        raise ProofInvalid("wire count implausible")
    inf_a = np.frombuffer(rd.take(n_wires), dtype=np.uint8).astype(bool)
    inf_b = np.frombuffer(rd.take(n_wires), dtype=np.uint8).astype(bool)
    if int(inf_a.sum()) != n_inf_a or int(inf_b.sum()) != n_inf_b:
        raise ProofInvalid("infinity masks do not match their counts")
    if lens["A"] != n_wires - n_inf_a or lens["B1"] != n_wires - n_inf_b or lens["B2"] != n_wires - n_inf_b:
        raise ProofInvalid("point arrays do not match the infinity masks")
    if lens["Z"] != n - 1 and lens["Z"] != n:
        raise ProofInvalid("Z has %d points for a domain of %d" % (lens["Z"], n))
    if lens["K"] != n_wires - 1 - int(n_public):
        raise ProofInvalid("K has %d points, expected nbWires - nbPublic = %d" % (lens["K"], n_wires - 1 - int(n_public)))
    return inf_a, inf_b, bytes(rd.b[rd.o:])


def pk_from_gnark_bytes(data, n_public, raw=True):
    """-> the dict `Groth16Prover` takes (compacted A / B1 / B2 + infinity masks).  n_public: public inputs WITHOUT the constant
    wire (gnark keeps it in the R1CS file, not in the key: len(K) = nbWires - nbPublic where nbPublic counts the constant one)."""
    rd = _Reader(data)
    n = _read_domain(rd)
    g1, g2, pad1, pad2 = _padded(rd, raw)
    pk = {"n": n, "n_public": int(n_public), "alpha1": g1(), "beta1": g1(), "delta1": g1()}
    pk["A"] = _read_points(rd, read_g1, pad1)
    pk["B1"] = _read_points(rd, read_g1, pad1)
    pk["Z"] = _read_points(rd, read_g1, pad1)
    pk["K"] = _read_points(rd, read_g1, pad1)
    pk["beta2"], pk["delta2"] = g2(), g2()
    pk["B2"] = _read_points(rd, read_g2, pad2)
    pk["infinity_a"], pk["infinity_b"], pk["trailer"] = _read_tail(rd, {k: len(pk[k]) for k in ("A", "B1", "Z", "K", "B2")}, n, n_public)
    pk["Z"] = pk["Z"][:n - 1]
    return pk


def points_to_words(pts, g2=False):
    """affine integer tuples -> gnark-crypto's memory layout (uint64 [n, 8] / [n, 16]) for the `*_words` keys of Groth16Prover"""
    w = 16 if g2 else 8
    out = np.zeros((len(pts), w), dtype=np.uint64)
    for i, p in enumerate(pts):
        if p is None:
            continue
        coords = (p[0][0], p[0][1], p[1][0], p[1][1]) if g2 else p
        out[i] = np.array([v for c in coords for v in fp_to_mont_words(c)], dtype=np.uint64)
    return out


_MONT_INV = pow(1 << 256, P - 2, P)


def words_to_points(words, g2=False):
    """the inverse of `points_to_words`: uint64 [n, 8] / [n, 16] in gnark-crypto's memory layout -> affine integer tuples (an
    all-zero record = None, the point at infinity), what `pk_to_gnark_bytes` / `vk_to_gnark_bytes` and the verifiers take"""
    w = 16 if g2 else 8
    raw = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, w).tobytes()
    out = []
    for i in range(0, len(raw), 8 * w):
        c = [int.from_bytes(raw[i + 32 * j:i + 32 * j + 32], "little") * _MONT_INV % P for j in range(w // 4)]
        if not any(c):
            out.append(None)
        else:
            out.append(((c[0], c[1]), (c[2], c[3])) if g2 else (c[0], c[1]))
    return out


# ---------------------------------------------------------------------------------------------- batched decoding (C ABI)
# include/zklc.h zklc_bn254_g{1,2}_decode_{dev,host}: the point arrays of a key file go through the library -- one lane per point
# on the GPU, or the same lane functions on host threads -- instead of through read_g1 / read_g2 above, which stay the specification
# (and the fallback for a file that mixes encodings).
DECODE_WORKGROUP = 256          # lanes per workgroup of the kernels (csrc/gnark_points.hip)
_CHUNK_POINTS = 1 << 20


def _aligned_u8(nbytes):
    """zeroed uint8 array whose address is a multiple of 64"""
    raw = np.zeros(nbytes + 64, dtype=np.uint8)
    off = (-raw.ctypes.data) % 64
    return raw[off:off + nbytes]


def _stride(g2, compressed):
    return (128 if g2 else 64) >> (1 if compressed else 0)


def decode_points_host(data, n, g2=False, compressed=False, check_subgroup=False, nthreads=0, chunk_points=_CHUNK_POINTS):
    """n fixed-stride points of a gnark point array (any buffer of uint8) on host threads (0 = 16), no GPU
    -> (words uint64 [n, 8 | 16], status uint32 [n], summary [OK, infinity, rejected, first rejected index | None])"""
    from . import _lib
    lib = _lib.load()
    fn = lib.zklc_bn254_g2_decode_host if g2 else lib.zklc_bn254_g1_decode_host
    flags = (_lib.POINTS_COMPRESSED if compressed else 0) | (_lib.POINTS_CHECK_SUBGROUP if check_subgroup else 0)
    stride, width = _stride(g2, compressed), 16 if g2 else 8
    src = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.reshape(-1)
    if src.size < n * stride:
        raise ValueError("point array buffer too small")
    words = _aligned_u8(n * width * 8).view(np.uint64).reshape(n, width)
    status = np.zeros(n, dtype=np.uint32)
    total, summary = [0, 0, 0, None], np.zeros(4, dtype=np.uint64)
    stage = _aligned_u8(min(max(n, 1), chunk_points) * stride)
    for off in range(0, max(n, 1), chunk_points):
        k = min(chunk_points, n - off)
        stage[:k * stride] = src[off * stride:(off + k) * stride]        # the file's bytes to an aligned address, nothing else
        rc = fn(stage.ctypes.data, k, flags, nthreads, words.ctypes.data + off * width * 8, status.ctypes.data + off * 4,
                summary.ctypes.data)
        if rc != 0:
            raise _lib.ZklcError(rc)
        _add_summary(total, summary, off)
    return words, status, total


def _add_summary(total, summary, off):
    for j in range(3):
        total[j] += int(summary[j])
    if total[3] is None and int(summary[3]) != (1 << 64) - 1:
        total[3] = off + int(summary[3])


def decode_points_dev(ctx, data, n, g2=False, compressed=False, check_subgroup=False, chunk_points=_CHUNK_POINTS):
    """the same on ctx's GPU: the bytes are uploaded chunk by chunk through one page-locked buffer and decoded there
    -> (words: torch int64 [n, 8 | 16] on the device, status: torch int32 [n] on the device, summary as decode_points_host)"""
    import torch
    from . import _lib
    flags = (_lib.POINTS_COMPRESSED if compressed else 0) | (_lib.POINTS_CHECK_SUBGROUP if check_subgroup else 0)
    stride, width = _stride(g2, compressed), 16 if g2 else 8
    src = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.reshape(-1)
    if src.size < n * stride:
        raise ValueError("point array buffer too small")
    dev = torch.device("cuda", ctx.device_id)
    words = torch.zeros((n, width), dtype=torch.int64, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    d_summary = torch.zeros(4, dtype=torch.int64, device=dev)
    cap = min(max(n, 1), chunk_points)
    stage = torch.empty(cap * stride, dtype=torch.uint8).pin_memory()
    d_bytes = torch.empty(cap * stride, dtype=torch.uint8, device=dev)
    total = [0, 0, 0, None]
    for off in range(0, max(n, 1), chunk_points):
        k = min(chunk_points, n - off)
        stage.numpy()[:k * stride] = src[off * stride:(off + k) * stride]
        d_bytes[:k * stride].copy_(stage[:k * stride])
        torch.cuda.current_stream(dev).synchronize()               # torch copies on ITS stream; the kernels run on the context's
        ctx.bn254_points_decode_dev(d_bytes, k, words.data_ptr() + off * width * 8, status.data_ptr() + off * 4, d_summary,
                                    group=2 if g2 else 1, flags=flags, stream=ctx.stream_ptr())
        ctx.synchronize()
        _add_summary(total, d_summary.cpu().numpy().view(np.uint64), off)
    return words, status, total


def _span(rd, stride, unit):
    """a point array's length prefix and extent -> (offset, count); the reader moves past it"""
    count = rd.u32()
    left = len(rd.b) - rd.o
    if count * stride > left:
        # where the point-by-point reader runs out: it takes `unit` bytes at a time
        raise ProofInvalid("key file truncated at byte %d (+%d)" % (rd.o + left // unit * unit, unit))
    start = rd.o
    rd.o += count * stride
    return start, count


def load_pk(src, n_public, raw=True, ctx=None, check_subgroup=True, nthreads=0, chunk_points=_CHUNK_POINTS):
    """pk.bin -> the dict `Groth16Prover` takes, the five point arrays decoded and validated by the library.  src: a path (mapped
    with np.memmap: a multi-gigabyte file never becomes Python objects) or a buffer.  Parses what pk_from_gnark_bytes parses, with
    the same checks and messages.  ctx=None: host threads, arrays as uint64 numpy under A_words, B1_words, Z_words, K_words,
    B2_words; with a Context: on its GPU, arrays as device tensors under A_dev ... B2_dev.  B2 is tested for membership in the
    r-torsion subgroup unless check_subgroup=False.  A rejected point raises ProofInvalid with the array, the index and the class."""
    import os
    from . import _lib
    if isinstance(src, (str, os.PathLike)):
        buf = np.memmap(src, dtype=np.uint8, mode="r")
    else:
        buf = np.frombuffer(src, dtype=np.uint8)
    rd = _Reader(buf, copy=False)
    n = _read_domain(rd)
    g1, g2, _, _ = _padded(rd, raw)
    pk = {"n": n, "n_public": int(n_public), "alpha1": g1(), "beta1": g1(), "delta1": g1()}
    s1, s2 = _stride(False, not raw), _stride(True, not raw)
    spans = {name: _span(rd, s1, 32) for name in ("A", "B1", "Z", "K")}
    pk["beta2"], pk["delta2"] = g2(), g2()
    spans["B2"] = _span(rd, s2, 64)
    pk["infinity_a"], pk["infinity_b"], pk["trailer"] = _read_tail(rd, {k: v[1] for k, v in spans.items()}, n, n_public)
    for name, (start, count) in spans.items():
        is_g2 = name == "B2"
        stride = s2 if is_g2 else s1
        data = buf[start:start + count * stride]
        kw = dict(g2=is_g2, compressed=not raw, check_subgroup=check_subgroup and is_g2, chunk_points=chunk_points)
        if ctx is None:
            words, status, summary = decode_points_host(data, count, nthreads=nthreads, **kw)
        else:
            words, status, summary = decode_points_dev(ctx, data, count, **kw)
        if summary[3] is not None:
            i = summary[3]
            cls = int(status[i])
            msg = "%s[%d]: %s" % (name, i, _lib.POINT_CLASS_NAMES[cls])
            flag = int(buf[start + i * stride]) >> 6
            if cls == _lib.POINT_BAD_ENCODING and (flag in (2, 3) if raw else flag == 0):
                msg += (": a flag of the other encoding -- the file mixes point encodings; the point-by-point Python reader "
                        "(pk_from_gnark_bytes) is the fallback")
            raise ProofInvalid(msg)
        if name == "Z":
            words = words[:n - 1]
        pk[name + ("_words" if ctx is None else "_dev")] = words
    return pk


# ---------------------------------------------------------------------------------------------- batched encoding (C ABI)
# include/zklc.h zklc_bn254_g{1,2}_encode_{dev,host}: the writing direction.  The point arrays of a key in gnark-crypto's memory
# layout (what load_pk, groth16_setup.KeySetup and setup_host leave) become the bytes of a key file without a Python integer per
# point; write_g1 / write_g2 on words_to_points stay the specification of those kernels.
def _encode_flags(compressed, validate):
    from . import _lib
    return (_lib.POINTS_COMPRESSED if compressed else 0) | (_lib.POINTS_VALIDATE if validate else 0)


def _encode_chunks_host(words, n, g2, flags, nthreads, chunk_points):
    """the host entry over `words` (uint64 / int64 [n, 8 | 16]) chunk by chunk -> yields (offset, count, bytes, status, summary):
    views of buffers that the next step overwrites"""
    from . import _lib
    lib = _lib.load()
    fn = lib.zklc_bn254_g2_encode_host if g2 else lib.zklc_bn254_g1_encode_host
    stride, width = _stride(g2, bool(flags & _lib.POINTS_COMPRESSED)), 16 if g2 else 8
    src = np.ascontiguousarray(words).view(np.uint64).reshape(-1, width)
    if src.shape[0] < n:
        raise ValueError("point array too short")
    cap = min(max(n, 1), chunk_points)
    out, status, summary = _aligned_u8(cap * stride), np.zeros(cap, dtype=np.uint32), np.zeros(4, dtype=np.uint64)
    stage = None
    for off in range(0, max(n, 1), chunk_points):
        k = min(chunk_points, n - off)
        part = src[off:off + k]
        if k and part.ctypes.data % 16:                                   # a slice of the caller's array at an odd address
            if stage is None:
                stage = _aligned_u8(cap * width * 8).view(np.uint64).reshape(cap, width)
            stage[:k] = part
            part = stage[:k]
        rc = fn(part.ctypes.data if k else None, k, flags, nthreads, out.ctypes.data, status.ctypes.data, summary.ctypes.data)
        if rc != 0:
            raise _lib.ZklcError(rc)
        yield off, k, out[:k * stride], status[:k], summary


def encode_points_host(words, n, g2=False, compressed=False, validate=False, nthreads=0, chunk_points=_CHUNK_POINTS):
    """n points in gnark-crypto's memory layout (uint64 [n, 8 | 16]) on host threads (0 = 16), no GPU -> (bytes uint8 [n x stride]:
    the slots of a key file's point array, status uint32 [n], summary [OK, infinity, rejected, first rejected index | None]).  The
    slot of a rejected record is all 0xFF."""
    stride = _stride(g2, compressed)
    data, status, total = np.empty(n * stride, dtype=np.uint8), np.zeros(n, dtype=np.uint32), [0, 0, 0, None]
    for off, k, part, st, summary in _encode_chunks_host(words, n, g2, _encode_flags(compressed, validate), nthreads, chunk_points):
        data[off * stride:(off + k) * stride] = part
        status[off:off + k] = st
        _add_summary(total, summary, off)
    return data, status, total


def _device_words(ctx, words, width):
    """a key's point array as a contiguous, 16-byte aligned int64 device tensor [n, width] on ctx's GPU (a host array is uploaded)"""
    import torch
    dev = torch.device("cuda", ctx.device_id)
    if not isinstance(words, torch.Tensor):
        words = torch.from_numpy(np.ascontiguousarray(words).view(np.int64).reshape(-1, width))
    t = words.to(dev).reshape(-1, width).contiguous()
    if t.data_ptr() % 16:
        t = t.clone()
    return t


def encode_points_dev(ctx, words, n, g2=False, compressed=False, validate=False, chunk_points=_CHUNK_POINTS):
    """the same on ctx's GPU.  words: an int64 device tensor [n, 8 | 16] (a host array is uploaded first)
    -> (bytes: torch uint8 [n x stride] on the device, status: torch int32 [n] on the device, summary as encode_points_host)"""
    import torch
    flags = _encode_flags(compressed, validate)
    stride, width = _stride(g2, compressed), 16 if g2 else 8
    dev = torch.device("cuda", ctx.device_id)
    src = _device_words(ctx, words, width)
    if src.shape[0] < n:
        raise ValueError("point array too short")
    data = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    d_summary = torch.zeros(4, dtype=torch.int64, device=dev)
    torch.cuda.current_stream(dev).synchronize()                       # torch fills on ITS stream; the kernels run on the context's
    total = [0, 0, 0, None]
    for off in range(0, max(n, 1), chunk_points):
        k = min(chunk_points, n - off)
        ctx.bn254_points_encode_dev(src.data_ptr() + off * width * 8, k, data.data_ptr() + off * stride, status.data_ptr() + off * 4,
                                    d_summary, group=2 if g2 else 1, flags=flags, stream=ctx.stream_ptr())
        ctx.synchronize()
        _add_summary(total, d_summary.cpu().numpy().view(np.uint64), off)
    return data, status, total


def _rejected(name, index, cls):
    from . import _lib
    return ProofInvalid("%s[%d]: %s" % (name, index, _lib.POINT_CLASS_NAMES[int(cls)]))


def _tick(stats, key, t0):
    import time
    if stats is not None:
        stats[key] = stats.get(key, 0.0) + time.perf_counter() - t0


class _HostPointWriter:
    """point arrays through the host encoder into a file, chunk by chunk"""

    def __init__(self, raw, validate, nthreads, chunk_points, stats):
        self.flags, self.nthreads, self.chunk, self.stats = _encode_flags(not raw, validate), nthreads, chunk_points, stats

    def words(self, a, width):
        if not isinstance(a, np.ndarray):                                 # a device tensor of a key made or loaded on a GPU
            a = a.cpu().numpy()
        return np.ascontiguousarray(a).view(np.uint64).reshape(-1, width)

    def write(self, f, name, words, g2):
        import time
        n, total = words.shape[0], 0
        if not n:
            return 0
        chunks = _encode_chunks_host(words, n, g2, self.flags, self.nthreads, self.chunk)
        while True:
            t = time.perf_counter()
            step = next(chunks, None)
            _tick(self.stats, "encode_s", t)
            if step is None:
                return total
            off, k, part, status, summary = step
            if int(summary[2]):
                raise _rejected(name, off + int(summary[3]), status[int(summary[3])])
            t = time.perf_counter()
            f.write(part)
            _tick(self.stats, "write_s", t)
            total += part.size

    def close(self):
        pass


class _DevicePointWriter:
    """point arrays through the kernels into a file: two device buffers and two page-locked staging buffers, so that the write of
    chunk j runs while chunk j + 1 is encoded and read back.  Every read-back is enqueued after a wait for the context's stream
    (the ordering rule of zklc_readback_async: no copy parked in a DMA queue behind unfinished kernels)."""

    def __init__(self, ctx, raw, validate, chunk_points, stats):
        import torch
        self.ctx, self.flags, self.chunk, self.stats = ctx, _encode_flags(not raw, validate), chunk_points, stats
        self.compressed = not raw
        self.dev = torch.device("cuda", ctx.device_id)
        self.stream = torch.cuda.ExternalStream(ctx.stream_ptr(), device=self.dev)
        self.cap = 0

    def _reserve(self, nbytes, points):
        import torch
        if nbytes <= self.cap:
            return
        self.cap = nbytes
        self.d_out = [torch.empty(nbytes, dtype=torch.uint8, device=self.dev) for _ in range(2)]
        self.pinned = [torch.empty(nbytes, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.d_status = [torch.empty(points, dtype=torch.int32, device=self.dev) for _ in range(2)]
        self.d_summary = [torch.zeros(4, dtype=torch.int64, device=self.dev) for _ in range(2)]
        torch.cuda.current_stream(self.dev).synchronize()               # torch hands blocks out on ITS stream

    def words(self, a, width):
        return _device_words(self.ctx, a, width)

    def write(self, f, name, words, g2):
        import time
        import torch
        ctx, n = self.ctx, words.shape[0]
        if not n:
            return 0
        stride, width = _stride(g2, self.compressed), 16 if g2 else 8
        step = min(n, self.chunk)
        self._reserve(step * (128 if not self.compressed else 64), step)
        torch.cuda.current_stream(self.dev).synchronize()               # `words` may have been made on torch's stream
        m = (n + step - 1) // step
        count = lambda j: min(step, n - j * step)

        def launch(j):
            ctx.bn254_points_encode_dev(words.data_ptr() + j * step * width * 8, count(j), self.d_out[j & 1], self.d_status[j & 1],
                                        self.d_summary[j & 1], group=2 if g2 else 1, flags=self.flags, stream=ctx.stream_ptr())

        def put(j):
            t = time.perf_counter()
            f.write(self.pinned[j & 1].numpy()[:count(j) * stride])
            _tick(self.stats, "write_s", t)

        launch(0)
        for j in range(m):
            t = time.perf_counter()
            ctx.synchronize()                                           # settled: kernel j has run, read-back j - 1 has landed
            summary = self.d_summary[j & 1].cpu().numpy().view(np.uint64)
            _tick(self.stats, "device_wait_s", t)
            if int(summary[2]):
                i = int(summary[3])
                raise _rejected(name, j * step + i, self.d_status[j & 1][i].item())
            nb = count(j) * stride
            with torch.cuda.stream(self.stream):
                self.pinned[j & 1][:nb].copy_(self.d_out[j & 1][:nb], non_blocking=True)
            if j + 1 < m:
                launch(j + 1)
            if j:
                put(j - 1)
        t = time.perf_counter()
        ctx.synchronize()
        _tick(self.stats, "device_wait_s", t)
        put(m - 1)
        return n * stride

    def close(self):
        self.ctx.synchronize()


def _key_words(wr, key, name, g2):
    """the point array `name` of a key dictionary, whichever form it has: <name>_dev (device tensor), <name>_words (numpy) or a list
    of integer tuples under <name>"""
    width = 16 if g2 else 8
    for suffix in ("_dev", "_words"):
        if name + suffix in key:
            return wr.words(key[name + suffix], width)
    return wr.words(points_to_words(list(key[name]), g2=g2), width)


def _key_single(wr, key, name, g2):
    width = 16 if g2 else 8
    if name + "_words" in key:
        return wr.words(np.ascontiguousarray(key[name + "_words"]).reshape(1, width), width)
    return wr.words(points_to_words([key[name]], g2=g2), width)


def _open_dst(dst):
    import os
    if isinstance(dst, (str, os.PathLike)):
        return open(dst, "wb"), True
    return dst, False


def _save(dst, body):
    """runs body(f) -> bytes written; a file this call created is removed when the body raises"""
    import os
    f, is_path = _open_dst(dst)
    try:
        total = body(f)
    except BaseException:
        if is_path:
            f.close()
            os.remove(dst)
        raise
    if is_path:
        f.close()
    return total


def _point_writer(raw, ctx, validate, nthreads, chunk_points, stats):
    if chunk_points < 1:
        raise ValueError("chunk_points must be positive")
    if ctx is None:
        return _HostPointWriter(raw, validate, nthreads, chunk_points, stats)
    return _DevicePointWriter(ctx, raw, validate, chunk_points, stats)


def save_pk(pk, dst, raw=True, ctx=None, validate=True, nthreads=0, chunk_points=_CHUNK_POINTS, trailer=b"", stats=None):
    """pk.bin in the layout of pk_to_gnark_bytes, the point arrays encoded by the library and written as they arrive: the file
    never exists as one Python object.  dst: a path or a binary file object -> the number of bytes written.  pk: the dictionary of
    `KeySetup.run` / `load_pk(ctx)` (`*_dev` tensors) or of `setup_host` / `load_pk(ctx=None)` (`*_words` arrays), A / B1 / B2
    compacted with infinity_a / infinity_b; the five single points as `<name>_words` or integer tuples under `<name>`.  ctx=None: host threads; with a
    Context: on its GPU.  validate: every point is tested against its curve equation.  A rejected point raises ProofInvalid with
    the array, the index and the class, in load_pk's wording; a file this call opened is removed.  stats: a dictionary that
    receives the seconds spent waiting for the encoder and writing."""
    def body(f):
        put = lambda b: (f.write(b), len(b))[1]
        wr = _point_writer(raw, ctx, validate, nthreads, chunk_points, stats)
        try:
            arrays = {name: _key_words(wr, pk, name, name == "B2") for name in ("A", "B1", "Z", "K", "B2")}
            inf_a, inf_b = np.asarray(pk["infinity_a"]).astype(bool), np.asarray(pk["infinity_b"]).astype(bool)
            total = put(_domain_bytes(int(pk["n"])))
            for name in ("alpha1", "beta1", "delta1"):
                total += wr.write(f, name, _key_single(wr, pk, name, False), False)
            for name in ("A", "B1", "Z", "K"):
                total += put(struct.pack(">I", arrays[name].shape[0]))
                total += wr.write(f, name, arrays[name], False)
            for name in ("beta2", "delta2"):
                total += wr.write(f, name, _key_single(wr, pk, name, True), True)
            total += put(struct.pack(">I", arrays["B2"].shape[0]))
            total += wr.write(f, "B2", arrays["B2"], True)
            total += put(struct.pack(">QQQ", len(inf_a), int(inf_a.sum()), int(inf_b.sum())))
            total += put(inf_a.astype(np.uint8).tobytes()) + put(inf_b.astype(np.uint8).tobytes())
            return total + put(bytes(trailer))
        finally:
            wr.close()
    return _save(dst, body)


def save_vk(vk, dst, raw=True, ctx=None, validate=True, nthreads=0, chunk_points=_CHUNK_POINTS, trailer=b""):
    """vk.bin in the layout of vk_to_gnark_bytes, every point through the library's encoder.  vk: the integer-tuple dictionary of
    `Setup` (converted with points_to_words: a verifying key is small); `<name>_words` and K_words / K_dev are taken as they are.
    Otherwise as save_pk."""
    def body(f):
        put = lambda b: (f.write(b), len(b))[1]
        wr = _point_writer(raw, ctx, validate, nthreads, chunk_points, None)
        try:
            total = 0
            for name, g2 in (("alpha1", False), ("beta1", False), ("beta2", True), ("gamma2", True), ("delta1", False), ("delta2", True)):
                total += wr.write(f, name, _key_single(wr, vk, name, g2), g2)
            k = _key_words(wr, vk, "K", False)
            total += put(struct.pack(">I", k.shape[0]))
            total += wr.write(f, "K", k, False)
            return total + put(bytes(trailer))
        finally:
            wr.close()
    return _save(dst, body)
