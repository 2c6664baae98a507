"""Native plonky2 proof verifier: `CircuitData::verify` / `VerifierCircuitData::verify` of the reference
(near_bft_finality/src/prove_block_data/primitives.rs:110,160, header_bphash.rs:94; the tests of prove_crypto/ed25519.rs:175-202,
recursion.rs:124-153, sha256.rs:211-215) over the C ABI (include/zklc.h: zklc_plonky2_verifier_create / zklc_plonky2_verify_batch).

    v = Verifier(ctx, common, verifier_only)     # ctx=None: the host path (no GPU)
    v.verify(proof)                              # raises ProofRejected
    v.verify_batch([p0, p1, ...])                # -> list of ZKLC_PROOF_* statuses

A proof is its bytes (`ProofWithPublicInputs::to_bytes()`) or the proof.json dict.  The checks and their order are those of
gnark-plonky2-verifier: format, proof of work, vanishing identity, then the FRI query rounds.  With a context the query phase of
the whole batch runs on the GPU; the status of every proof is the same on both paths.
"""
import ctypes
import struct

import numpy as np

from .. import _lib
from . import gates as G
from . import serialization as S

HASH_GL, HASH_BN128 = S.HASH_GL, S.HASH_BN128

PROOF_OK, PROOF_BAD_FORMAT, PROOF_BAD_POW, PROOF_BAD_VANISHING, PROOF_BAD_MERKLE, PROOF_BAD_FRI = range(6)
STATUS_NAMES = {PROOF_OK: "ok", PROOF_BAD_FORMAT: "bad format", PROOF_BAD_POW: "bad proof of work",
                PROOF_BAD_VANISHING: "vanishing identity fails", PROOF_BAD_MERKLE: "Merkle opening fails",
                PROOF_BAD_FRI: "FRI check fails"}


class ProofRejected(ValueError):
    """a proof that does not verify; `.status` = ZKLC_PROOF_*, `.name` = its description"""

    def __init__(self, status):
        self.status, self.name = int(status), STATUS_NAMES.get(int(status), "status %d" % status)
        super().__init__("plonky2 proof rejected: %s" % self.name)


def _root_of_unity(bits):
    from .builder import root_of_unity
    return root_of_unity(bits)


def native_arguments_from_common(common, hasher=HASH_GL):
    """the argument blocks of zklc_plonky2_circuit_create / zklc_plonky2_verifier_create for a common_data dict (the reference's
    common_data.json or `CircuitData.common_data()`): (ParamsC, GateC array, extra u64 array, k_is u64 array) -- what
    container.native_arguments gives for a CircuitData"""
    from .builder import P
    from .prover import GateC, ParamsC
    cfg, fp = common["config"], common["fri_params"]
    if cfg.get("zero_knowledge") or fp.get("hiding"):
        raise ValueError("zero-knowledge (hiding) proofs are not supported by the native verifier")
    if common.get("num_lookup_polys") or common.get("num_lookup_selectors") or common.get("luts"):
        raise ValueError("lookup arguments are not supported by the native verifier")
    fc = fp["config"]
    arity_bits = list(fp["reduction_arity_bits"])
    if len(arity_bits) > 8:
        raise ValueError("more than 8 FRI reductions")
    sel = common["selectors_info"]
    groups = [(g["start"], g["end"]) for g in sel["groups"]]
    p = ParamsC()
    p.degree_bits, p.num_wires, p.num_routed_wires = fp["degree_bits"], cfg["num_wires"], cfg["num_routed_wires"]
    p.num_constants, p.num_selectors, p.num_challenges = common["num_constants"], len(groups), cfg["num_challenges"]
    p.rate_bits, p.cap_height, p.proof_of_work_bits = fc["rate_bits"], fc["cap_height"], fc["proof_of_work_bits"]
    p.num_query_rounds = fc["num_query_rounds"]
    p.quotient_degree_factor, p.num_partial_products = common["quotient_degree_factor"], common["num_partial_products"]
    p.num_gate_constraints, p.num_public_inputs = common["num_gate_constraints"], common["num_public_inputs"]
    p.hasher, p.num_gates, p.num_arities = int(hasher), len(common["gates"]), len(arity_bits)
    for i, a in enumerate(arity_bits):
        p.arity_bits[i] = a
    gates = (GateC * len(common["gates"]))()
    extra = []
    for i, gid in enumerate(common["gates"]):
        g = G.gate_from_id(gid)
        gates[i].type = g.code
        for k in range(4):
            gates[i].p[k] = g.params[k]
        si = sel["selector_indices"][i]
        s, e = groups[si]
        gates[i].selector_index, gates[i].group_start, gates[i].group_end = si, s, e
        gates[i].extra_off = len(extra)
        if g.code == G.COSET_INTERPOLATION:   # barycentric weights, then the subgroup points
            w = _root_of_unity(g.subgroup_bits)
            extra += list(g.weights) + [pow(w, j, P) for j in range(1 << g.subgroup_bits)]
    kis = [int(k) for k in common["k_is"][:cfg["num_routed_wires"]]]
    return p, gates, np.array(extra, dtype=np.uint64), np.array(kis, dtype=np.uint64)


def hasher_of(verifier_only):
    return HASH_GL if isinstance(verifier_only["circuit_digest"], dict) else HASH_BN128


class Verifier:
    """One circuit's verifier (zklc_plonky2_verifier).  ctx: a zklc_amd.Context for the GPU query phase, or None (host only)."""

    def __init__(self, ctx, common, verifier_only, hasher=None):
        self.ctx, self.common = ctx, common
        self.hasher = hasher_of(verifier_only) if hasher is None else int(hasher)
        self._lib = _lib.load()
        p, gates, ex, kis = native_arguments_from_common(common, self.hasher)
        cap = np.frombuffer(b"".join(S._hash_bytes(h, self.hasher) for h in verifier_only["constants_sigmas_cap"]), dtype=np.uint8)
        dig = np.frombuffer(S._hash_bytes(verifier_only["circuit_digest"], self.hasher), dtype=np.uint8)
        lde_bits = p.degree_bits + p.rate_bits
        if cap.size != 32 << min(p.cap_height, lde_bits):
            raise ValueError("constants_sigmas_cap has %d entries, the circuit's cap %d" % (cap.size // 32, 1 << min(p.cap_height, lde_bits)))
        h = ctypes.c_void_p()
        rc = self._lib.zklc_plonky2_verifier_create(None if ctx is None else ctx._h, ctypes.byref(p), gates,
                                                    ex.ctypes.data if ex.size else None, ex.size, kis.ctypes.data,
                                                    cap.ctypes.data, dig.ctypes.data, ctypes.byref(h))
        if rc != 0:
            raise _lib.ZklcError(rc, "zklc_plonky2_verifier_create")
        self._h = h
        self.proof_bytes = int(self._lib.zklc_plonky2_verifier_proof_bytes(h))

    @classmethod
    def from_prover(cls, prover):
        """the verifier of a zklc_amd.plonky2.Prover's circuit, on the prover's context
        (zklc_plonky2_verifier_create_from_circuit: cap and digest from the circuit's commitment)"""
        v = cls.__new__(cls)
        v.ctx, v.common, v.hasher = prover.ctx, prover.common, prover.hasher
        v._lib = _lib.load()
        h = ctypes.c_void_p()
        prover.ctx._check(v._lib.zklc_plonky2_verifier_create_from_circuit(prover.ctx._h, prover._h, ctypes.byref(h)))
        v._h = h
        v.proof_bytes = int(v._lib.zklc_plonky2_verifier_proof_bytes(h))
        return v

    def close(self):
        if getattr(self, "_h", None):
            self._lib.zklc_plonky2_verifier_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _bytes(self, proof):
        if isinstance(proof, (bytes, bytearray, memoryview)):
            return bytes(proof)
        if not isinstance(proof, dict):
            raise TypeError("a proof is its bytes or the proof.json dict, not %s" % type(proof).__name__)
        try:
            return S.proof_to_bytes(proof, self.common, self.hasher)
        except (KeyError, IndexError, AssertionError, struct.error):
            return None     # a proof.json that does not have this circuit's shape, or a value that is not a u64: BAD_FORMAT

    def _run(self, proofs, host, threads):
        raws = [self._bytes(p) for p in proofs]
        status = [PROOF_BAD_FORMAT] * len(raws)
        keep = [i for i, r in enumerate(raws) if r is not None and len(r) == self.proof_bytes]
        if keep:
            buf = np.frombuffer(b"".join(raws[i] for i in keep), dtype=np.uint8)
            out = np.zeros(len(keep), dtype=np.int32)
            if host or self.ctx is None:
                rc = self._lib.zklc_plonky2_verify_batch_host(self._h, buf.ctypes.data, len(keep), int(threads), out.ctypes.data)
                if rc != 0:
                    raise _lib.ZklcError(rc, "zklc_plonky2_verify_batch_host")
            else:
                self.ctx._check(self._lib.zklc_plonky2_verify_batch(self.ctx._h, self._h, buf.ctypes.data, len(keep), out.ctypes.data))
            for k, i in enumerate(keep):
                status[i] = int(out[k])
        return status

    def verify_batch(self, proofs, threads=16):
        """-> [ZKLC_PROOF_* per proof]; the GPU query phase when the verifier has a context"""
        return self._run(list(proofs), False, threads)

    def verify_batch_host(self, proofs, threads=16):
        """-> [ZKLC_PROOF_* per proof], every check on the host (`threads` host threads, 1 proof per task)"""
        return self._run(list(proofs), True, threads)

    def verify(self, proof):
        """returns None for a valid proof, raises ProofRejected otherwise"""
        st = self.verify_batch([proof])[0]
        if st != PROOF_OK:
            raise ProofRejected(st)

    def last_timings(self):
        """milliseconds of the last GPU batch: host stage, Merkle kernel, FRI kernel, total"""
        buf = np.zeros(4, dtype=np.float64)
        k = self._lib.zklc_plonky2_verifier_last_timings(self._h, buf.ctypes.data, 4)
        return dict(zip(["host", "merkle_kernel", "fri_kernel", "total"][:k], [float(x) for x in buf[:k]]))
