#!/usr/bin/env python3
"""A w, B w, C w on the GPU at 2^log_n constraints, alone and inside `groth16.Prove` (tools/groth16_quickbench.py's synthetic key):
    python tools/r1cs_eval_quickbench.py [log_n=22] [reps=20] [proofs=10]
 1. the evaluation alone (zklc_r1cs_abc_dev), device events around the enqueue, warmed, `reps` repetitions, with and without the
    satisfaction check; algorithmic bytes = nnz x (8 + 32) (terms, gathered witness words) + 3 n x 32 written, as bytes/s beside the
    8 TB/s HBM peak of an MI355X (information only); the share of every length bin in rows and terms;
 2. whole proofs in one process, alternating `prove_words(w, abc)` with a, b, c PRECOMPUTED (the path without a resident constraint
    system: the host's three matrix-vector products are not in it at all, only their 3 n x 32 byte upload) and
    `prove_witness_words(w)` -- medians and spreads, and the acceptance line: the new median is not above the old one by more than
    the old path's own spread (max - min);
 3. the cost of check=True over check=False, in whole proofs and in the evaluation alone.
PARTS=1 (environment) runs part 1 only -- the form to put under rocprofv3 --kernel-trace --stats for the per-kernel split.

THE SYSTEM IS SYNTHETIC AND ITS MIX IS AN ASSUMPTION (the reference ships no r1cs.bin; the row-length distribution of the gnark
plonky2-verifier circuit is unknown): 70 % of the rows have 1-3 terms, 25 % 4-32, 5 % 33-512, eight rows have 4096; 60 % of the
coefficients are +1 / -1, the others come from a dictionary of 64; wires are drawn uniformly (no locality: the worst case for the
gather).  It is satisfied by EVERY witness: C's rows are A's, and every B row is {wire 0: 1} plus pairs (k: v), (k: -v) -- so b_j =
1 and a_j b_j = c_j, whatever the wires hold, with all three matrices following the mix."""
import os
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np

R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
N_DICT = 64
MIX = "70 % of rows 1-3 terms, 25 % 4-32, 5 % 33-512, eight rows of 4096; 60 % of coefficients +-1; uniform wires"


def row_lengths(rng, n):
    u = rng.random(n)
    length = np.where(u < 0.70, rng.integers(1, 4, n), np.where(u < 0.95, rng.integers(4, 33, n), rng.integers(33, 513, n)))
    length[rng.choice(n, size=min(8, n), replace=False)] = 4096
    return length.astype(np.int64)


def synthetic_system(lg, seed=5):
    """-> (n_constraints, n_wires, row_ptr, term_wire, term_coeff, coeffs) with n_wires = n_constraints = 2^lg"""
    from zklc_amd.groth16 import fr_to_mont_words
    rng = np.random.default_rng(seed)
    n = 1 << lg
    # the dictionary: ids 2 k and 2 k + 1 hold v and -v; ids 0 and 1 are +1 and -1
    vals = [1, R - 1]
    for _ in range(N_DICT // 2 - 1):
        v = int(rng.integers(2, 2**62)) * int(rng.integers(2, 2**62)) * int(rng.integers(2, 2**62)) * int(rng.integers(2, 2**62)) % R
        vals += [v, R - v]
    coeffs = np.array([fr_to_mont_words(v) for v in vals], dtype=np.uint64)
    la = row_lengths(rng, n)
    lb = row_lengths(rng, n) | 1                        # odd: one term for the constant, the rest in cancelling pairs
    nnz_a, nnz_b = int(la.sum()), int(lb.sum())

    def terms(k):
        wire = rng.integers(0, n, k, dtype=np.uint32)
        cid = np.where(rng.random(k) < 0.6, rng.integers(0, 2, k, dtype=np.uint32), rng.integers(2, N_DICT, k, dtype=np.uint32)).astype(np.uint32)
        return wire, cid
    wa, ca = terms(nnz_a)
    wb, cb = terms(nnz_b)
    start_b = np.cumsum(lb) - lb
    pos = np.arange(nnz_b, dtype=np.int64) - np.repeat(start_b, lb)
    second = (pos >= 2) & (pos % 2 == 0)                # the second term of a pair: the wire of the first, the negated coefficient
    idx = np.nonzero(second)[0]
    wb[idx] = wb[idx - 1]
    cb[idx] = cb[idx - 1] ^ np.uint32(1)
    first = start_b                                     # the constant: wire 0 (the witness holds 1 there), coefficient +1
    wb[first] = 0
    cb[first] = 0
    del pos, second, idx
    row_ptr = np.concatenate([[0], np.cumsum(np.concatenate([la, lb, la]))]).astype(np.uint64)
    return n, n, row_ptr, np.concatenate([wa, wb, wa]), np.concatenate([ca, cb, ca]), coeffs


def bin_shares(row_ptr, limits):
    length = np.diff(row_ptr.astype(np.int64))
    bins = np.where(length <= limits[0], 0, np.where(length <= limits[1], 1, 2))
    return [(int((bins == k).sum()), int(length[bins == k].sum())) for k in range(3)]


def synthetic_key(n):
    from oracle import bn254 as B          # test data only: 256 points of each group
    cur, step, g2 = B.g2_mul(12345, B.G2), B.g2_mul(777, B.G2), []
    for _ in range(256):
        g2.append(B.g2_to_words(cur))
        cur = B.g2_add(cur, step)
    cur, step, g1 = B.mul(54321, B.G1), B.mul(999, B.G1), []
    for _ in range(256):
        g1.append(B.to_mont_words(cur[0]) + B.to_mont_words(cur[1]))
        cur = B.add(cur, step)
    g1p, g2p = np.array(g1, dtype=np.uint64), np.array(g2, dtype=np.uint64)
    tile1 = lambda k: np.tile(g1p, ((k + 255) // 256, 1))[:k]
    return {"n": n, "n_public": 4, "A_words": tile1(n), "B1_words": tile1(n), "K_words": tile1(n - 5), "Z_words": tile1(n - 1),
            "B2_words": np.tile(g2p, ((n + 255) // 256, 1))[:n], "alpha1_words": g1p[1:2], "beta1_words": g1p[2:3], "delta1_words": g1p[3:4],
            "beta2_words": g2p[1:2], "delta2_words": g2p[2:3]}


def stats(xs):
    return "median %.2f ms  min %.2f  max %.2f  spread (max - min) %.2f  n = %d" % (statistics.median(xs), min(xs), max(xs), max(xs) - min(xs), len(xs))


def main():
    import torch
    import zklc_amd
    from zklc_amd.groth16 import Groth16Prover
    from zklc_amd.r1cs import BIN_LIMITS, R1CS, summary_tuple
    lg = int(sys.argv[1]) if len(sys.argv) > 1 else 22
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    n_proofs = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    parts = os.environ.get("PARTS", "1,2,3").split(",")
    n = 1 << lg
    ctx = zklc_amd.Context(0)
    dev = torch.device("cuda", 0)
    t0 = time.perf_counter()
    csr = synthetic_system(lg)
    nnz = int(csr[3].size)
    t1 = time.perf_counter()
    system = R1CS.from_csr(*csr, ctx=ctx)
    t2 = time.perf_counter()
    print("r1cs evaluation quickbench: 2^%d constraints, %d wires, %d terms (%.1f per row), dictionary of %d" % (lg, n, nnz, nnz / (3 * n), N_DICT))
    print("SYNTHETIC system, the mix is an ASSUMPTION: " + MIX)
    print("generated in %.1f s; validated, classified, binned and uploaded in %.1f s" % (t1 - t0, t2 - t1))
    shares = bin_shares(csr[2], BIN_LIMITS)
    for k, (rows, terms) in enumerate(shares):
        print("  bin %d (%s terms, %d lane%s per row): %d rows (%.1f %%), %d terms (%.1f %%)"
              % (k, ["<= %d" % BIN_LIMITS[0], "%d-%d" % (BIN_LIMITS[0] + 1, BIN_LIMITS[1]), "> %d" % BIN_LIMITS[1]][k], (1, 8, 64)[k],
                 "" if k == 0 else "s", rows, 100.0 * rows / (3 * n), terms, 100.0 * terms / max(nnz, 1)))
    print("  most terms: bin %d (the per-kernel times: this tool with PARTS=1 under rocprofv3 --kernel-trace --stats)" % max(range(3), key=lambda k: shares[k][1]))
    del csr
    rng = np.random.default_rng(3)
    w = rng.integers(0, 2**63, size=(n, 4), dtype=np.uint64)
    w[:, 3] &= np.uint64((1 << 60) - 1)
    w[0] = [1, 0, 0, 0]
    d_w = torch.from_numpy(w.view(np.int64)).to(dev)
    a, b, c = (torch.empty((n, 4), dtype=torch.int64, device=dev) for _ in range(3))
    d_sum = torch.zeros(2, dtype=torch.int64, device=dev)
    stream = torch.cuda.ExternalStream(ctx.stream_ptr(), device=dev)
    torch.cuda.synchronize(dev)

    # ---- 1. the evaluation alone
    alone = {}
    for check in (False, True):
        ms = []
        for i in range(3 + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            system.enqueue(ctx, d_w, n, a, b, c, d_sum if check else None)
            e1.record(stream)
            ctx.synchronize()
            if i >= 3:
                ms.append(e0.elapsed_time(e1))
        alone[check] = ms
        byts = nnz * (8 + 32) + 3 * n * 32
        print("1. evaluation alone, check=%s: %s" % (check, stats(ms)))
        print("   algorithmic bytes %.3f GB -> %.2f TB/s at the median (HBM peak 8 TB/s; information only)"
              % (byts / 1e9, byts / 1e12 / (statistics.median(ms) * 1e-3)))
    count, first = summary_tuple(d_sum.cpu().numpy().view(np.uint64))
    print("   summary: %d unsatisfied, first %s (the system is satisfied by construction)" % (count, first))
    assert count == 0 and first is None
    print("3a. check=True over check=False, evaluation alone: %+.2f ms at the medians"
          % (statistics.median(alone[True]) - statistics.median(alone[False])))
    if "2" not in parts:
        return
    abc = tuple(t.cpu().numpy().view(np.uint64) for t in (a, b, c))
    del a, b, c

    # ---- 2. whole proofs, old path and new path alternating
    t0 = time.perf_counter()
    gp = Groth16Prover(ctx, synthetic_key(n), system)
    print("key resident after %.1f s" % (time.perf_counter() - t0))
    p_old = gp.prove_words(w, abc, 12345, 67890)
    p_new = gp.prove_witness_words(w, 12345, 67890, check=True)
    assert p_old == p_new, "prove_witness_words differs from prove_words on the evaluated a, b, c"
    print("prove_witness_words == prove_words given the evaluated a, b, c (8 words)")
    old, new, new_nocheck, ev = [], [], [], []
    for _ in range(n_proofs):
        t0 = time.perf_counter()
        gp.prove_words(w, abc, 12345, 67890)
        old.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        gp.prove_witness_words(w, 12345, 67890, check=True)
        new.append((time.perf_counter() - t0) * 1e3)
        ev.append(gp.last_ms["r1cs_eval_device"])
        if "3" in parts:
            t0 = time.perf_counter()
            gp.prove_witness_words(w, 12345, 67890, check=False)
            new_nocheck.append((time.perf_counter() - t0) * 1e3)
    print("2. whole proof, prove_words(w, abc precomputed):      " + stats(old))
    print("   whole proof, prove_witness_words(w, check=True):   " + stats(new))
    print("   evaluation + check inside the proof (device events, beside the sums of the other streams): " + stats(ev))
    over = statistics.median(new) - statistics.median(old)
    spread = max(old) - min(old)
    print("   acceptance (new median - old median = %+.2f ms <= old spread %.2f ms): %s" % (over, spread, "PASS" if over <= spread else "FAIL"))
    if new_nocheck:
        print("3b. whole proof, prove_witness_words(w, check=False): " + stats(new_nocheck))
        print("    check=True over check=False, whole proof: %+.2f ms at the medians" % (statistics.median(new) - statistics.median(new_nocheck)))
    gp.close()
    system.close()


if __name__ == "__main__":
    main()
