"""Batched Groth16 verification: (a) NativeGroth16Verifier.verify_batch on the GPU with its last_timings breakdown, (b) the Python
path Groth16Verifier.verify looped over the same proofs (one proof per call: Python point checks, two multi-exponentiations and one
pairing launch, three host synchronisations), (c) verify_batch_host at 16 threads.

    python tools/groth16_verify_quickbench.py [--reps 5] [--out profiles/groth16_verify_quickbench.json]

Proofs: the reference's known-answer proof and key (tests/golden/groth16_kat.json, 4 public inputs), n copies per batch -- the work
of a verification does not depend on the values.  Each size is warmed up, the variants alternate inside one run, the profiler is
off.  (b) is a loop of identical calls: above --loop-cap proofs it is timed on the first --loop-cap of them and scaled by
n / loop_cap (recorded as "b_extrapolated": true).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1,16,256,2048")
    ap.add_argument("--loop-cap", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groth16_verify_quickbench.json"))
    a = ap.parse_args()
    import zklc_amd
    from zklc_amd import formats as F
    from zklc_amd.groth16 import Groth16Verifier, NativeGroth16Verifier
    import groth16_cases as C
    vk, proof, inputs, _, _ = C.kat()
    raw = F.proof_to_raw_bytes(proof)
    res = {"workload": "groth16_kat.json: 4 public inputs, n copies of the known-answer proof", "reps": a.reps, "sizes": {}}
    med = statistics.median
    with zklc_amd.Context(0) as ctx:
        new, old = NativeGroth16Verifier(ctx, vk), Groth16Verifier(ctx, vk)
        for n in [int(x) for x in a.sizes.split(",")]:
            ps, xs = [raw] * n, [inputs] * n
            nb = min(n, a.loop_cap)
            assert new.verify_batch(ps, xs) == [0] * n                  # warm-up of every variant at this size
            assert all(old.verify(proof, inputs) for _ in range(min(nb, 4)))
            assert new.verify_batch_host(ps, xs, nthreads=16) == [0] * n
            ta, tb, tc, parts = [], [], [], []
            for _ in range(a.reps):
                t = time.perf_counter()
                new.verify_batch(ps, xs)
                ta.append((time.perf_counter() - t) * 1e3)
                parts.append(new.last_timings())
                t = time.perf_counter()
                for _ in range(nb):
                    old.verify(proof, inputs)
                tb.append((time.perf_counter() - t) * 1e3 * n / nb)
                t = time.perf_counter()
                new.verify_batch_host(ps, xs, nthreads=16)
                tc.append((time.perf_counter() - t) * 1e3)
            r = {"a_gpu_batch_ms_median": med(ta), "a_all": ta, "a_breakdown_ms_median": {k: med(p[k] for p in parts) for k in parts[0]},
                 "a_breakdown_all": parts, "b_python_loop_ms_median": med(tb), "b_all": tb, "b_extrapolated": nb < n, "b_timed_proofs": nb,
                 "c_host16_ms_median": med(tc), "c_all": tc, "b_over_a": med(tb) / med(ta), "c_over_a": med(tc) / med(ta)}
            res["sizes"][str(n)] = r
            print(n, json.dumps(r), flush=True)
        new.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
