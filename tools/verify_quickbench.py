"""Native plonky2 verifier: a batch on the GPU (zklc_plonky2_verify_batch) against the host path at 16 threads
(zklc_plonky2_verify_batch_host), with the GPU call split into the host stage (parse, transcript, vanishing identity, reduced
openings), the Merkle kernel and the FRI kernel.

    python tools/verify_quickbench.py [--reps 5] [--out profiles/verify_quickbench.json]

Workloads: 73 proofs of the Ed25519-circuit shape (synthetic ed25519_shape_mix, 2^18 x 234, Poseidon-Goldilocks), 73 proofs of the
fold shape (recursion mix, 2^12 x 135, Goldilocks) and the reference's 4 golden Poseidon-BN128 proofs.  The verification work of a
proof does not depend on its values, so a batch is byte copies of one GPU-made proof (the golden batch: the 4 proofs).
"""
import argparse
import gzip
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _synthetic(shape, degree_bits):
    from zklc_amd.plonky2 import synthetic as SY, gates as G, standard_recursion_config, wide_ecc_config
    if shape == "recursion":
        cfg = standard_recursion_config()
        mix = SY.recursion_shape_mix(cfg) + [(G.ExponentiationGate(20), 3)]
    else:
        cfg = wide_ecc_config()
        mix = SY.ed25519_shape_mix(cfg)
    return SY.synthetic_circuit(degree_bits, cfg, mix, num_public_inputs=16, seed=5)


def _measure(v, batch, reps):
    v.verify_batch(batch)                                   # warm-up: kernels loaded, buffers grown
    gpu, parts = [], []
    for _ in range(reps):
        t = time.perf_counter()
        st = v.verify_batch(batch)
        gpu.append((time.perf_counter() - t) * 1e3)
        parts.append(v.last_timings())
    assert all(s == 0 for s in st), st
    host = []
    for _ in range(max(1, reps // 2)):
        t = time.perf_counter()
        sh = v.verify_batch_host(batch, threads=16)
        host.append((time.perf_counter() - t) * 1e3)
    assert sh == st
    med = statistics.median(gpu)
    return {"n": len(batch), "gpu_ms_median": med, "gpu_ms_all": gpu, "host16_ms_median": statistics.median(host),
            "speedup_vs_host16": statistics.median(host) / med,
            "gpu_breakdown_ms_median": {k: statistics.median(p[k] for p in parts) for k in parts[0]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import zklc_amd
    from zklc_amd.plonky2 import HASH_GL, serialization as S
    from zklc_amd.plonky2.verifier import Verifier
    res = {}
    with zklc_amd.Context(0) as ctx:
        for name, shape, bits in (("ed25519_2^18x234_gl", "ed25519", 18), ("fold_2^12x135_gl", "recursion", 12)):
            data, wires, pis = _synthetic(shape, bits)
            prover = data.prover(ctx, HASH_GL)
            raw = prover.prove_bytes(wires, pis)
            with Verifier.from_prover(prover) as v:
                res[name] = _measure(v, [raw] * 73, a.reps)
            prover.close()
            print(name, json.dumps(res[name]), flush=True)
        with gzip.open(os.path.join(ROOT, "tests", "golden", "plonky2_reference_proofs_full.json.gz")) as f:
            cases = json.load(f)
        # the four golden proofs are of two circuits (three share one common data): one verifier per circuit
        groups = {}
        for c in cases:
            groups.setdefault(json.dumps(c["common_data"], sort_keys=True) + json.dumps(c["verifier_data"], sort_keys=True), []).append(c)
        out = []
        for cs in groups.values():
            with Verifier(ctx, cs[0]["common_data"], cs[0]["verifier_data"]) as v:
                out.append(_measure(v, [S.proof_to_bytes(c["proof"], c["common_data"], v.hasher) for c in cs], a.reps))
        res["golden_bn128"] = out
        print("golden_bn128", json.dumps(out), flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
