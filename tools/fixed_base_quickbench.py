#!/usr/bin/env python3
"""Batched fixed-base multiplication on the GPU (zklc_bn254_g{1,2}_fixed_mul_dev), the point stage of `groth16.Setup`:
    python tools/fixed_base_quickbench.py [log_n=22] [reps=5] [out=profiles/fixed_base_quickbench.txt]
For window_bits 12..16 and both groups: the table's bytes and its build time (wall clock, the call returns when the table is
complete), then 2^log_n uniformly random scalars below r (what the scalars of a key look like: every digit non-zero with probability
1 - 2^-c) through the table -- device events around the enqueue of both stages, warmed, `reps` repetitions.  WINDOWS=16 REPS=1
(environment) is the form to put under `rocprofv3 --kernel-trace --stats` for the split between the stages.
Beside each time: mixed additions per second = n x ceil(254 / c) / time, against the one comparable figure of the repository, the G1
bucket kernel of the multi-exponentiation: 2^22 x 16 additions in 6.93 ms = 9.68e9 / s (profiles/r05f_*).
The host twin on 16 threads at 2^16 scalars, for scale.  Peak device memory of a G1 / G2 multiplication = table + scalars + output +
workspace; everything but the output goes back to the allocator."""
import os
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np

R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
MSM_ADDS_PER_S = (1 << 22) * 16 / 6.93e-3


def random_scalars(n, seed):
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 2**63, size=(n, 4), dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    w[:, 3] &= np.uint64((1 << 61) - 1)          # below 2^253 < r
    return w


def main():
    import torch
    import zklc_amd
    from zklc_amd import fixed_base as FB
    lg = int(sys.argv[1]) if len(sys.argv) > 1 else 22
    reps = int(os.environ.get("REPS", sys.argv[2] if len(sys.argv) > 2 else 5))
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join("profiles", "fixed_base_quickbench.txt")
    windows = [int(x) for x in os.environ.get("WINDOWS", "12,13,14,15,16").split(",")]
    n = 1 << lg
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    ctx = zklc_amd.Context(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.ExternalStream(ctx.stream_ptr(), device=dev)
    say("fixed-base multiplication quickbench: 2^%d uniformly random scalars below r, one MI355X, %d repetitions after 2" % (lg, reps))
    say("reference rate: G1 bucket kernel of the multi-exponentiation, 2^22 x 16 additions in 6.93 ms = %.2fe9 additions / s" % (MSM_ADDS_PER_S / 1e9))
    d_s = torch.from_numpy(random_scalars(n, 11).view(np.int64)).to(dev)
    for group, name in ((FB.G1, "G1"), (FB.G2, "G2")):
        words = torch.empty((n, 16 if group == FB.G2 else 8), dtype=torch.int64, device=dev)
        summary = torch.empty(2, dtype=torch.int64, device=dev)
        for c in windows:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            tab = FB.FixedBase(ctx, group, None, c)
            build_ms = (time.perf_counter() - t0) * 1e3
            ws = torch.empty(tab.workspace_bytes(n), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)
            ms = []
            for i in range(2 + reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                tab.enqueue(d_s, words, summary, ws)
                e1.record(stream)
                ctx.synchronize()
                if i >= 2:
                    ms.append(e0.elapsed_time(e1))
            med = statistics.median(ms)
            rows = -(-254 // c)
            rate = n * rows / (med * 1e-3)
            inf = FB.summary_tuple(summary.cpu().numpy().view(np.uint64))
            peak = tab.table_bytes() + n * 32 + words.numel() * 8 + ws.numel()
            say("%s c = %2d: table %6.1f MB built in %7.1f ms (wall); %d rows; multiplication median %7.2f ms (min %.2f, max %.2f) = %.2fe9 additions / s "
                "= %.2f x the reference rate; workspace %.0f MB, peak %.2f GB; infinities %s"
                % (name, c, tab.table_bytes() / 1e6, build_ms, rows, med, min(ms), max(ms), rate / 1e9, rate / MSM_ADDS_PER_S, ws.numel() / 1e6, peak / 1e9, inf))
            ws.zero_()
            del ws
            tab.close()
        del words
    # the host twin, for scale
    hn = 1 << 16
    hs = random_scalars(hn, 12)
    for group, name, c in ((FB.G1, "G1", 13), (FB.G2, "G2", 13)):
        t0 = time.perf_counter()
        tab = FB.FixedBase(None, group, None, c)
        t1 = time.perf_counter()
        tab.mul_host(hs, nthreads=16)
        t2 = time.perf_counter()
        say("host twin %s c = %d, 16 threads: table in %.0f ms, 2^16 scalars in %.0f ms (%.2fe6 additions / s)"
            % (name, c, (t1 - t0) * 1e3, (t2 - t1) * 1e3, hn * -(-254 // c) / (t2 - t1) / 1e6))
        tab.close()
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
