#!/usr/bin/env python3
"""`groth16.Setup` on the GPU at 2^log_n constraints, stage by stage:
    python tools/groth16_setup_quickbench.py [log_n=22] [runs=5] [warmups=2]
Device events around every stage of `KeySetup.run()`: the scalar stage's transposition (with the call's one host wait), powers,
Lagrange values (the inverse transform), column sums and combination (zklc_groth16_setup_last_timings), and each of the five
multiplications of the point stage (A, B1, K, Z in G1; B2 in G2).  Medians of `runs` runs after `warmups` warm-ups; every run
draws nothing and clears its buffers (the toxic waste is fixed: this is a benchmark, not a ceremony).  In the same process, the
same system's row evaluation (zklc_r1cs_abc_dev) as the yardstick of the column sums: the same products over the same terms.
Peak device memory: torch's own high-water mark (every scalar, point array and workspace of a run is a torch tensor; the scalars
stay alive until the run's clear(), a fixed-base workspace until its multiplication has run) plus the two fixed-base tables, which
are the library's allocations.

THE SYSTEM IS SYNTHETIC AND ITS MIX IS AN ASSUMPTION: the one of tools/r1cs_eval_quickbench.py (see there).  What matters here: the
wires are drawn uniformly, so a column has about as many terms as a row on average, but wire 0 is the first term of EVERY B row: one
column of 2^log_n terms, the case the segment split exists for."""
import statistics
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
import numpy as np

TOXIC = (0x1234567891abcdef1234567891abcdef, 0xabcdef12345, 0x777766665555, 0x3133731337, 0x42424242)
N_PUBLIC = 4


def med(xs):
    return "median %8.3f ms  min %8.3f  max %8.3f" % (statistics.median(xs), min(xs), max(xs))


def main():
    import torch
    import zklc_amd
    from r1cs_eval_quickbench import MIX, synthetic_system
    from zklc_amd import groth16_setup as GS
    from zklc_amd.r1cs import R1CS
    lg = int(sys.argv[1]) if len(sys.argv) > 1 else 22
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    warm = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    n = 1 << lg
    ctx = zklc_amd.Context(0)
    dev = torch.device("cuda", 0)
    t0 = time.perf_counter()
    csr = synthetic_system(lg)
    nnz = int(csr[3].size)
    system = R1CS.from_csr(*csr, ctx=ctx)
    del csr
    print("groth16 setup quickbench: 2^%d constraints, %d wires, %d terms, n_public %d, window 16" % (lg, n, nnz, N_PUBLIC))
    print("SYNTHETIC system, the mix is an ASSUMPTION: " + MIX)
    print("system generated and resident after %.1f s" % (time.perf_counter() - t0))
    t0 = time.perf_counter()
    plan = GS.plan(system)
    print("plan (host, %.1f s): %s; segments of %d terms" % (time.perf_counter() - t0, plan, GS.SEG_TERMS))
    ws_bytes = int(ctx._lib.zklc_groth16_setup_workspace_bytes(system._handle(), n))
    print("scalar-stage workspace: %.3f GB" % (ws_bytes / 1e9))

    # ---- the yardstick: the row evaluation of the same system
    rng = np.random.default_rng(3)
    w = rng.integers(0, 2**63, size=(n, 4), dtype=np.uint64)
    w[:, 3] &= np.uint64((1 << 60) - 1)
    d_w = torch.from_numpy(w.view(np.int64)).to(dev)
    a, b, c = (torch.empty((n, 4), dtype=torch.int64, device=dev) for _ in range(3))
    stream = torch.cuda.ExternalStream(ctx.stream_ptr(), device=dev)
    torch.cuda.synchronize(dev)
    rows_ms = []
    for i in range(warm + runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        system.enqueue(ctx, d_w, n, a, b, c, None)
        e1.record(stream)
        ctx.synchronize()
        if i >= warm:
            rows_ms.append(e0.elapsed_time(e1))
    del a, b, c, d_w
    torch.cuda.empty_cache()
    print("row evaluation (zklc_r1cs_abc_dev, no check), same system, same process: " + med(rows_ms))

    # ---- Setup, stage by stage
    total = torch.cuda.mem_get_info(dev)[1]
    torch.cuda.reset_peak_memory_stats(dev)
    per, wall = {}, []
    for i in range(warm + runs):
        ks = GS.KeySetup(ctx, system, N_PUBLIC, TOXIC, window_bits=16)
        t0 = time.perf_counter()
        pk, vk = ks.run(timings=True)
        t1 = time.perf_counter()
        if i == 0:
            got = ks.scalars.plan()                       # the head of the scalar stage's workspace: the device's own count
            print("plan (device): %s -- %s" % (got, "the host's" if got == plan else "DIFFERS from the host's"))
            print("key: %d A, %d B1 / B2, %d K, %d Z points; %d / %d wires without an A / B point"
                  % (len(pk["A_dev"]), len(pk["B1_dev"]), len(pk["K_dev"]), len(pk["Z_dev"]), int(pk["infinity_a"].sum()), int(pk["infinity_b"].sum())))
        ks.clear()
        if i >= warm:
            wall.append((t1 - t0) * 1e3)
            for k, v in ks.last_ms.items():
                per.setdefault(k, []).append(v)
        del pk, vk, ks
    scalar = [sum(per[s][i] for s in GS.STAGES) for i in range(runs)]
    points = [sum(per["points_" + s][i] for s in ("A", "B1", "K", "Z", "B2")) for i in range(runs)]
    print("scalar stage, device events (%d runs after %d warm-ups):" % (runs, warm))
    for s in GS.STAGES:
        print("  %-14s %s%s" % (s, med(per[s]), "   (includes the call's one host wait)" if s == "transposition" else ""))
    print("  %-14s %s" % ("whole", med(scalar)))
    print("point stage, device events:")
    for s in ("A", "B1", "K", "Z", "B2"):
        print("  %-14s %s" % (s + (" (G2)" if s == "B2" else " (G1)"), med(per["points_" + s])))
    print("  %-14s %s" % ("whole", med(points)))
    print("KeySetup.run() wall clock (tables, masks, compaction and read-backs included): " + med(wall))
    cs, rw = statistics.median(per["column_sums"]), statistics.median(rows_ms)
    print("column sums / row evaluation: %.2f (%.3f ms / %.3f ms)%s" % (cs / rw, cs, rw, "  -- above 2: see the counter run" if cs > 2 * rw else ""))
    sm, pm = statistics.median(scalar), statistics.median(points)
    print("scalar stage / point stage: %.2f (%.3f ms / %.3f ms)" % (sm / pm, sm, pm))
    from zklc_amd import fixed_base as FB
    tables = sum(int(ctx._lib.zklc_bn254_fixed_base_table_bytes(g, 16)) for g in (FB.G1, FB.G2))
    hw = torch.cuda.max_memory_allocated(dev)
    print("peak device memory: torch high-water %.3f GB + the two tables %.3f GB = %.3f GB of %.1f GB"
          % (hw / 1e9, tables / 1e9, (hw + tables) / 1e9, total / 1e9))
    system.close()


if __name__ == "__main__":
    main()
