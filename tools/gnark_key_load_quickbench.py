"""Decoding of a gnark proving key's point arrays: (a) the kernels of csrc/gnark_points.hip on bytes resident in HBM (enqueue to
settled stream, host clock), (a2) the same through gnark_keys.decode_points_dev, upload included, (b) the host path at 16 threads,
(c) the point-by-point Python reader (gnark_keys._read_points + points_to_words) on 2000 points for scale.

    python tools/gnark_key_load_quickbench.py [--reps 5] [--sizes 65536,1048576] [--out profiles/gnark_key_load_quickbench.json]

Points: 512 multiples of the generator (both signs of y), repeated to n -- the work of a decoding does not depend on the values, and
every point is valid, so the membership test runs in full on every lane.  Each variant is warmed up at each size; the profiler is
off.  (b) is timed once per size above 2^16 points (seconds per run).  No time is asserted anywhere.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = [("g1_raw", False, False, False), ("g1_compressed", False, True, False), ("g2_raw", True, False, False),
            ("g2_compressed", True, True, False), ("g2_raw_checked", True, False, True), ("g2_compressed_checked", True, True, True)]


def _points(g2, count=512):
    from oracle import bn254 as B
    gen, add, neg = (B.G2, B.g2_add, B.g2_neg) if g2 else (B.G1, B.add, B.neg)
    out, p = [], gen
    for i in range(count):
        out.append(neg(p) if i & 1 else p)
        p = add(p, gen)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--python-points", type=int, default=2000)
    ap.add_argument("--host-only", action="store_true", help="skip the GPU variants (a machine without one)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gnark_key_load_quickbench.json"))
    a = ap.parse_args()
    import numpy as np
    import zklc_amd
    from zklc_amd import _lib, gnark_keys as K
    med = statistics.median
    res = {"workload": "512 multiples of the generator repeated to n points; valid points only", "reps": a.reps, "host_threads": 16,
           "sizes": {}, "python_reader": {}}
    pts = {False: _points(False), True: _points(True)}
    blocks = {}
    for name, g2, compressed, _ in VARIANTS:
        write = K.write_g2 if g2 else K.write_g1
        blocks[(g2, compressed)] = b"".join(write(p, not compressed) for p in pts[g2])
    # (c) the Python reader
    for name, g2, compressed, checked in VARIANTS:
        if checked:
            continue
        m = a.python_points
        block = blocks[(g2, compressed)]
        data = (m.to_bytes(4, "big") + block * (m // 512 + 1))[:4 + m * K._stride(g2, compressed)]
        t = time.perf_counter()
        got = K._read_points(K._Reader(data), K.read_g2 if g2 else K.read_g1, (64 if g2 else 32) if not compressed else 0)
        t1 = time.perf_counter()
        K.points_to_words(got, g2=g2)
        t2 = time.perf_counter()
        res["python_reader"][name] = {"points": m, "read_us_per_point": (t1 - t) * 1e6 / m, "to_words_us_per_point": (t2 - t1) * 1e6 / m}
        print("python", name, json.dumps(res["python_reader"][name]), flush=True)
    ctx = None if a.host_only else zklc_amd.Context(0)
    if ctx is not None:
        import torch
        dev = torch.device("cuda", ctx.device_id)
    for n in [int(x) for x in a.sizes.split(",")]:
        res["sizes"][str(n)] = {}
        for name, g2, compressed, checked in VARIANTS:
            stride, width = K._stride(g2, compressed), 16 if g2 else 8
            data = np.frombuffer(blocks[(g2, compressed)] * (n // 512 + 1), dtype=np.uint8)[:n * stride]
            flags = (_lib.POINTS_COMPRESSED if compressed else 0) | (_lib.POINTS_CHECK_SUBGROUP if checked else 0)
            r = {"bytes_in": n * stride, "bytes_out": n * (width * 8 + 4)}
            if ctx is not None:
                d_bytes = torch.from_numpy(data.copy()).to(dev)
                d_words = torch.empty((n, width), dtype=torch.int64, device=dev)
                d_status = torch.empty(n, dtype=torch.int32, device=dev)
                d_summary = torch.zeros(4, dtype=torch.int64, device=dev)
                torch.cuda.synchronize(dev)
                ta, tu = [], []
                for rep in range(a.reps + 1):                           # the first run is the warm-up
                    t = time.perf_counter()
                    ctx.bn254_points_decode_dev(d_bytes, n, d_words, d_status, d_summary, group=2 if g2 else 1, flags=flags,
                                                stream=ctx.stream_ptr())
                    ctx.synchronize()
                    if rep:
                        ta.append((time.perf_counter() - t) * 1e3)
                assert d_summary.cpu().tolist() == [n, 0, 0, -1], name
                for rep in range(min(a.reps, 3) + 1):
                    t = time.perf_counter()
                    _, _, summary = K.decode_points_dev(ctx, data, n, g2=g2, compressed=compressed, check_subgroup=checked)
                    if rep:
                        tu.append((time.perf_counter() - t) * 1e3)
                assert summary == [n, 0, 0, None]
                r.update({"a_gpu_kernels_ms_median": med(ta), "a_all": ta, "a_ns_per_point": med(ta) * 1e6 / n,
                          "a_gbytes_per_s_in_plus_out": (r["bytes_in"] + r["bytes_out"]) / med(ta) / 1e6,
                          "a2_gpu_with_upload_ms_median": med(tu), "a2_all": tu})
                del d_bytes, d_words, d_status
            tb = []
            for rep in range(1 if n > 65536 else 2):
                t = time.perf_counter()
                _, _, summary = K.decode_points_host(data, n, g2=g2, compressed=compressed, check_subgroup=checked, nthreads=16)
                tb.append((time.perf_counter() - t) * 1e3)
            assert summary == [n, 0, 0, None]
            r.update({"b_host16_ms": min(tb), "b_all": tb, "b_us_per_point": min(tb) * 1e3 / n})
            if "a_gpu_kernels_ms_median" in r:
                r["b_over_a"] = min(tb) / med(ta)
            res["sizes"][str(n)][name] = r
            print(n, name, json.dumps(r), flush=True)
    if ctx is not None:
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
