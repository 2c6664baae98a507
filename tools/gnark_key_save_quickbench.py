"""Encoding of a gnark proving key's point arrays and the writing of a key file: (a) the kernels of csrc/gnark_points_encode.hip on
words resident in HBM (enqueue to settled stream, host clock), each beside the DECODING kernel of the same form timed in the same
run on the same points, (a2) gnark_keys.encode_points_dev followed by the read-back of the bytes, (b) the host path at 16 threads,
(c) gnark_keys.save_pk of a synthetic key at 2^16 wires, on the GPU and on host threads, against the Python path
(pk_to_gnark_bytes on words_to_points of the same key), (d) save_pk alone at 2^20 wires with its split: waiting for the device
(kernels and read-backs), writing the file, the rest.

    python tools/gnark_key_save_quickbench.py [--reps 7] [--sizes 65536,1048576] [--out profiles/gnark_key_save_quickbench.json]

Points: 512 multiples of the generator (both signs of y), repeated to n -- the work of an encoding does not depend on the values.
A synthetic key of w wires: A, B1, K of w points, Z of w - 1, B2 of w points, no point at infinity.  Each variant is warmed up at
each size; the profiler is off; encode and decode kernels alternate inside one loop.  The file of (c) and (d) is written to
--dir (default: the system's temporary directory) and removed.  No time is asserted anywhere: the comparison the project asks for
(the median of a raw encode kernel against the median of the raw decode kernel of its group, with that kernel's min-to-max spread
as the margin) is computed and recorded under "raw_encode_vs_decode".
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = [("g1_raw", False, False), ("g1_compressed", False, True), ("g2_raw", True, False), ("g2_compressed", True, True)]


def _points(g2, count=512):
    from oracle import bn254 as B
    gen, add, neg = (B.G2, B.g2_add, B.g2_neg) if g2 else (B.G1, B.add, B.neg)
    out, p = [], gen
    for i in range(count):
        out.append(neg(p) if i & 1 else p)
        p = add(p, gen)
    return out


def _tile(block, n):
    import numpy as np
    return np.ascontiguousarray(np.tile(block, (n // len(block) + 1, 1))[:n])


def synthetic_key(blocks, wires):
    """-> the dictionary save_pk takes, with *_words arrays"""
    import numpy as np
    g1, g2 = blocks[False], blocks[True]
    pk = {"n": wires, "n_public": 1, "infinity_a": np.zeros(wires, dtype=bool), "infinity_b": np.zeros(wires, dtype=bool),
          "A_words": _tile(g1, wires), "B1_words": _tile(g1[3:], wires), "K_words": _tile(g1[5:], wires), "Z_words": _tile(g1[7:], wires - 1),
          "B2_words": _tile(g2, wires)}
    for i, name in enumerate(("alpha1", "beta1", "delta1")):
        pk[name + "_words"] = g1[i].copy()
    for i, name in enumerate(("beta2", "delta2")):
        pk[name + "_words"] = g2[i].copy()
    return pk


def key_bytes(wires, raw=True):
    s1, s2 = (64, 128) if raw else (32, 64)
    return 8 + 5 * 32 + 3 * s1 + 4 * 4 + (4 * wires - 1) * s1 + 2 * s2 + 4 + wires * s2 + 24 + 2 * wires


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--python-wires", type=int, default=1 << 16)
    ap.add_argument("--save-wires", type=int, default=1 << 20)
    ap.add_argument("--dir", default=tempfile.gettempdir())
    ap.add_argument("--host-only", action="store_true", help="skip the GPU variants (a machine without one)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gnark_key_save_quickbench.json"))
    a = ap.parse_args()
    import numpy as np
    import zklc_amd
    from zklc_amd import _lib, gnark_keys as K
    med = statistics.median
    res = {"workload": "512 multiples of the generator repeated to n points; valid points only; validation off in (a), (a2), (b), "
                       "on in (c), (d)", "reps": a.reps, "host_threads": 16, "sizes": {}, "raw_encode_vs_decode": {}}
    blocks = {g2: K.points_to_words(_points(g2), g2=g2) for g2 in (False, True)}
    files = {(g2, c): b"".join((K.write_g2 if g2 else K.write_g1)(p, not c) for p in K.words_to_points(blocks[g2], g2=g2))
             for _, g2, c in FORMS}
    ctx = None if a.host_only else zklc_amd.Context(0)
    if ctx is not None:
        import torch
        dev = torch.device("cuda", ctx.device_id)
    for n in [int(x) for x in a.sizes.split(",")]:
        res["sizes"][str(n)] = {}
        for name, g2, compressed in FORMS:
            stride, width = K._stride(g2, compressed), 16 if g2 else 8
            words = _tile(blocks[g2], n)
            flags = _lib.POINTS_COMPRESSED if compressed else 0
            r = {"bytes_in": n * width * 8, "bytes_out": n * (stride + 4)}
            if ctx is not None:
                d_words = torch.from_numpy(words.view(np.int64)).to(dev)
                d_bytes = torch.empty(n * stride, dtype=torch.uint8, device=dev)
                d_status = torch.empty(n, dtype=torch.int32, device=dev)
                d_summary = torch.zeros(4, dtype=torch.int64, device=dev)
                # the decoder's side: the file bytes of the same points, and its own outputs
                f_bytes = torch.from_numpy(np.frombuffer(files[(g2, compressed)] * (n // 512 + 1), dtype=np.uint8)[:n * stride].copy()).to(dev)
                f_words = torch.empty((n, width), dtype=torch.int64, device=dev)
                torch.cuda.synchronize(dev)
                te, td, t2 = [], [], []
                for rep in range(a.reps + 1):                           # the first round is the warm-up
                    t = time.perf_counter()
                    ctx.bn254_points_encode_dev(d_words, n, d_bytes, d_status, d_summary, group=2 if g2 else 1, flags=flags,
                                                stream=ctx.stream_ptr())
                    ctx.synchronize()
                    t1 = time.perf_counter()
                    ctx.bn254_points_decode_dev(f_bytes, n, f_words, d_status, d_summary, group=2 if g2 else 1, flags=flags,
                                                stream=ctx.stream_ptr())
                    ctx.synchronize()
                    if rep:
                        te.append((t1 - t) * 1e3)
                        td.append((time.perf_counter() - t1) * 1e3)
                assert d_summary.cpu().tolist() == [n, 0, 0, -1], name
                assert torch.equal(f_words, d_words) and torch.equal(d_bytes, f_bytes), name      # each is the other's inverse
                for rep in range(min(a.reps, 3) + 1):
                    t = time.perf_counter()
                    data, _, summary = K.encode_points_dev(ctx, d_words, n, g2=g2, compressed=compressed)
                    host = data.cpu()
                    if rep:
                        t2.append((time.perf_counter() - t) * 1e3)
                assert summary == [n, 0, 0, None] and host.numpy()[:stride].tobytes() == files[(g2, compressed)][:stride]
                r.update({"a_encode_kernel_ms_median": med(te), "a_encode_all": te, "a_encode_ns_per_point": med(te) * 1e6 / n,
                          "a_encode_gbytes_per_s_in_plus_out": (r["bytes_in"] + r["bytes_out"]) / med(te) / 1e6,
                          "a_decode_kernel_ms_median": med(td), "a_decode_all": td, "a_decode_spread_ms": max(td) - min(td),
                          "a_encode_over_decode": med(te) / med(td),
                          "a2_encode_with_readback_ms_median": med(t2), "a2_all": t2})
                del d_words, d_bytes, d_status, f_bytes, f_words, data, host
            tb = []
            for rep in range(1 if n > 65536 else 2):
                t = time.perf_counter()
                _, _, summary = K.encode_points_host(words, n, g2=g2, compressed=compressed, nthreads=16)
                tb.append((time.perf_counter() - t) * 1e3)
            assert summary == [n, 0, 0, None]
            r.update({"b_host16_ms": min(tb), "b_all": tb, "b_us_per_point": min(tb) * 1e3 / n})
            if "a_encode_kernel_ms_median" in r:
                r["b_over_a"] = min(tb) / r["a_encode_kernel_ms_median"]
            res["sizes"][str(n)][name] = r
            print(n, name, json.dumps(r), flush=True)
        if ctx is not None:
            s = res["sizes"][str(n)]
            for group in ("g1", "g2"):
                raw, comp = s[group + "_raw"], s[group + "_compressed"]
                res["raw_encode_vs_decode"]["%s_%d" % (group, n)] = {
                    "encode_ms_median": raw["a_encode_kernel_ms_median"], "decode_ms_median": raw["a_decode_kernel_ms_median"],
                    "decode_spread_ms": raw["a_decode_spread_ms"],
                    "encode_within_decode_plus_spread": raw["a_encode_kernel_ms_median"] <= raw["a_decode_kernel_ms_median"] + raw["a_decode_spread_ms"],
                    "compressed_encode_ms_median": comp["a_encode_kernel_ms_median"],
                    "compressed_over_raw_encode": comp["a_encode_kernel_ms_median"] / raw["a_encode_kernel_ms_median"]}
            print(n, "raw encode against raw decode", json.dumps({k: v for k, v in res["raw_encode_vs_decode"].items() if k.endswith(str(n))}),
                  flush=True)
    # (c), (d): whole key files
    path = os.path.join(a.dir, "gnark_key_save_quickbench_%d.bin" % os.getpid())

    def timed_save(pk, **kw):
        stats = {}
        t = time.perf_counter()
        nbytes = K.save_pk(pk, path, stats=stats, **kw)
        wall = time.perf_counter() - t
        os.remove(path)
        out = {"wall_s": wall, "file_bytes": nbytes, "gbytes_per_s": nbytes / wall / 1e9}
        out.update({k: v for k, v in stats.items()})
        out["other_s"] = wall - sum(stats.values())
        return out

    def on_device(pk):
        """the five arrays as *_dev tensors, as KeySetup.run leaves them"""
        arrays = ("A_words", "B1_words", "K_words", "Z_words", "B2_words")
        return {(k[:-6] + "_dev" if k in arrays else k): (torch.from_numpy(v.view(np.int64)).to(dev) if k in arrays else v)
                for k, v in pk.items()}

    try:
        w = a.python_wires
        pk = synthetic_key(blocks, w)
        c = {"wires": w, "file_bytes": key_bytes(w)}
        t = time.perf_counter()
        ints = {"n": w, "infinity_a": pk["infinity_a"], "infinity_b": pk["infinity_b"]}
        for name in ("A", "B1", "Z", "K", "B2"):
            ints[name] = K.words_to_points(pk[name + "_words"], g2=name == "B2")
        for name in ("alpha1", "beta1", "delta1", "beta2", "delta2"):
            ints[name] = K.words_to_points(pk[name + "_words"], g2=name.endswith("2"))[0]
        t1 = time.perf_counter()
        want = K.pk_to_gnark_bytes(ints)
        t2 = time.perf_counter()
        assert len(want) == c["file_bytes"]
        c["python"] = {"words_to_points_s": t1 - t, "pk_to_gnark_bytes_s": t2 - t1, "wall_s": t2 - t}
        K.save_pk(pk, path, nthreads=16)
        assert open(path, "rb").read() == want
        c["save_pk_host16"] = min((timed_save(pk, nthreads=16) for _ in range(2)), key=lambda x: x["wall_s"])
        if ctx is not None:
            dpk = on_device(pk)
            K.save_pk(dpk, path, ctx=ctx)
            assert open(path, "rb").read() == want
            c["save_pk_gpu"] = min((timed_save(dpk, ctx=ctx) for _ in range(3)), key=lambda x: x["wall_s"])
            c["python_over_save_pk_gpu"] = c["python"]["wall_s"] / c["save_pk_gpu"]["wall_s"]
        c["python_over_save_pk_host16"] = c["python"]["wall_s"] / c["save_pk_host16"]["wall_s"]
        res["c_save_pk_against_python"] = c
        print("c", json.dumps(c), flush=True)
        del want, ints
        w = a.save_wires
        d = {"wires": w, "file_bytes": key_bytes(w)}
        if ctx is not None:
            dpk = on_device(synthetic_key(blocks, w))
            runs = [timed_save(dpk, ctx=ctx) for _ in range(4)][1:]                 # the first run pins the staging buffers' pages
            best = min(runs, key=lambda x: x["wall_s"])
            assert best["file_bytes"] == d["file_bytes"]
            d.update({"save_pk_gpu": best, "save_pk_gpu_all_wall_s": [x["wall_s"] for x in runs],
                      "bound_by": max(("device_wait_s", "write_s", "other_s"), key=lambda k: best.get(k, 0.0))})
            res["d_save_pk"] = d
            print("d", json.dumps(d), flush=True)
    finally:
        if os.path.exists(path):
            os.remove(path)
    if ctx is not None:
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
