"""`groth16.Setup(r1cs)` (gnark-plonky2-verifier/cmd/compile.go:40; gnark v0.9.1 backend/groth16/bn254/setup.go, un-vendored) on the
GPU: from a resident constraint system (zklc_amd/r1cs.py) to the proving key `Groth16Prover` takes and the verifying key the
verifiers take.  Two stages, both through the C ABI (include/zklc.h):

  scalars   zklc_groth16_setup_scalars_dev: the Lagrange values at tau, the columns of A, B, C summed against them, k and z --
            the discrete logarithms of the key's points, in regular form, in HBM
  points    zklc_bn254_g{1,2}_fixed_mul_dev over two tables of the generators (zklc_amd/fixed_base.py): A, B1, K, Z in G1, B2 in G2,
            the single multiples (alpha, beta, delta in G1; beta, gamma, delta in G2) at the end of the first batch of each group

Nothing on the data path is a Python integer; no CPU fallback for the device path.  `setup_host` is the same over the library's host
twins (the same lane functions, g++).  The toxic waste and everything computed from it is the caller's to destroy: `KeySetup.clear`
zero-fills every device tensor that held a scalar, `Setup` does so in a `finally`."""
import secrets

import numpy as np

from . import _lib
from . import fixed_base as FB

R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
_M64 = (1 << 64) - 1
SEG_TERMS = 2048          # csrc/groth16_setup.cuh: SETUP_SEG_TERMS, the longest column one wave sums
MAX_LOG_N = 28
PLAN_KEYS = ("cols_1_lane", "cols_8_lanes", "cols_64_lanes", "cols_segmented", "segments")
STAGES = ("transposition", "powers", "lagrange", "column_sums", "combination")


def domain_size(n_constraints):
    n = 2
    while n < n_constraints:
        n *= 2
    return n


def toxic_words(toxic):
    """(tau, alpha, beta, gamma, delta), integers below 2^256 -> uint64 [5, 4], regular form (the library reduces)"""
    t = [int(x) for x in toxic]
    if len(t) != 5 or any(x < 0 or x >> 256 for x in t):
        raise ValueError("groth16 setup: the toxic waste is five integers below 2^256")
    return np.array([[(x >> (64 * i)) & _M64 for i in range(4)] for x in t], dtype=np.uint64)


def random_toxic():
    """five values in [1, r) from the operating system's generator"""
    return tuple(1 + secrets.randbelow(R - 1) for _ in range(5))


def plan(r1cs):
    """how the device sums the system's columns: columns taken by 1 / 8 / 64 lanes, columns cut into segments of SEG_TERMS terms,
    and the number of segments (zklc_groth16_setup_plan: computed on the host from the system alone)"""
    out = np.zeros(5, dtype=np.uint64)
    rc = _lib.load().zklc_groth16_setup_plan(r1cs._handle(), out.ctypes.data)
    if rc != 0:
        raise _lib.ZklcError(rc, "zklc_groth16_setup_plan")
    return dict(zip(PLAN_KEYS, (int(x) for x in out)))


def last_timings():
    """milliseconds of the stages of this thread's last device scalar stage (device events; waits for its work)"""
    out = np.zeros(len(STAGES), dtype=np.float64)
    k = _lib.load().zklc_groth16_setup_last_timings(out.ctypes.data, len(STAGES))
    return dict(zip(STAGES[:k], out[:k].tolist()))


class DeviceScalars:
    """what `setup_scalars_dev` leaves in HBM: a_t, b_t, k int64 [n_wires, 4], z int64 [n - 1, 4] (regular form) and the call's
    workspace (uint8), which still holds functions of the toxic waste and, in its first five words, the plan the device made"""

    def __init__(self, n, a_t, b_t, k, z, workspace):
        self.n, self.a_t, self.b_t, self.k, self.z, self.workspace = n, a_t, b_t, k, z, workspace

    def plan(self):
        """the device's own count of its column lists (read after the stream has been waited for)"""
        return dict(zip(PLAN_KEYS, (int(x) & _M64 for x in self.workspace[:40].view(self.a_t.dtype).cpu().tolist())))

    def tensors(self):
        return [self.a_t, self.b_t, self.k, self.z, self.workspace]


def setup_scalars_dev(ctx, r1cs, n_public, toxic, n=None, stream=None, keep=None):
    """zklc_groth16_setup_scalars_dev on `stream` (default: ctx's own) -> DeviceScalars.  The call waits once on the stream (the
    sizes of the column lists) and returns with the rest enqueued: synchronise before reading.  keep: a list that receives the
    five tensors before the call is made (a caller that clears them whether the call succeeds or not)."""
    import torch
    lib = ctx._lib
    n = domain_size(r1cs.n_constraints) if n is None else int(n)
    tw = toxic_words(toxic)
    try:
        ws_bytes = int(lib.zklc_groth16_setup_workspace_bytes(r1cs._handle(), n))
        if ws_bytes == 0:
            raise _lib.ZklcError(-1, "zklc_groth16_setup_workspace_bytes: a domain of %d for %d constraints and %d wires"
                                 % (n, r1cs.n_constraints, r1cs.n_wires))
        dev = torch.device("cuda", ctx.device_id)
        a_t, b_t, k = (torch.empty((r1cs.n_wires, 4), dtype=torch.int64, device=dev) for _ in range(3))
        z = torch.empty((n - 1, 4), dtype=torch.int64, device=dev)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        if keep is not None:
            keep += [a_t, b_t, k, z, ws]
        torch.cuda.current_stream(dev).synchronize()      # torch hands blocks out on ITS stream; the kernels run on the context's
        ctx._check(lib.zklc_groth16_setup_scalars_dev(ctx._h, ctx.stream_ptr() if stream is None else stream, r1cs._handle(),
                                                      tw.ctypes.data, int(n_public), n, a_t.data_ptr(), b_t.data_ptr(), k.data_ptr(),
                                                      z.data_ptr(), ws.data_ptr(), ws.numel()))
    finally:
        tw.fill(0)
    return DeviceScalars(n, a_t, b_t, k, z, ws)


def setup_scalars_host(r1cs, n_public, toxic, n=None, nthreads=0):
    """the host twin -> (a_t, b_t, k, z): uint64 [n_wires, 4] x 3 and [n - 1, 4], regular form"""
    n = domain_size(r1cs.n_constraints) if n is None else int(n)
    tw = toxic_words(toxic)
    a_t, b_t, k = (np.empty((r1cs.n_wires, 4), dtype=np.uint64) for _ in range(3))
    z = np.empty((max(n - 1, 1), 4), dtype=np.uint64)
    try:
        rc = _lib.load().zklc_groth16_setup_scalars_host(r1cs._handle(), tw.ctypes.data, int(n_public), n, int(nthreads), a_t.ctypes.data,
                                                         b_t.ctypes.data, k.ctypes.data, z.ctypes.data)
    finally:
        tw.fill(0)
    if rc != 0:
        raise _lib.ZklcError(rc, "zklc_groth16_setup_scalars_host")
    return a_t, b_t, k, z[:n - 1]


def _vk(words):
    """the verifying key as integer tuples from the words of its seven kinds of point"""
    from .gnark_keys import words_to_points
    one = lambda name, g2=False: words_to_points(words[name], g2)[0]
    return {"alpha1": one("alpha1"), "beta1": one("beta1"), "delta1": one("delta1"), "beta2": one("beta2", True),
            "gamma2": one("gamma2", True), "delta2": one("delta2", True), "K": words_to_points(words["K_vk"])}


class KeySetup:
    """One run of Setup on one GPU.  r1cs: a zklc_amd.r1cs.R1CS resident on ctx's GPU; n_public: public inputs without the constant
    wire; toxic: (tau, alpha, beta, gamma, delta) or None = drawn from `secrets`.  `run()` -> (pk, vk); `clear()` destroys what is
    left of the toxic waste on the device and in this object."""

    def __init__(self, ctx, r1cs, n_public, toxic=None, window_bits=16):
        self.ctx, self.r1cs, self.n_public, self.window_bits = ctx, r1cs, int(n_public), int(window_bits)
        self.toxic = tuple(int(x) for x in toxic) if toxic is not None else random_toxic()
        self._bufs = []
        self.scalars = None          # the DeviceScalars of the last run (its tensors are zero after clear())
        self.last_ms = {}

    def buffers(self):
        """every device tensor that holds a scalar of the key or a workspace of the two stages.  A fixed-base workspace (the
        multiples of the caller's scalars) is listed while its multiplication runs and leaves the list zero-filled"""
        return list({id(t): t for t in self._bufs}.values())

    def _mul(self, table, d_scalars, name, events):
        """one multiplication of the point stage.  The scalars and the workspace are in `buffers()` from the moment they exist; the
        workspace (the multiples of the scalars as limbs: 200 / 400 bytes per point) is zero-filled and handed back as soon as its
        multiplication has run, so that one workspace is alive at a time"""
        import torch
        dev, n = d_scalars.device, d_scalars.shape[0]
        self._bufs.append(d_scalars)
        words = torch.empty((n, table.width), dtype=torch.int64, device=dev)
        summary = torch.empty(2, dtype=torch.int64, device=dev)
        ws = torch.empty(max(table.workspace_bytes(n), 16), dtype=torch.uint8, device=dev)
        self._bufs.append(ws)
        s = torch.cuda.ExternalStream(self.ctx.stream_ptr(), device=dev)
        torch.cuda.current_stream(dev).synchronize()       # torch hands blocks out on ITS stream; the kernels run on the context's
        if events is not None:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record(s)
        table.enqueue(d_scalars, words, summary, ws)
        if events is not None:
            ev[1].record(s)
            events[name] = ev
        with torch.cuda.stream(s):
            ws.zero_()
        self.ctx.synchronize()                             # the block goes back to torch's allocator only when nothing uses it
        self._bufs = [t for t in self._bufs if t is not ws]
        return words

    def run(self, timings=False):
        """-> (pk, vk).  pk: n, n_public, A_dev / B1_dev / B2_dev (points at infinity removed, as gnark stores them), K_dev, Z_dev
        (int64 device tensors in gnark-crypto's memory layout), infinity_a / infinity_b (bool [n_wires]) and alpha1_words ..
        delta2_words: what `Groth16Prover(ctx, pk, r1cs)` takes.  vk: alpha1, beta1, delta1, beta2, gamma2, delta2, K as integer
        tuples: what the verifiers and `vk_to_gnark_bytes` take.  timings=True: device events around the five multiplications,
        in `last_ms` with the stages of the scalar stage.  Every tensor that holds a scalar is in `buffers()` before the first
        kernel reads it: a run that raises half-way leaves nothing that `clear()` does not reach."""
        import torch
        ctx, npub = self.ctx, self.n_public
        if self.toxic is None:
            raise ValueError("groth16 setup: the toxic waste of this object has been cleared")
        dev = torch.device("cuda", ctx.device_id)
        sc = self.scalars = setup_scalars_dev(ctx, self.r1cs, npub, self.toxic, keep=self._bufs)
        tau, alpha, beta, gamma, delta = self.toxic
        singles = []
        for vals in ((alpha, beta, delta), (beta, gamma, delta)):
            h = FB.scalar_words([v % R for v in vals])
            try:
                singles.append(torch.from_numpy(h.view(np.int64)).to(dev))
                self._bufs.append(singles[-1])
                torch.cuda.current_stream(dev).synchronize()
            finally:
                h.fill(0)
        s1, s2 = singles
        ctx.synchronize()                                  # the scalars are complete before torch's stream joins them
        nw = self.r1cs.n_wires
        inf_a, inf_b = (sc.a_t == 0).all(dim=1), (sc.b_t == 0).all(dim=1)
        events = {} if timings else None
        with FB.FixedBase(ctx, FB.G1, window_bits=self.window_bits) as g1, FB.FixedBase(ctx, FB.G2, window_bits=self.window_bits) as g2:
            A = self._mul(g1, torch.cat([sc.a_t, s1]), "A", events)
            B1 = self._mul(g1, sc.b_t, "B1", events)
            K = self._mul(g1, sc.k, "K", events)
            Z = self._mul(g1, sc.z, "Z", events)
            B2 = self._mul(g2, torch.cat([sc.b_t, s2]), "B2", events)
        if timings:
            self.last_ms = dict(last_timings())
            self.last_ms.update({"points_" + k: e[0].elapsed_time(e[1]) for k, e in events.items()})
        host = lambda t: t.cpu().numpy().view(np.uint64).copy()
        words = {"alpha1": host(A[nw]), "beta1": host(A[nw + 1]), "delta1": host(A[nw + 2]), "beta2": host(B2[nw]),
                 "gamma2": host(B2[nw + 1]), "delta2": host(B2[nw + 2]), "K_vk": host(K[:npub + 1])}
        pk = {"n": sc.n, "n_public": npub, "A_dev": A[:nw][~inf_a], "B1_dev": B1[~inf_b], "B2_dev": B2[:nw][~inf_b],
              "K_dev": K[npub + 1:], "Z_dev": Z, "infinity_a": inf_a.cpu().numpy(), "infinity_b": inf_b.cpu().numpy()}
        for name in ("alpha1", "beta1", "delta1", "beta2", "delta2"):
            pk[name + "_words"] = words[name]
        torch.cuda.current_stream(dev).synchronize()
        return pk, _vk(words)

    def clear(self):
        """zero-fills `buffers()` on the context's stream, waits, and drops the toxic tuple"""
        import torch
        if self._bufs:
            dev = self._bufs[0].device
            torch.cuda.current_stream(dev).synchronize()
            with torch.cuda.stream(torch.cuda.ExternalStream(self.ctx.stream_ptr(), device=dev)):
                for t in self.buffers():
                    t.zero_()
            self.ctx.synchronize()
        self.toxic = None


def Setup(ctx, r1cs, n_public, toxic=None, window_bits=16):
    """`groth16.Setup(r1cs)`: -> (pk, vk) of `KeySetup.run`, with the toxic waste and its traces on the device destroyed whether the
    run succeeds or not.  The buffers of the run stay referenced by nothing afterwards: torch's allocator has them back, zeroed."""
    ks = KeySetup(ctx, r1cs, n_public, toxic, window_bits)
    try:
        return ks.run()
    finally:
        ks.clear()


def setup_host(r1cs, n_public, toxic=None, window_bits=13, nthreads=0):
    """the same over the host twins (no GPU, no context; r1cs may have been created without one) -> (pk, vk) with the point
    arrays as uint64 `*_words` arrays (A / B1 / B2 compacted, with infinity_a / infinity_b)"""
    toxic = tuple(int(x) for x in toxic) if toxic is not None else random_toxic()
    npub, nw = int(n_public), r1cs.n_wires
    a_t, b_t, k, z = setup_scalars_host(r1cs, npub, toxic, nthreads=nthreads)
    tau, alpha, beta, gamma, delta = toxic
    s1, s2 = FB.scalar_words([v % R for v in (alpha, beta, delta)]), FB.scalar_words([v % R for v in (beta, gamma, delta)])
    sa, sb = np.concatenate([a_t, s1]), np.concatenate([b_t, s2])
    scalars = [a_t, b_t, k, z, s1, s2, sa, sb]
    try:
        with FB.FixedBase(None, FB.G1, window_bits=window_bits) as g1, FB.FixedBase(None, FB.G2, window_bits=window_bits) as g2:
            A = g1.mul_host(sa, nthreads)[0]
            B1 = g1.mul_host(b_t, nthreads)[0]
            K = g1.mul_host(k, nthreads)[0]
            Z = g1.mul_host(z, nthreads)[0]
            B2 = g2.mul_host(sb, nthreads)[0]
        inf_a, inf_b = ~a_t.any(axis=1), ~b_t.any(axis=1)
    finally:
        for s in scalars:
            s.fill(0)
    words = {"alpha1": A[nw], "beta1": A[nw + 1], "delta1": A[nw + 2], "beta2": B2[nw], "gamma2": B2[nw + 1], "delta2": B2[nw + 2],
             "K_vk": K[:npub + 1]}
    pk = {"n": domain_size(r1cs.n_constraints), "n_public": npub, "A_words": A[:nw][~inf_a], "B1_words": B1[~inf_b],
          "B2_words": B2[:nw][~inf_b], "K_words": K[npub + 1:], "Z_words": Z, "infinity_a": inf_a, "infinity_b": inf_b}
    for name in ("alpha1", "beta1", "delta1", "beta2", "delta2"):
        pk[name + "_words"] = words[name].copy()
    return pk, _vk(words)
