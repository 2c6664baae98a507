"""plonky2 prover restatement (pure Python, small circuits only).  TEST INFRASTRUCTURE.

The prover lives in the un-vendored fork wormhole-foundation/plonky2-near @ 2244a9d (Cargo.toml:44-47), reached from
`data.prove(pw)` at near_bft_finality/src/prove_crypto/ed25519.rs:60,100 and recursion.rs:95.  Its source is not in
the reference tree, so this restates the published algorithm (plonky2 `plonk/prover.rs`, `plonk/vanishing_poly.rs`,
`fri/oracle.rs`, `fri/prover.rs`) and is anchored on what the tree DOES pin: every proof produced here must be accepted
by oracle/plonky2_verifier.py, which restates the reference's in-tree Go verifier line by line and accepts all four
golden proofs.  PARITY OF PROOF BYTES against the Rust prover is UNPINNED (the golden proofs ship without their
witnesses) -- the deterministic choices made here are: lowest valid proof-of-work witness (the fork uses
rayon `find_any`), sigma = next wire of the copy class in (column, row) order.

Order of operations (plonk/prover.rs `prove_with_partition_witness`):
  wires commit -> betas, gammas -> Z / partial products commit -> alphas -> quotient chunks commit -> zeta ->
  openings -> FRI (alpha, batched quotient, fold by arity with betas, final polynomial, PoW, query rounds).
"""
from . import goldilocks as gl
from . import plonky2_gates as G
from . import plonky2_verifier as V
from . import poseidon_gl as pgl

P = gl.P
pgl.use_c_port()


def bitrev_list(v):
    bits = (len(v) - 1).bit_length()
    return [v[gl.bitrev(i, bits)] for i in range(len(v))]


def ext_ntt(vals, inverse=False):
    a = gl.ntt([v[0] for v in vals], inverse)
    b = gl.ntt([v[1] for v in vals], inverse)
    return list(zip(a, b))


def ext_coset_fft(coeffs, shift):
    s, out = 1, []
    for c in coeffs:
        out.append((c[0] * s % P, c[1] * s % P))
        s = s * shift % P
    return ext_ntt(out)


class Tree:
    def __init__(self, H, leaves, cap_height):
        self.H, self.leaves = H, leaves
        layer = [H.hash_or_noop(l) for l in leaves]
        self.layers = []
        while len(layer) > (1 << cap_height):
            self.layers.append(layer)
            layer = [H.two_to_one(layer[2 * i], layer[2 * i + 1]) for i in range(len(layer) // 2)]
        self.cap = layer

    def prove(self, index):
        sib = []
        for layer in self.layers:
            sib.append(layer[index ^ 1])
            index >>= 1
        return sib


class Batch:
    """PolynomialBatch: coefficients, LDE values on g*<w_N> and the Merkle tree over bit-reversed rows"""

    def __init__(self, H, coeffs, rate_bits, cap_height, leaf_hook=None):
        self.coeffs = coeffs
        self.lde = [gl.coset_lde(c, rate_bits) for c in coeffs]      # natural order
        N = len(self.lde[0])
        bits = N.bit_length() - 1
        self.leaves = [[p[gl.bitrev(i, bits)] for p in self.lde] for i in range(N)]
        if leaf_hook is not None:        # a dishonest prover: the committed leaves differ from the LDE of the coefficients
            self.leaves = leaf_hook(self.leaves) or self.leaves
        self.tree = Tree(H, self.leaves, cap_height)

    @classmethod
    def from_values(cls, H, values, rate_bits, cap_height, leaf_hook=None):
        return cls(H, [gl.ntt(v, inverse=True) for v in values], rate_bits, cap_height, leaf_hook)


def eval_poly_ext(coeffs, x):
    r = (0, 0)
    for c in reversed(coeffs):
        r = gl.ext_add(gl.ext_mul(r, x), (c, 0))
    return r


def preprocess(common, constants, sigmas, H):
    """constants_sigmas commitment + circuit digest (plonky2 circuit_builder.rs `build`: digest =
    hash_no_pad(cap elements || hash_pad(domain separator = []) || degree_bits))"""
    fc = common["fri_params"]["config"]
    batch = Batch.from_values(H, [list(map(int, c)) for c in constants] + [list(map(int, s)) for s in sigmas], fc["rate_bits"],
                              fc["cap_height"])
    parts = []
    for h in batch.tree.cap:
        parts += H.to_vec(h)
    parts += H.to_vec(V.hash_pad(H, []))      # domain separator = [] (pad10*1 to the sponge rate)
    parts.append(common["fri_params"]["degree_bits"])
    digest = H.hash_no_pad(parts)
    return batch, digest


def prove(common, constants, sigmas, wires, public_inputs, H=V.HasherGL, cs_batch=None, digest=None, trace=None, hooks=None):
    """hooks: None (the honest prover), or a dict of callables that make a DISHONEST prover for the verifier's tests.  Each one
    changes a value before it is committed or observed, so the Merkle paths, the transcript and the proof of work of the
    resulting proof are honest for the changed data:
      "leaves"(name, leaves)      name in "wires" / "zs_pp" / "quotient"; leaves[x_index][column] as committed (bit-reversed row
                                  order).  The coefficients, and so the openings and every later layer, stay honest.
      "fri_layer"(i, cosets)      cosets[coset index][position] = (a, b): the values of FRI layer i before its tree is built
      "final_poly"(coeffs)        the final polynomial before it is observed
      "pow_witness"(candidates)   candidates yields (witness, query indices that follow from it) for every valid witness in
                                  increasing order; returns the witness to use
    The first three change their argument in place or return a replacement."""
    hk = hooks or {}
    leaf_hook = lambda name: (lambda leaves: hk["leaves"](name, leaves)) if "leaves" in hk else None
    cfg, fp = common["config"], common["fri_params"]
    fc = fp["config"]
    rate_bits, cap_h = fc["rate_bits"], fc["cap_height"]
    degree_bits = fp["degree_bits"]
    n = 1 << degree_bits
    N = n << rate_bits
    lde_bits = degree_bits + rate_bits
    nch, routed = cfg["num_challenges"], cfg["num_routed_wires"]
    npp, qdf = common["num_partial_products"], common["quotient_degree_factor"]
    assert qdf == 1 << rate_bits
    gates = [G.gate_from_id(g) for g in common["gates"]]
    if cs_batch is None:
        cs_batch, digest = preprocess(common, constants, sigmas, H)
    wires = [list(map(int, w)) for w in wires]
    sig_vals = [list(map(int, s)) for s in sigmas]
    pih = pgl.hash_no_pad(public_inputs)
    tr = trace if trace is not None else {}

    ch = V.Challenger(H)
    ch.observe_hash(digest)
    ch.observe_many(pih)
    wires_b = Batch.from_values(H, wires, rate_bits, cap_h, leaf_hook("wires"))
    ch.observe_cap(wires_b.tree.cap)
    betas, gammas = ch.challenges(nch), ch.challenges(nch)
    tr["betas"], tr["gammas"] = betas, gammas

    # ---- Z and partial products (prover.rs `wires_permutation_partial_products_and_zs`)
    w_n = gl.root_of_unity(degree_bits)
    sub = [pow(w_n, i, P) for i in range(n)]
    k_is = common["k_is"]
    zs, pps = [], []
    for c in range(nch):
        b, g = betas[c], gammas[c]
        z = [0] * n
        pp = [[0] * n for _ in range(npp)]
        zx = 1
        for i in range(n):
            acc = zx
            z[i] = zx
            for k in range(npp + 1):
                for j in range(k * qdf, min((k + 1) * qdf, routed)):
                    num = (wires[j][i] + b * k_is[j] % P * sub[i] + g) % P
                    den = (wires[j][i] + b * sig_vals[j][i] + g) % P
                    acc = acc * num % P * gl.inv(den) % P
                if k < npp:
                    pp[k][i] = acc
            zx = acc
        assert zx == 1, "copy constraints are not satisfied by the witness (Z does not close)"
        zs.append(z)
        pps.append(pp)
    zs_pp_b = Batch.from_values(H, zs + [p for pp in pps for p in pp], rate_bits, cap_h, leaf_hook("zs_pp"))
    ch.observe_cap(zs_pp_b.tree.cap)
    alphas = ch.challenges(nch)
    tr["alphas"] = alphas

    # ---- quotient (prover.rs `compute_quotient_polys`, vanishing_poly.rs `eval_vanishing_poly_base_batch`)
    K = G.BaseK
    w_N = gl.root_of_unity(lde_bits)
    quotient_vals = [[0] * N for _ in range(nch)]
    n_inv = gl.inv(n)
    nc = common["num_constants"]
    for i in range(N):
        x = gl.GENERATOR * pow(w_N, i, P) % P
        zh = (pow(x, n, P) - 1) % P
        l0 = zh * gl.inv((x - 1) * n % P) % P
        i_next = (i + (1 << rate_bits)) % N
        cs = [p[i] for p in cs_batch.lde]
        wv = [p[i] for p in wires_b.lde]
        zp = [p[i] for p in zs_pp_b.lde]
        zn = [zs_pp_b.lde[c][i_next] for c in range(nch)]
        terms = G.vanishing_terms(K, common, gates, x, l0, cs[:nc], cs[nc:], wv, zp[:nch], zn, zp[nch:], betas, gammas, pih)
        zh_inv = gl.inv(zh)
        for c in range(nch):
            quotient_vals[c][i] = G.reduce_with_powers(K, terms, alphas[c]) * zh_inv % P
    chunks = []
    for c in range(nch):
        # coset_ifft: values on g*<w_N> -> coefficients
        co = gl.ntt(quotient_vals[c], inverse=True)
        gi, s = gl.inv(gl.GENERATOR), 1
        for j in range(N):
            co[j] = co[j] * s % P
            s = s * gi % P
        assert all(v == 0 for v in co[qdf * n:])
        for k in range(qdf):
            chunks.append(co[k * n:(k + 1) * n])
    quot_b = Batch(H, chunks, rate_bits, cap_h, leaf_hook("quotient"))
    ch.observe_cap(quot_b.tree.cap)
    zeta = ch.ext_challenge()
    tr["zeta"] = zeta

    # ---- openings (proof.rs `OpeningSet::new`)
    g_zeta = gl.ext_mul((w_n, 0), zeta)
    ev = lambda batch, x: [eval_poly_ext(c, x) for c in batch.coeffs]
    cs_e, w_e, zp_e, q_e = ev(cs_batch, zeta), ev(wires_b, zeta), ev(zs_pp_b, zeta), ev(quot_b, zeta)
    zn_e = [eval_poly_ext(c, g_zeta) for c in zs_pp_b.coeffs[:nch]]
    openings = {"constants": cs_e[:nc], "plonk_sigmas": cs_e[nc:], "wires": w_e, "plonk_zs": zp_e[:nch], "plonk_zs_next": zn_e,
                "partial_products": zp_e[nch:], "quotient_polys": q_e, "lookup_zs": [], "lookup_zs_next": []}
    batch0 = cs_e + w_e + zp_e + q_e
    batch1 = zn_e
    for x in batch0 + batch1:
        ch.observe_ext(x)

    # ---- FRI (fri/oracle.rs `prove_openings`, fri/prover.rs)
    alpha = ch.ext_challenge()
    tr["fri_alpha"] = alpha
    batches = [cs_batch, wires_b, zs_pp_b, quot_b]
    all_polys = [c for b_ in batches for c in b_.coeffs]
    final = [(0, 0)] * n
    for polys, point, opened in ((all_polys, zeta, batch0), (zs_pp_b.coeffs[:nch], g_zeta, batch1)):
        comp = [(0, 0)] * n
        for p in reversed(polys):            # sum_i alpha^i p_i
            comp = [gl.ext_add(gl.ext_mul(c, alpha), (pc, 0)) for c, pc in zip(comp, p)]
        # divide_by_linear: q = (comp - comp(point)) / (X - point)
        q = [(0, 0)] * n
        carry = (0, 0)
        for j in reversed(range(n)):
            cur = gl.ext_add(comp[j], gl.ext_mul(carry, point))
            if j:
                q[j - 1] = cur
            carry = cur
        assert carry == V.reduce_with_powers(opened, alpha), "opening mismatch"
        scale = V.ext_pow(alpha, len(polys))
        final = [gl.ext_add(gl.ext_mul(f, scale), qq) for f, qq in zip(final, q)]
    coeffs = final + [(0, 0)] * (N - n)
    values = ext_coset_fft(coeffs, gl.GENERATOR)
    shift = gl.GENERATOR
    trees, fri_betas = [], []
    tr["fri_betas"] = fri_betas          # grows with the layers: a "fri_layer" hook of layer i sees the betas of the layers before
    for arity_bits in fp["reduction_arity_bits"]:
        arity = 1 << arity_bits
        rv = bitrev_list(values)
        chunked = [rv[k:k + arity] for k in range(0, len(rv), arity)]
        if "fri_layer" in hk:
            chunked = hk["fri_layer"](len(trees), chunked) or chunked
        leaves = [[c for e in coset for c in e] for coset in chunked]
        t = Tree(H, leaves, cap_h)
        ch.observe_cap(t.cap)
        trees.append((t, chunked))
        beta = ch.ext_challenge()
        fri_betas.append(beta)
        coeffs = [V.reduce_with_powers(coeffs[k:k + arity], beta) for k in range(0, len(coeffs), arity)]
        shift = pow(shift, arity, P)
        values = ext_coset_fft(coeffs, shift)
    assert all(c == (0, 0) for c in coeffs[len(coeffs) >> rate_bits:])
    final_poly = coeffs[:len(coeffs) >> rate_bits]
    if "final_poly" in hk:
        final_poly = hk["final_poly"](final_poly) or final_poly
    for c in final_poly:
        ch.observe_ext(c)
    # proof of work: lowest witness whose response has pow_bits leading zeros
    pow_bits = fc["proof_of_work_bits"]
    base_state, base_inp = list(ch.state), list(ch.inp)

    def valid_witnesses():
        witness = 0
        while True:
            st = list(base_state)
            inp = base_inp + [witness]
            for i, e in enumerate(inp):
                st[i] = e
            st = pgl._perm(st)
            if st[7] < (1 << (64 - pow_bits)):
                yield witness
            witness += 1

    def query_indices(witness):
        c2 = V.Challenger(H)
        c2.state, c2.inp, c2.out = list(ch.state), list(ch.inp), list(ch.out)
        c2.observe(witness)
        c2.challenge()
        return [c2.challenge() % N for _ in range(fc["num_query_rounds"])]
    if "pow_witness" in hk:
        witness = hk["pow_witness"]((w, query_indices(w)) for w in valid_witnesses())
    else:
        witness = next(valid_witnesses())
    ch.observe(witness)
    resp = ch.challenge()
    assert resp < (1 << (64 - pow_bits))
    rounds = []
    for _ in range(fc["num_query_rounds"]):
        x_index = ch.challenge() % N
        init = []
        for b_ in batches:
            init.append([b_.leaves[x_index], {"siblings": [H.dump(s) for s in b_.tree.prove(x_index)]}])
        steps = []
        idx = x_index
        for (t, chunked), arity_bits in zip(trees, fp["reduction_arity_bits"]):
            idx >>= arity_bits
            steps.append({"evals": [list(e) for e in chunked[idx]], "merkle_proof": {"siblings": [H.dump(s) for s in t.prove(idx)]}})
        rounds.append({"initial_trees_proof": {"evals_proofs": init}, "steps": steps})
    dump_cap = lambda cap: [H.dump(h) for h in cap]
    proof = {
        "proof": {
            "wires_cap": dump_cap(wires_b.tree.cap),
            "plonk_zs_partial_products_cap": dump_cap(zs_pp_b.tree.cap),
            "quotient_polys_cap": dump_cap(quot_b.tree.cap),
            "openings": {k: [list(e) for e in v] for k, v in openings.items()},
            "opening_proof": {
                "commit_phase_merkle_caps": [dump_cap(t.cap) for t, _ in trees],
                "query_round_proofs": rounds,
                "final_poly": {"coeffs": [list(c) for c in final_poly]},
                "pow_witness": witness,
            },
        },
        "public_inputs": [int(x) for x in public_inputs],
    }
    verifier_data = {"constants_sigmas_cap": dump_cap(cs_batch.tree.cap), "circuit_digest": H.dump(digest)}
    return proof, verifier_data
