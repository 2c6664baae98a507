"""Groth16 over BN254 as gnark v0.9.1 runs it (backend/groth16/bn254/{setup,prove,verify}.go -- un-vendored: gnark-plonky2-verifier/
go.mod:8; called at cmd/compile.go:40, cmd/web-api.go:77,84).  TEST INFRASTRUCTURE: pure Python on oracle/bn254*.py; only tests/,
smoke() and bench.py's checker role may import it.

What pins it: the verification equation is Verifier.sol's (contracts/hardhat/contracts/Verifier.sol:503-548:
e(A, B) e(C, -delta) e(alpha, -beta) e(L_pub, -gamma) = 1), which the reference's own proof satisfies under the reference's key
(tests/test_oracle_pairing.py); proofs made by `prove` below must satisfy it under keys made by `setup`.  The quotient step
(computeH: three inverse FFTs, three coset FFTs, (a b - c) / Z on the coset, one coset inverse FFT) is restated from gnark's prover;
the PROOF BYTES of the Go prover cannot be pinned (they are randomised by r, s and the reference ships no proving key):
**parity unpinned** beyond the verification equation.

R1CS: rows of {wire: coefficient}; wires = [1, public.., private..] (gnark's ordering).

`setup` = `key_scalars` (the discrete logarithms of the key's points) + one scalar multiplication per point.  With the toxic waste
known, a proof of a SATISFYING witness has a closed form in the exponent (`closed_form_proof`, `closed_form_vk`): field sums and
three scalar multiplications instead of transforms and multi-exponentiations -- the reference of the GPU prover's tests at domain
sizes where `setup` / `prove` themselves are out of reach (tests/test_gpu_groth16_sizes.py).
"""
from . import bn254 as B
from . import bn254_fr as FR

R = B.R


def domain_size(n_constraints):
    n = 1
    while n < max(2, n_constraints):
        n *= 2
    return n


def lagrange_at(tau, n):
    """L_j(tau) for the subgroup of size n: (tau^n - 1) w^j / (n (tau - w^j)); the n denominators share ONE inversion (Montgomery's
    trick: prefix products, invert the last, walk back)"""
    w = FR.root(n.bit_length() - 1)
    tau %= R
    z = (pow(tau, n, R) - 1) % R
    num, den, wj = [], [], 1
    for _ in range(n):
        num.append(z * wj % R)
        den.append(n * (tau - wj) % R)
        wj = wj * w % R
    if z == 0:                                      # tau is a point of the domain: L_j(tau) is 1 there and 0 elsewhere
        return [int(d == 0) for d in den]
    pre, acc = [], 1
    for d in den:
        pre.append(acc)
        acc = acc * d % R
    inv = pow(acc, R - 2, R)
    out = [0] * n
    for j in range(n - 1, -1, -1):
        out[j] = num[j] * inv % R * pre[j] % R
        inv = inv * den[j] % R
    return out


def key_scalars(r1cs, n_public, toxic):
    """the discrete logarithms of a key's points (the scalar stage of gnark's `Setup`): r1cs = (A, B, C) lists of sparse rows;
    toxic = (tau, alpha, beta, gamma, delta).  -> dict: n (domain size), n_wires, n_public; a_t, b_t, c_t [n_wires] = the columns of
    A, B, C evaluated at tau (a_t[i] = sum_j A_ji L_j(tau)); k_pk [n_wires - 1 - n_public] = (beta a_t + alpha b_t + c_t) / delta of the
    private wires; k_vk [1 + n_public] = the same over gamma for the constant and public wires; z [n - 1] = tau^i (tau^n - 1) / delta"""
    A, Bm, C = r1cs
    tau, alpha, beta, gamma, delta = [x % R for x in toxic]
    n_wires = 1 + max(max((max(row) if row else 0) for M in (A, Bm, C) for row in M), n_public)
    n = domain_size(len(A))
    L = lagrange_at(tau, n)
    a_t, b_t, c_t = [0] * n_wires, [0] * n_wires, [0] * n_wires
    for M, acc in ((A, a_t), (Bm, b_t), (C, c_t)):
        for j, row in enumerate(M):
            for w, coef in row.items():
                acc[w] = (acc[w] + coef * L[j]) % R
    dinv, ginv = pow(delta, R - 2, R), pow(gamma, R - 2, R)
    k = [(beta * a_t[i] + alpha * b_t[i] + c_t[i]) % R for i in range(n_wires)]
    zt = (pow(tau, n, R) - 1) % R * dinv % R
    z, ti = [], 1
    for _ in range(n - 1):
        z.append(ti * zt % R)
        ti = ti * tau % R
    return {"n": n, "n_wires": n_wires, "n_public": n_public, "a_t": a_t, "b_t": b_t, "c_t": c_t,
            "k_pk": [k[i] * dinv % R for i in range(1 + n_public, n_wires)], "k_vk": [k[i] * ginv % R for i in range(1 + n_public)], "z": z}


def _g1(s):
    return B.mul(s % R, B.G1) if s % R else None


def _g2(s):
    return B.g2_mul(s % R, B.G2) if s % R else None


def setup(r1cs, n_public, toxic):
    """r1cs = (A, B, C) lists of sparse rows over n_wires wires; toxic = (tau, alpha, beta, gamma, delta).
    -> (pk, vk) with every point as an affine tuple (None = infinity): the point stage over `key_scalars`"""
    tau, alpha, beta, gamma, delta = [x % R for x in toxic]
    sc = key_scalars(r1cs, n_public, toxic)
    pk = {"n": sc["n"], "n_wires": sc["n_wires"], "n_public": n_public,
          "A": [_g1(x) for x in sc["a_t"]], "B1": [_g1(x) for x in sc["b_t"]], "B2": [_g2(x) for x in sc["b_t"]],
          "K": [_g1(x) for x in sc["k_pk"]], "Z": [_g1(x) for x in sc["z"]],
          "alpha1": _g1(alpha), "beta1": _g1(beta), "delta1": _g1(delta), "beta2": _g2(beta), "delta2": _g2(delta)}
    return pk, closed_form_vk(sc, toxic, n_public)


def closed_form_vk(scalars, toxic, n_public):
    """the verifying key from the scalars of `key_scalars`: 4 + n_public + 1 scalar multiplications of the generators"""
    tau, alpha, beta, gamma, delta = [x % R for x in toxic]
    assert len(scalars["k_vk"]) == 1 + n_public
    return {"alpha1": _g1(alpha), "beta2": _g2(beta), "gamma2": _g2(gamma), "delta2": _g2(delta), "K": [_g1(x) for x in scalars["k_vk"]]}


def closed_form_proof(scalars, toxic, n_public, witness, r, s):
    """The proof of `prove` in the exponent, for a witness that SATISFIES the system (with the toxic waste known, as in a test).
    With At = sum_i w_i a_t[i] and Bt, Ct likewise:
        Ar  = (alpha + At + r delta) G1            Bs = (beta + Bt + s delta) G2
        Krs = ((sum_private w_i (beta a_t[i] + alpha b_t[i] + c_t[i]) + At Bt - Ct) / delta + s ar + r bs - r s delta) G1
    where ar, bs are the two scalars above and At Bt - Ct = h(tau) Z(tau): deg h <= n - 2, so the n - 1 coefficients the prover
    sums over are all of h.  For a witness that violates a constraint A B - C is no multiple of Z and the prover's h is another
    polynomial: the words then DIFFER from `prove` (tests/test_oracle_groth16.py).  O(n_wires) field operations and three scalar
    multiplications: no transform, no multi-exponentiation, no key point.  -> the eight words in `proof_to_uint256x8` order"""
    tau, alpha, beta, gamma, delta = [x % R for x in toxic]
    a_t, b_t, c_t = scalars["a_t"], scalars["b_t"], scalars["c_t"]
    assert len(witness) == scalars["n_wires"] and n_public == scalars["n_public"] and witness[0] % R == 1
    at = sum(x * y for x, y in zip(witness, a_t)) % R
    bt = sum(x * y for x, y in zip(witness, b_t)) % R
    ct = sum(x * y for x, y in zip(witness, c_t)) % R
    ar = (alpha + at + r * delta) % R
    bs = (beta + bt + s * delta) % R
    kp = sum(witness[i] * (beta * a_t[i] + alpha * b_t[i] + c_t[i]) for i in range(1 + n_public, len(witness))) % R
    krs = ((kp + at * bt - ct) * pow(delta, R - 2, R) + s * ar + r * bs - r * s * delta) % R
    return proof_to_uint256x8((B.mul(ar, B.G1), B.g2_mul(bs, B.G2), B.mul(krs, B.G1)))


def abc_evaluations(r1cs, witness, n):
    out = []
    for M in r1cs:
        v = [sum(coef * witness[w] for w, coef in row.items()) % R for row in M]
        out.append(v + [0] * (n - len(v)))
    return out


def compute_h(a, b, c):
    """gnark `computeH`: coefficients of (A B - C) / Z, n - 1 of them used"""
    n = len(a)
    ca, cb, cc = FR.ntt(a, inverse=True), FR.ntt(b, inverse=True), FR.ntt(c, inverse=True)
    ea, eb, ec = FR.ntt(ca, coset=True), FR.ntt(cb, coset=True), FR.ntt(cc, coset=True)
    den = pow((pow(FR.GENERATOR, n, R) - 1) % R, R - 2, R)
    q = [(x * y - z) % R * den % R for x, y, z in zip(ea, eb, ec)]
    return FR.ntt(q, inverse=True, coset=True)


def _msm1(scalars, points):
    acc = None
    for s, p in zip(scalars, points):
        if p is not None and s % R:
            acc = B.add(acc, B.mul(s % R, p))
    return acc


def _msm2(scalars, points):
    acc = None
    for s, p in zip(scalars, points):
        if p is not None and s % R:
            acc = B.g2_add(acc, B.g2_mul(s % R, p))
    return acc


def prove(pk, r1cs, witness, r, s):
    """-> (Ar, Bs, Krs) affine; witness = values of all wires, witness[0] = 1"""
    n, npub = pk["n"], pk["n_public"]
    a, b, c = abc_evaluations(r1cs, witness, n)
    h = compute_h(a, b, c)
    ar = B.add(B.add(pk["alpha1"], _msm1(witness, pk["A"])), B.mul(r % R, pk["delta1"]))
    bs2 = B.g2_add(B.g2_add(pk["beta2"], _msm2(witness, pk["B2"])), B.g2_mul(s % R, pk["delta2"]))
    bs1 = B.add(B.add(pk["beta1"], _msm1(witness, pk["B1"])), B.mul(s % R, pk["delta1"]))
    krs = B.add(_msm1(witness[1 + npub:], pk["K"]), _msm1(h[:n - 1], pk["Z"]))
    krs = B.add(krs, B.mul(s % R, ar))
    krs = B.add(krs, B.mul(r % R, bs1))
    krs = B.add(krs, B.neg(B.mul(r * s % R, pk["delta1"])))
    return ar, bs2, krs


def verify(vk, proof, public_inputs):
    """through oracle.bn254_pairing.groth16_verify -- the function the reference's own proof / tampered vectors pin
    (Verifier.sol:503-548: e(A, B) e(C, -delta) e(alpha, -beta) e(L, -gamma) == 1)"""
    from . import bn254_pairing as PR
    v = {"alpha": vk["alpha1"], "beta_neg": B.g2_neg(vk["beta2"]), "gamma_neg": B.g2_neg(vk["gamma2"]),
         "delta_neg": B.g2_neg(vk["delta2"]), "ic": vk["K"]}
    return PR.groth16_verify(v, proof_to_uint256x8(proof), [x % R for x in public_inputs])


def proof_to_uint256x8(proof):
    """the order of gnark's WriteRawTo / Verifier.sol: A.x, A.y, B.x1, B.x0, B.y1, B.y0, C.x, C.y"""
    ar, bs, krs = proof
    (bx0, bx1), (by0, by1) = bs
    return [ar[0], ar[1], bx1, bx0, by1, by0, krs[0], krs[1]]


def square_chain_r1cs(n_constraints, n_public=2):
    """a small satisfiable system for the tests: wires [1, p1..p_np, x0, x1, ...]; constraint j: x_j * x_j = x_{j+1} - p_(j mod np) - 3
    i.e. x_{j+1} = x_j^2 + p + 3.  Returns (r1cs, witness_fn(publics, x0))"""
    base = 1 + n_public
    A, Bm, C = [], [], []
    for j in range(n_constraints):
        A.append({base + j: 1})
        Bm.append({base + j: 1})
        C.append({base + j + 1: 1, 1 + (j % n_public): R - 1, 0: R - 3})

    def witness(publics, x0):
        w = [1] + [p % R for p in publics] + [x0 % R]
        for j in range(n_constraints):
            w.append((w[base + j] ** 2 + publics[j % n_public] + 3) % R)
        return w
    return (A, Bm, C), witness


BIT_COUNTS = (3, 16, 100, 8, 64, 65, 5, 33)


def bit_recomposition_r1cs(n_constraints, n_public=2, bit_counts=BIT_COUNTS, chain_steps=4):
    """a satisfiable system shaped like a real Groth16 witness (mostly bits): wires [1, p1..p_np, x0, ...]; group g with
    k = bit_counts[g mod len] bits adds the wires b_0..b_(k-1), v, u and `chain_steps` chain values, and the rows
        b_i * b_i = b_i                              (k booleanity rows, one term each)
        (sum_i 2^i b_i) * 1 = v - p                  (one recomposition row of k terms: coefficient +1, then general ones; -1 on p)
        v * v = u                                    (u occurs in no A or B column: its A / B1 / B2 key points are at infinity)
        x * x = x' - p - 3                           (chain_steps steps of the square chain, one chain through all groups)
    with p = the public wire 1 + (g mod n_public).  Groups are added while they fit; the rows left over are chain steps.
    Returns (r1cs, witness_fn(publics, x0, seed), layout) -- layout: the wire indices by kind ("bits", "v", "u", "chain")."""
    import random
    A, Bm, C = [], [], []
    x_cur = 1 + n_public
    next_wire = x_cur + 1
    layout = {"bits": [], "v": [], "u": [], "chain": [x_cur]}
    plan = []                       # how the witness is computed, in wire order

    def chain_step(pw):
        nonlocal x_cur, next_wire
        A.append({x_cur: 1})
        Bm.append({x_cur: 1})
        C.append({next_wire: 1, pw: R - 1, 0: R - 3})
        plan.append(("chain", x_cur, next_wire, pw))
        layout["chain"].append(next_wire)
        x_cur, next_wire = next_wire, next_wire + 1
    g = 0
    while True:
        k = bit_counts[g % len(bit_counts)]
        if len(A) + k + 2 + chain_steps > n_constraints:
            break
        pw = 1 + (g % n_public)
        bits = list(range(next_wire, next_wire + k))
        v, u = next_wire + k, next_wire + k + 1
        next_wire += k + 2
        for b in bits:
            A.append({b: 1})
            Bm.append({b: 1})
            C.append({b: 1})
        A.append({b: 1 << i for i, b in enumerate(bits)})
        Bm.append({0: 1})
        C.append({v: 1, pw: R - 1})
        A.append({v: 1})
        Bm.append({v: 1})
        C.append({u: 1})
        plan.append(("group", bits, v, u, pw))
        layout["bits"] += bits
        layout["v"].append(v)
        layout["u"].append(u)
        for _ in range(chain_steps):
            chain_step(pw)
        g += 1
    j = 0
    while len(A) < n_constraints:
        chain_step(1 + (j % n_public))
        j += 1
    n_wires = next_wire

    def witness(publics, x0, seed=0):
        rng = random.Random(seed)
        w = [0] * n_wires
        w[0] = 1
        w[1:1 + n_public] = [p % R for p in publics]
        w[1 + n_public] = x0 % R
        for step in plan:
            if step[0] == "chain":
                _, src, dst, pw = step
                w[dst] = (w[src] * w[src] + w[pw] + 3) % R
            else:
                _, bits, v, u, pw = step
                acc = 0
                for i, b in enumerate(bits):
                    w[b] = rng.randrange(2)
                    acc += w[b] << i
                w[v] = (acc + w[pw]) % R
                w[u] = w[v] * w[v] % R
        return w
    return (A, Bm, C), witness, layout
