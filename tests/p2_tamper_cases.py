"""Rejected plonky2 proofs for the native verifier (tests/test_p2_tamper_host.py, tests/test_gpu_p2_tamper.py), two families.

A. The field sweep.  proof_fields(common, hasher) names every field of a serialised proof -- Goldilocks elements, the 32-byte
Poseidon-BN128 digests, the u8 sibling counts, the public-input count, the proof-of-work witness -- and sweep(circuit) is one
tampered copy of the circuit's honest proof per field: an element becomes (v + 1) mod p and a digest (v + 1) mod r, so the copy is
still canonical and goes through the query phase; a count gets its low bit flipped.  noncanonical(circuit) holds a few copies
with an element >= p or a digest >= r.  Small circuits are swept whole; the reference's golden wrap proof (28 rounds, 128 KB)
through the stratified selection of golden_selection().

B. Dishonest-prover proofs.  forgeries(name) runs the oracle's prover restatement with hooks (oracle/plonky2_prover.py) that
change a value BEFORE it is committed or observed: every Merkle path, the transcript and the proof of work are honest for the
changed data, so only the checks of the FRI fold chain (initial combination, per-step consistency, interpolation, final
polynomial) can reject the proof.  The "sole_check" ones go further: one query round, and every layer after the changed
value follows from it, so that ONE comparison of ONE extension component is all that fails.

Everything is computed once per process."""
import collections
import copy
import random

from oracle import goldilocks as gl, plonky2_prover as OP, plonky2_verifier as V
from oracle.poseidon_bn254 import R
from zklc_amd.plonky2 import serialization as S, HASH_GL, HASH_BN128
from zklc_amd.plonky2.verifier import PROOF_OK, PROOF_BAD_FORMAT, PROOF_BAD_FRI
import p2_matrix_cases as M
from test_plonky2_verifier_host import golden, oracle_status

P = 2**64 - 2**32 + 1
Circuit = collections.namedtuple("Circuit", "name common vd hasher raw")
Field = collections.namedtuple("Field", "offset size kind label")     # kind: "gl", "digest", "count8", "count64"

# the circuits of the sweep: the C prover's proof of each
SWEEP_CASES = [M.BY_NAME["rounds-3"], M.BY_NAME["combined-2^9"],
               M._case("tamper-tiny-2^2", "tiny", 2, rounds=2),                       # no reduction
               M._case("tamper-six-steps", "recursion", 7, arity=(1, 0), rounds=2)]   # trees 4..9, 4-element step leaves
BN128_CASE = M._case("tamper-bn128", "tiny", 3, arity=(1, 0), rounds=3, pow=3)         # the Python prover restatement
SWEEP_NAMES = [c.name for c in SWEEP_CASES] + [BN128_CASE.name]
# the circuits of the forgeries: name -> (case, the arity list it must have)
FORGE_CASES = {
    "f-1-1": (M._case("forge-1-1", "tiny", 3, arity=(1, 0), rounds=4, pow=3), [1, 1]),
    "f-2-2": (M._case("forge-2-2", "tiny", 5, arity=(2, 0), rounds=4, pow=3), [2, 2]),
    "f-3": (M._case("forge-3", "tiny", 4, arity=(3, 0), rounds=4, pow=3), [3]),
    "f-4": (M._case("forge-4", "tiny", 5, arity=(4, 0), rounds=4, pow=3), [4]),
    "f-none": (M._case("forge-none", "tiny", 3, rounds=4, pow=3), []),
    "f-28": (M._case("forge-28", "tiny", 3, arity=(1, 0), rounds=28, pow=3), [1, 1]),
    "f-one": (M._case("forge-one", "tiny", 3, arity=(1, 0), rounds=1, pow=3), [1, 1]),
    "f-bn128": (BN128_CASE, [1, 1]),
}
_BY_NAME = {c.name: c for c in SWEEP_CASES + [BN128_CASE]}
_CIRCUIT, _FIELDS, _SWEEP, _FORGERIES = {}, {}, {}, {}


def hasher_of(case):
    return HASH_BN128 if case.name == BN128_CASE.name else HASH_GL


def honest(case):
    """-> Circuit with the honest proof: the C prover's under Poseidon-Goldilocks, the Python restatement's under Poseidon-BN128"""
    if case.name not in _CIRCUIT:
        data, wires, pis = M.make(case)
        common = data.common_data()
        if hasher_of(case) == HASH_GL:
            raw, vd = M.reference(case)
        else:
            pj, vd = OP.prove(common, data.constants, data.sigmas, wires, pis, V.HasherBN128)
            raw = S.proof_to_bytes(pj, common, HASH_BN128)
        _CIRCUIT[case.name] = Circuit(case.name, common, vd, hasher_of(case), raw)
    return _CIRCUIT[case.name]


def circuit(name):
    if name == "golden":
        if name not in _CIRCUIT:
            c = golden()[0]
            _CIRCUIT[name] = Circuit(name, c["common_data"], c["verifier_data"], HASH_BN128,
                                     S.proof_to_bytes(c["proof"], c["common_data"], HASH_BN128))
        return _CIRCUIT[name]
    return honest(_BY_NAME[name] if name in _BY_NAME else FORGE_CASES[name][0])


# ------------------------------------------------------------------------------------------------------------- field map
def proof_fields(common, hasher):
    """every field of a serialised proof of the circuit, in byte order: [Field(offset, size, kind, label)].  Labels:
    ("cap", k, i, e) k = 0 wires / 1 zs, partial products / 2 quotient      ("commit_cap", step, i, e)
    ("opening", name, i, component)                                         ("final", i, component)
    ("leaf", round, tree, i)    ("count", round, tree)    ("sibling", round, tree, level, e)      tree 4 + step: a reduction
    ("eval", round, step, position, component)             ("pow",)    ("npi",)    ("pi", i)
    e is the word of a Poseidon-Goldilocks digest (4 fields of kind "gl") and None for a Poseidon-BN128 one (kind "digest")."""
    sh = S.shapes(common)
    out, o = [], [0]

    def put(size, kind, *label):
        out.append(Field(o[0], size, kind, label))
        o[0] += size

    def digest(*label):
        if hasher == HASH_GL:
            for e in range(4):
                put(8, "gl", *(label + (e,)))
        else:
            put(32, "digest", *(label + (None,)))
    for k in range(3):
        for i in range(sh["cap"]):
            digest("cap", k, i)
    for name, n in sh["openings"]:
        for i in range(n):
            for c in range(2):
                put(8, "gl", "opening", name, i, c)
    for s in range(len(sh["arity_bits"])):
        for i in range(sh["cap"]):
            digest("commit_cap", s, i)
    depth0 = sh["lde_bits"] - sh["cap_height"]
    for r in range(sh["rounds"]):
        for t, w in enumerate(sh["leaf_widths"]):
            for i in range(w):
                put(8, "gl", "leaf", r, t, i)
            put(1, "count8", "count", r, t)
            for d in range(depth0):
                digest("sibling", r, t, d)
        bits = sh["lde_bits"]
        for s, a in enumerate(sh["arity_bits"]):
            bits -= a
            for pos in range(1 << a):
                for c in range(2):
                    put(8, "gl", "eval", r, s, pos, c)
            put(1, "count8", "count", r, 4 + s)
            for d in range(max(bits - sh["cap_height"], 0)):
                digest("sibling", r, 4 + s, d)
    for i in range(sh["final_len"]):
        for c in range(2):
            put(8, "gl", "final", i, c)
    put(8, "gl", "pow")
    put(8, "count64", "npi")
    for i in range(common["num_public_inputs"]):
        put(8, "gl", "pi", i)
    return out


def fields(name):
    if name not in _FIELDS:
        c = circuit(name)
        _FIELDS[name] = proof_fields(c.common, c.hasher)
    return _FIELDS[name]


def region(f):
    """what a field belongs to, for stratified samples: (label kind, tree or step or cap where there is one, round)"""
    lb = f.label
    if lb[0] in ("leaf", "count", "sibling"):
        return (lb[0], lb[2], lb[1])
    if lb[0] == "eval":
        return ("eval", lb[2], lb[1])
    if lb[0] in ("cap", "commit_cap"):
        return (lb[0], lb[1], None)
    if lb[0] == "opening":
        return ("opening", lb[1], None)
    return (lb[0], None, None)


def value(raw, f):
    return int.from_bytes(raw[f.offset:f.offset + f.size], "little")


def patched(raw, f, v):
    return raw[:f.offset] + int(v).to_bytes(f.size, "little") + raw[f.offset + f.size:]


def tampered_value(raw, f):
    """the changed value of the sweep: still canonical where the field is an element or a digest"""
    v = value(raw, f)
    if f.kind == "gl":
        return (v + 1) % P
    if f.kind == "digest":
        return (v + 1) % R
    return v ^ 1


def noncanonical_value(raw, f):
    v = value(raw, f)
    if f.kind == "gl":
        return v + P if v + P < 2**64 else P
    assert f.kind == "digest"
    return v + R           # r < 2^254: always fits in 32 bytes


def json_with(pj, f, v):
    """the proof.json `pj` with field `f` set to `v` -- the JSON-level form of patched() (count fields have none: a JSON
    proof's counts are the lengths of its lists)"""
    j = copy.deepcopy(pj)
    pr, lb = j["proof"], f.label
    op = pr["opening_proof"]

    def set_digest(lst, i, e):
        if e is None:
            lst[i] = str(v)
        else:
            lst[i]["elements"][e] = v
    if lb[0] == "cap":
        set_digest(pr[("wires_cap", "plonk_zs_partial_products_cap", "quotient_polys_cap")[lb[1]]], lb[2], lb[3])
    elif lb[0] == "commit_cap":
        set_digest(op["commit_phase_merkle_caps"][lb[1]], lb[2], lb[3])
    elif lb[0] == "opening":
        pr["openings"][lb[1]][lb[2]][lb[3]] = v
    elif lb[0] == "leaf":
        op["query_round_proofs"][lb[1]]["initial_trees_proof"]["evals_proofs"][lb[2]][0][lb[3]] = v
    elif lb[0] == "sibling":
        q = op["query_round_proofs"][lb[1]]
        m = q["initial_trees_proof"]["evals_proofs"][lb[2]][1] if lb[2] < 4 else q["steps"][lb[2] - 4]["merkle_proof"]
        set_digest(m["siblings"], lb[3], lb[4])
    elif lb[0] == "eval":
        op["query_round_proofs"][lb[1]]["steps"][lb[2]]["evals"][lb[3]][lb[4]] = v
    elif lb[0] == "final":
        op["final_poly"]["coeffs"][lb[1]][lb[2]] = v
    elif lb[0] == "pow":
        op["pow_witness"] = v
    elif lb[0] == "pi":
        j["public_inputs"][lb[1]] = v
    else:
        raise KeyError(lb)
    return j


def read_evals(name, rounds):
    """labels of the evaluations that the consistency checks of the honest proof's query rounds `rounds` read (both components)"""
    c = circuit(name)
    sh = S.shapes(c.common)
    qi = V.challenges(V.parse_proof(S.proof_from_bytes(c.raw, c.common, c.hasher), c.vd), c.common)["query_indices"]
    read = set()
    for r in rounds:
        x = qi[r] % (1 << sh["lde_bits"])
        for s, ab in enumerate(sh["arity_bits"]):
            read |= {("eval", r, s, x & ((1 << ab) - 1), comp) for comp in (0, 1)}
            x >>= ab
    return read


def sweep(name):
    """-> [(Field, bytes)]: one tampered copy of the circuit's honest proof per field (the golden proof: per selected field,
    and the siblings of golden_selection() a second time with the low bit of their top word flipped)"""
    if name not in _SWEEP:
        c = circuit(name)
        if name == "golden":
            _SWEEP[name] = golden_selection()
        else:
            _SWEEP[name] = [(f, patched(c.raw, f, tampered_value(c.raw, f))) for f in fields(name)]
    return _SWEEP[name]


def golden_selection():
    """the stratified selection over the golden wrap proof: for every round and every tree the first and last leaf element and
    the first and last 8 bytes of the first and last sibling; for every step the first and last evaluation and the one its
    consistency check reads, both components;
    every cap's first and last entry; every seventh opening; every final-polynomial coefficient; the proof-of-work witness;
    every public input; every count"""
    c = circuit("golden")
    sh = S.shapes(c.common)
    depth = {}
    for f in fields("golden"):
        if f.label[0] == "sibling":
            depth[f.label[2]] = max(depth.get(f.label[2], 0), f.label[3] + 1)
    out, n_open = [], 0
    read = read_evals("golden", range(sh["rounds"]))
    for f in fields("golden"):
        lb = f.label
        if lb[0] == "leaf":
            take = lb[3] in (0, sh["leaf_widths"][lb[2]] - 1)
        elif lb[0] == "sibling":
            take = lb[3] in (0, depth[lb[2]] - 1)
        elif lb[0] == "eval":
            take = lb[3] in (0, (1 << sh["arity_bits"][lb[2]]) - 1) or lb in read
        elif lb[0] in ("cap", "commit_cap"):
            take = lb[2] in (0, sh["cap"] - 1)
        elif lb[0] == "opening":
            take = (n_open // 2) % 7 == 0      # every seventh extension element, both components
            n_open += 1
        else:
            take = True
        if not take:
            continue
        out.append((f, patched(c.raw, f, tampered_value(c.raw, f))))     # a digest: its first 8 bytes change
        if lb[0] == "sibling":                                           # its last 8 bytes: bit 192 (may leave it >= r)
            out.append((f, patched(c.raw, f, value(c.raw, f) ^ (1 << 192))))
    return out


def is_canonical(f, raw):
    return f.kind not in ("gl", "digest") or value(raw, f) < (P if f.kind == "gl" else R)


def noncanonical(name):
    """-> [(Field, bytes)]: an element >= p / a digest >= r in one field of every region of the proof, first and last round"""
    c = circuit(name)
    last = S.shapes(c.common)["rounds"] - 1
    seen, out = set(), []
    for f in fields(name):
        rg = region(f)
        if f.kind in ("count8", "count64") or rg[2] not in (None, 0, last) or (rg, f.kind) in seen:
            continue
        seen.add((rg, f.kind))
        out.append((f, patched(c.raw, f, noncanonical_value(c.raw, f))))
    return out


def oracle_sample(name, at_least=150, seed=1):
    """indices into sweep(name): one field per region (kind of field, tree, first and last round), filled to `at_least`"""
    sw = sweep(name)
    last = S.shapes(circuit(name).common)["rounds"] - 1
    rng = random.Random(seed)
    by_region = collections.defaultdict(list)
    for i, (f, _) in enumerate(sw):
        rg = region(f)
        if rg[2] in (None, 0, last):
            by_region[(rg, f.kind)].append(i)
    picked = {rng.choice(v) for v in by_region.values()}
    # the evaluation each step's consistency check reads (the only byte-level change that ends at FRI), first and last round
    read = read_evals(name, (0, last))
    picked |= {i for i, (f, _) in enumerate(sw) if f.label in read}
    rest =[i for i in range(len(sw)) if i not in picked]
    rng.shuffle(rest)
    picked |= set(rest[:max(0, at_least - len(picked))])
    return sorted(picked)


def expected_status(c, f, raw):
    """the oracle's verdict on a tampered copy.  Two rules stand in for it where the restatement has no such input: a count that
    differs from the circuit's is a proof of another shape (FORMAT), and so is an element >= p or a digest >= r, which the
    restatement would reduce"""
    if f.kind in ("count8", "count64") or not is_canonical(f, raw):
        return PROOF_BAD_FORMAT
    return oracle_status(S.proof_from_bytes(raw, c.common, c.hasher), c.vd, c.common)


def device_batch(name, proofs, seed=7, honest_inside=5):
    """-> (batch, positions of the honest copies): `proofs` with the circuit's honest proof at position 0, at the last position
    and at seeded interior positions; the length is no multiple of 64"""
    c = circuit(name)
    rng = random.Random(seed)
    batch = list(proofs)
    for _ in range(honest_inside):
        batch.insert(rng.randrange(1, len(batch)), c.raw)
    batch = [c.raw] + batch + [c.raw]
    if len(batch) % 64 == 0:
        batch.append(c.raw)
    return batch, [i for i, b in enumerate(batch) if b is c.raw]


def chunks(batch, limit=64 << 20):
    """the batch in calls of at most `limit` proof bytes each"""
    per = max(1, limit // len(batch[0]))
    return [batch[i:i + per] for i in range(0, len(batch), per)]


# ------------------------------------------------------------------------------------------------------------- forgeries
Forgery = collections.namedtuple("Forgery", "kind label raw want")


def _bump(e, comp):
    e = list(e)
    e[comp] = (e[comp] + 1) % P
    return tuple(e)


def _nth_witness(pred, k=0, limit=200000):
    """pow_witness hook: the k-th valid witness whose query indices satisfy pred"""
    def hook(candidates):
        seen = 0
        for n, (w, idx) in enumerate(candidates):
            if pred(idx):
                if seen == k:
                    return w
                seen += 1
            assert n < limit, "no such proof-of-work witness"
    return hook


def _forge(name, hooks, trace=None):
    case = FORGE_CASES[name][0]
    data, wires, pis = M.make(case)
    c = circuit(name)
    H = V.HasherBN128 if c.hasher == HASH_BN128 else V.HasherGL
    pj, vd = OP.prove(c.common, data.constants, data.sigmas, wires, pis, H, trace=trace, hooks=hooks)
    assert vd == c.vd
    return S.proof_to_bytes(pj, c.common, c.hasher)


def _within(arity_bits, i):
    """query index -> its position in the coset of layer i"""
    lo = sum(arity_bits[:i])
    return lambda x: (x >> lo) & ((1 << arity_bits[i]) - 1)


def _layer_hook(layer, pos, comp, cosets=None):
    def hook(i, chunked):
        if i == layer:
            for k, coset in enumerate(chunked):
                if cosets is None or k in cosets:
                    for p in (range(len(coset)) if pos is None else [pos]):
                        coset[p] = _bump(coset[p], comp)
    return hook


def _column_hook(batch, col):
    def hook(name, leaves):
        if name == batch:
            for leaf in leaves:
                leaf[col] = (leaf[col] + 1) % P
    return hook


def _one_round_hooks(c, k, rng):
    """about a quarter of the cosets of layer 0 (1 / rounds of them when there are many rounds) changed in every position, and a
    witness whose queries meet a changed coset in round k and in no other round"""
    sh = S.shapes(c.common)
    n_cosets = 1 << (sh["lde_bits"] - sh["arity_bits"][0])
    changed = set(rng.sample(range(n_cosets), max(1, n_cosets // max(4, sh["rounds"]))))
    a0 = sh["arity_bits"][0]
    pred = lambda idx: [r for r, x in enumerate(idx) if (x >> a0) in changed] == [k]
    return {"fri_layer": _layer_hook(0, None, 0, changed), "pow_witness": _nth_witness(pred)}


def _sole_check_forgery(name, step, comp, target):
    """One query round, query index `target`: the evaluation that the consistency check of reduction `step` reads is changed in
    one component, and every later layer and the final polynomial are made to FOLLOW from the changed value (the fold of the
    changed coset at that layer's beta; the final polynomial's constant term moved by the difference).  One comparison of one
    component is then the only check of the whole proof that fails."""
    c = circuit(name)
    sh = S.shapes(c.common)
    arities, n_log = sh["arity_bits"], sh["lde_bits"]
    trace, pending = {}, []

    def fold():
        evals, x, within, i = pending.pop()
        return V.interpolate_coset(evals, x, within, arities[i], trace["fri_betas"][i])

    def layer(i, chunked):
        if i < step:
            return
        lo = sum(arities[:i])
        idx = target >> lo
        within, coset = idx & ((1 << arities[i]) - 1), idx >> arities[i]
        chunked[coset][within] = _bump(chunked[coset][within], comp) if i == step else fold()
        pending.append((list(chunked[coset]), pow(V.subgroup_x(target, n_log), 1 << lo, P), within, i))

    def final(coeffs):
        x = pow(V.subgroup_x(target, n_log), 1 << sum(arities), P)
        ev = (0, 0)
        for co in reversed(coeffs):
            ev = gl.ext_add(gl.ext_mul(ev, (x, 0)), co)
        return [gl.ext_add(coeffs[0], gl.ext_sub(fold(), ev))] + coeffs[1:]
    hooks = {"fri_layer": layer, "final_poly": final, "pow_witness": _nth_witness(lambda idx: idx == [target])}
    return _forge(name, hooks, trace)


def forgeries(name):
    """-> [Forgery(kind, label, proof bytes, expected status)] of one circuit of FORGE_CASES"""
    if name in _FORGERIES:
        return _FORGERIES[name]
    case, arities = FORGE_CASES[name]
    c = circuit(name)
    sh = S.shapes(c.common)
    assert sh["arity_bits"] == arities, (name, sh["arity_bits"])
    rng = random.Random(len(name) + 100 * sh["rounds"])
    out = []
    add = lambda kind, label, hooks, want=PROOF_BAD_FRI: out.append(Forgery(kind, label, _forge(name, hooks), want))
    nch = c.common["config"]["num_challenges"]
    w_zs, w_q = sh["leaf_widths"][2], sh["leaf_widths"][3]
    columns = [("wires", 0), ("wires", sh["leaf_widths"][1] - 1), ("zs_pp", 0), ("zs_pp", nch), ("zs_pp", w_zs - 1),
               ("quotient", 0), ("quotient", w_q - 1)]       # Z of challenge 0, the first and the last partial product
    if name == "f-one":
        for step in range(len(arities)):
            for comp in (0, 1):
                target = rng.randrange(1 << sh["lde_bits"])
                out.append(Forgery("sole_check", (step, comp), _sole_check_forgery(name, step, comp, target), PROOF_BAD_FRI))
    elif name == "f-28":
        for k in (0, 13, 27):
            add("one_round", k, _one_round_hooks(c, k, rng))
    elif name == "f-bn128":
        add("fri_layer", (1, "within"), {"fri_layer": _layer_hook(1, 1, 0),
                                         "pow_witness": _nth_witness(lambda idx: _within(arities, 1)(idx[0]) == 1)})
        add("initial", ("quotient", w_q - 1), {"leaves": _column_hook("quotient", w_q - 1)})
        add("final_poly", (sh["final_len"] - 1, 1), {"final_poly": lambda f: f[:-1] + [_bump(f[-1], 1)]})
    elif name == "f-none":
        for b, col in columns:
            add("initial", (b, col), {"leaves": _column_hook(b, col)})
    else:
        for i, ab in enumerate(arities):
            pos = rng.randrange(1 << ab)
            wi = _within(arities, i)
            add("fri_layer", (i, "within"), {"fri_layer": _layer_hook(i, pos, 0), "pow_witness": _nth_witness(lambda idx: wi(idx[0]) == pos)})
            add("fri_layer", (i, "other"), {"fri_layer": _layer_hook(i, pos, 0),
                                            "pow_witness": _nth_witness(lambda idx: all(wi(x) != pos for x in idx))})
            add("fri_layer", (i, "second"), {"fri_layer": _layer_hook(i, pos, 1), "pow_witness": _nth_witness(lambda idx: wi(idx[0]) == pos)})
    if name == "f-1-1":
        for k in (1, 4):      # the second and the fifth valid witness: accepted
            add("witness", k, {"pow_witness": _nth_witness(lambda idx: True, k)}, PROOF_OK)
        for b, col in columns:
            add("initial", (b, col), {"leaves": _column_hook(b, col)})
        last = sh["final_len"] - 1
        assert last >= 1
        for i in (0, last):
            for comp in (0, 1):
                add("final_poly", (i, comp), {"final_poly": lambda f, i=i, comp=comp: f[:i] + [_bump(f[i], comp)] + f[i + 1:]})
        for k in range(sh["rounds"]):
            add("one_round", k, _one_round_hooks(c, k, rng))
        # precedence: a fold fault in round 0 and a Merkle fault in round 3, then the other way round (the oracle decides)
        sib = {(f.label[1], f.label[2]): f for f in fields(name) if f.label[0] == "sibling" and f.label[3:] == (0, 0)}
        for k_fri, r_merkle in ((0, 3), (3, 0)):
            raw = _forge(name, _one_round_hooks(c, k_fri, rng))
            f = sib[(r_merkle, 1)]
            raw = patched(raw, f, tampered_value(raw, f))
            out.append(Forgery("precedence", (k_fri, r_merkle), raw, None))
    _FORGERIES[name] = out
    return out
