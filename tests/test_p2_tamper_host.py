"""Native plonky2 verifier, host path, against rejected proofs (tests/p2_tamper_cases.py): a change to ANY field of a proof is
rejected, with the status of the verifier restatement (oracle/plonky2_verifier.py) on a stratified sample; proofs of a dishonest
prover with honest Merkle paths, transcript and proof of work are rejected by the FRI fold chain alone.  The GPU tests
(tests/test_gpu_p2_tamper.py) compare the kernels with the host path on the same batches."""
import concurrent.futures
import multiprocessing
import random

import pytest

import zklc_amd  # noqa: F401
from zklc_amd.plonky2 import serialization as S, HASH_GL, HASH_BN128
from zklc_amd.plonky2.verifier import Verifier, PROOF_OK, PROOF_BAD_FORMAT, PROOF_BAD_MERKLE, PROOF_BAD_FRI
from oracle import plonky2_prover as OP, plonky2_verifier as V, poseidon_gl as pgl
from test_plonky2_verifier_host import oracle_status
import p2_matrix_cases as M
import p2_tamper_cases as T

ALL_SWEEPS = T.SWEEP_NAMES + ["golden"]


@pytest.fixture(scope="module", autouse=True)
def _fast_poseidon():
    pgl.use_c_port()


def _expected(job):
    name, f, raw = job
    return T.expected_status(T.circuit(name), f, raw)


def oracle_statuses(name, items):
    """expected_status of [(Field, bytes)], on 16 forked workers (the restatement is pure Python; the golden proof takes it 1.5 s)"""
    T.circuit(name)
    with concurrent.futures.ProcessPoolExecutor(16, mp_context=multiprocessing.get_context("fork")) as ex:
        return list(ex.map(_expected, [(name, f, raw) for f, raw in items], chunksize=4))


def host_statuses(name, proofs):
    c = T.circuit(name)
    out = []
    with Verifier(None, c.common, c.vd, c.hasher) as v:
        assert v.proof_bytes == len(c.raw)
        for part in T.chunks(proofs):
            out += v.verify_batch_host(part)
    return out


@pytest.mark.parametrize("hasher", [HASH_GL, HASH_BN128])
def test_field_map_tiles_the_proof(hasher):
    for name in ALL_SWEEPS + list(T.FORGE_CASES):
        c = T.circuit(name)
        if c.hasher != hasher:
            continue
        fs = T.proof_fields(c.common, c.hasher)
        at = 0
        for f in fs:
            assert f.offset == at and f.size in (1, 8, 32), (name, f)      # no gap, no overlap
            at += f.size
        assert at == len(c.raw) == S.proof_size(c.common, c.hasher), name
        assert len({f.label for f in fs}) == len(fs)
        kinds = {f.kind for f in fs}
        assert kinds == ({"gl", "count8", "count64"} | ({"digest"} if hasher == HASH_BN128 else set())), (name, kinds)
        assert [f.label for f in fs if f.kind == "count64"] == [("npi",)] and T.value(c.raw, fs[-1 - c.common["num_public_inputs"]]) \
            == c.common["num_public_inputs"]
        assert sum(f.label == ("pow",) for f in fs) == 1
        if hasher == HASH_GL:      # the u64 fields are exactly serialization.proof_offsets' elements
            flat = []

            def walk(x):
                if isinstance(x, dict):
                    for y in x.values():
                        walk(y)
                elif isinstance(x, list):
                    for y in x:
                        walk(y)
                else:
                    flat.append(x)
            walk(S.proof_offsets(c.raw, c.common, HASH_GL))
            assert sorted(flat) == [f.offset for f in fs if f.kind == "gl"], name


@pytest.mark.parametrize("name", ALL_SWEEPS)
def test_patched_bytes_are_the_json_level_change(name):
    """a seeded sample of fields: the patched bytes == proof_to_bytes of the proof.json with that one value changed; the field
    holds the honest proof's value of that label"""
    c = T.circuit(name)
    pj = S.proof_from_bytes(c.raw, c.common, c.hasher)
    fs = [f for f in T.fields(name) if f.kind in ("gl", "digest")]
    rng = random.Random(5)
    by_region = {}
    for f in fs:
        by_region.setdefault((T.region(f)[:2], f.kind), []).append(f)
    sample = [rng.choice(v) for v in by_region.values()] + rng.sample(fs, 40)
    for f in sample:
        v = T.tampered_value(c.raw, f)
        assert v != T.value(c.raw, f)
        assert S.proof_to_bytes(T.json_with(pj, f, v), c.common, c.hasher) == T.patched(c.raw, f, v), (name, f)
        assert S.proof_to_bytes(T.json_with(pj, f, T.value(c.raw, f)), c.common, c.hasher) == c.raw, (name, f)


def test_prover_without_hooks_is_unchanged():
    """prove(hooks=None), prove(hooks={}) and the C prover give the same bytes (tests/test_oracle_cprover.py pins the last two to
    each other over more circuits)"""
    case = T.FORGE_CASES["f-1-1"][0]
    data, wires, pis = M.make(case)
    c = T.circuit("f-1-1")
    for hooks in (None, {}):
        pj, vd = OP.prove(c.common, data.constants, data.sigmas, wires, pis, V.HasherGL, hooks=hooks)
        assert S.proof_to_bytes(pj, c.common, HASH_GL) == c.raw and vd == c.vd
    # a hook that changes nothing and the lowest witness: the same bytes again
    same = {"leaves": lambda n, l: None, "fri_layer": lambda i, l: None, "final_poly": lambda f: None,
            "pow_witness": lambda cands: next(cands)[0]}
    pj, _ = OP.prove(c.common, data.constants, data.sigmas, wires, pis, V.HasherGL, hooks=same)
    assert S.proof_to_bytes(pj, c.common, HASH_GL) == c.raw


@pytest.mark.parametrize("name", ALL_SWEEPS)
def test_every_tampered_field_is_rejected(name):
    """NO exemptions: the format leaves no field of a proof unbound"""
    c = T.circuit(name)
    sw = T.sweep(name)
    assert host_statuses(name, [c.raw]) == [PROOF_OK]
    got = host_statuses(name, [raw for _, raw in sw])
    accepted = [f.label for (f, _), st in zip(sw, got) if st == PROOF_OK]
    print(name, len(c.raw), "bytes,", len(sw), "tampered copies, statuses", sorted(set(got)))
    assert not accepted, (name, accepted[:20])
    if name != "golden":
        assert len(sw) == len(T.fields(name))
    # elements and digests stay canonical, so only the counts may stop at FORMAT (the golden selection's top-word flips apart)
    for (f, raw), st in zip(sw, got):
        assert (st == PROOF_BAD_FORMAT) == (f.kind in ("count8", "count64") or not T.is_canonical(f, raw)), (name, f, st)


@pytest.mark.parametrize("name", ALL_SWEEPS)
def test_host_path_equals_the_oracle_on_a_sample(name):
    sw = T.sweep(name)
    idx = T.oracle_sample(name)
    assert len(idx) >= 150
    items = [sw[i] for i in idx]
    want = oracle_statuses(name, items)
    got = host_statuses(name, [raw for _, raw in items])
    bad = [(f.label, g, w) for (f, _), g, w in zip(items, got, want) if g != w]
    print(name, len(items), "sampled, statuses", sorted(set(want)))
    assert not bad, (name, bad[:20])
    assert PROOF_OK not in want
    if name != "tamper-tiny-2^2":
        assert {PROOF_BAD_MERKLE, PROOF_BAD_FRI} <= set(want), (name, set(want))


@pytest.mark.parametrize("name", ALL_SWEEPS)
def test_noncanonical_values_are_format_errors(name):
    items = T.noncanonical(name)
    regions = {T.region(f)[0] for f, _ in items}
    assert {"cap", "opening", "leaf", "sibling", "final", "pow", "pi"} <= regions
    if S.shapes(T.circuit(name).common)["arity_bits"]:
        assert {"commit_cap", "eval"} <= regions
    assert host_statuses(name, [raw for _, raw in items]) == [PROOF_BAD_FORMAT] * len(items)


@pytest.mark.parametrize("name", list(T.FORGE_CASES))
def test_forgeries(name):
    """the oracle first: its verdict is the expected one (FRI; OK for a non-minimal witness); then the host path equals it"""
    c = T.circuit(name)
    fg = T.forgeries(name)
    want = []
    for f in fg:
        st = oracle_status(S.proof_from_bytes(f.raw, c.common, c.hasher), c.vd, c.common)
        assert f.want is None or st == f.want, (name, f.kind, f.label, st)
        want.append(st)
    got = host_statuses(name, [f.raw for f in fg])
    print(name, [(f.kind, f.label, st) for f, st in zip(fg, want)])
    assert got == want, [(f.kind, f.label, g, w) for f, g, w in zip(fg, got, want) if g != w]
    prec = {f.label: st for f, st in zip(fg, want) if f.kind == "precedence"}
    if prec:      # the earlier round's fault decides
        assert prec == {(0, 3): PROOF_BAD_FRI, (3, 0): PROOF_BAD_MERKLE}


def test_forgery_catalogue_counts():
    kinds = {}
    for name in T.FORGE_CASES:
        for f in T.forgeries(name):
            kinds[f.kind] = kinds.get(f.kind, 0) + 1
    assert kinds == {"witness": 2, "fri_layer": 19, "initial": 15, "final_poly": 5, "one_round": 7, "precedence": 2,
                     "sole_check": 4}, kinds
