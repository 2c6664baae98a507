"""Native plonky2 verifier on the GPU against the rejected proofs of tests/p2_tamper_cases.py: the kernels give every tampered
copy and every dishonest-prover proof the host path's status (which tests/test_p2_tamper_host.py pins to the verifier
restatement), element for element, in batches with honest proofs at the first, the last and seeded interior positions."""
import random

import pytest

import zklc_amd  # noqa: F401
from zklc_amd.plonky2 import serialization as S
from zklc_amd.plonky2.verifier import Verifier, PROOF_OK
import p2_tamper_cases as T

pytestmark = pytest.mark.gpu
GOLDEN_PARTS = 7       # of 4 query rounds each: a batch is under 64 MB of proof bytes


def _compare(zctx, name, proofs, seed=7):
    """one batch on the device and on the host: equal statuses, the honest copies accepted and nothing else; then a batch of 3
    on the same verifier, whose buffers still hold the large batch beyond the new one's end"""
    c = T.circuit(name)
    batch, honest = T.device_batch(name, proofs, seed)
    assert len(batch) % 64 and honest[0] == 0 and honest[-1] == len(batch) - 1 and len(honest) >= 4
    assert len(batch) * len(c.raw) <= 64 << 20
    with Verifier(zctx, c.common, c.vd, c.hasher) as v:
        got, want = v.verify_batch(batch), v.verify_batch_host(batch)
        wrong = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not wrong, (name, len(batch), wrong[:20])
        assert all(got[i] == PROOF_OK for i in honest), (name, [got[i] for i in honest])
        rng = random.Random(seed)
        three = [honest[2], rng.choice([i for i in range(len(batch)) if i not in honest]), len(batch) - 2]
        assert v.verify_batch([batch[i] for i in three]) == [got[i] for i in three], (name, three)
    return batch, honest, got


@pytest.mark.parametrize("name", T.SWEEP_NAMES)
def test_field_sweep(zctx, name):
    """every field of the proof: the whole sweep and the non-canonical copies in one batch; no tampered copy is accepted"""
    proofs = [raw for _, raw in T.sweep(name) + T.noncanonical(name)]
    batch, honest, got = _compare(zctx, name, proofs)
    accepted = [i for i, st in enumerate(got) if st == PROOF_OK and i not in honest]
    assert not accepted, (name, accepted[:20])
    assert len(set(got)) >= 4, (name, set(got))


@pytest.mark.parametrize("part", range(GOLDEN_PARTS))
def test_golden_selection(zctx, part):
    """the stratified selection over the reference's 28-round wrap proof, four query rounds to a batch (the fields outside the
    query rounds with the first)"""
    rounds = S.shapes(T.circuit("golden").common)["rounds"]
    assert rounds == 4 * GOLDEN_PARTS
    proofs = []
    for f, raw in T.sweep("golden") + T.noncanonical("golden"):
        r = T.region(f)[2]
        if (r // 4 if r is not None else 0) == part:
            proofs.append(raw)
    assert len(proofs) >= 150
    batch, honest, got = _compare(zctx, "golden", proofs, seed=part)
    assert not [i for i, st in enumerate(got) if st == PROOF_OK and i not in honest]


@pytest.mark.parametrize("name", list(T.FORGE_CASES))
def test_forgeries(zctx, name):
    """every dishonest-prover proof of one circuit beside honest proofs and a seeded sample of its honest proof's field sweep:
    the fold-chain checks of p2v_fri_kernel are the only thing that rejects the forgeries"""
    c = T.circuit(name)
    fg = T.forgeries(name)
    rng = random.Random(3)
    tampers = [T.patched(c.raw, f, T.tampered_value(c.raw, f)) for f in rng.sample(T.fields(name), 60)]
    proofs = [f.raw for f in fg] + tampers
    rng.shuffle(proofs)
    batch, honest, got = _compare(zctx, name, proofs)
    status = dict(zip(batch, got))
    for f in fg:
        assert f.want is None or status[f.raw] == f.want, (name, f.kind, f.label, status[f.raw])
