"""groth16.Setup on the GPU.  The scalar stage (zklc_groth16_setup_scalars_dev: csrc/groth16_setup.{cuh,hip}) against
`oracle.groth16.key_scalars` and against the host twin on every system and toxic set of tests/setup_cases.py -- domains 2 and 4 (the
transform's smallest sizes), live padding, a column cut into segments (asserted from the plan the DEVICE made, read back from the
head of its workspace), columns for 1 / 8 / 64 lanes, duplicates and zero coefficients, tau = 0 and tau in the domain.  Then the
whole of `KeySetup.run()` at the 4000-constraint chain system and the 2^13 bits system: the key it makes is handed to `Groth16Prover`
as it is, and the proofs are the closed form's.  Every comparison is exact equality of integers."""
import numpy as np
import pytest
import torch

import groth16_size_cases as S
import setup_cases as C
from oracle import groth16 as G
from zklc_amd import _lib, groth16_setup as GS
from zklc_amd.groth16 import (Groth16Prover, Groth16Verifier, KeySetup, NativeGroth16Verifier, Setup, setup_scalars_dev,
                              setup_scalars_host)
from zklc_amd.r1cs import R1CS

pytestmark = pytest.mark.gpu

R = G.R
INVALID = -1
RS = [(0, 0), (R - 1, R - 1), (0x2b1f0c3d5e6f708192a3b4c5d6e7f8091a2b3c4d5e6f70819a, 0x1d9e8f7a6b5c4d3e2f1a0b9c8d7e6f5a4b3c2d1e0f9a8b7c6d)]
KEY_CASES = [("chain", 12, "chain4000"), ("bits", 13, "bits8192")]


def make_r1cs(name, ctx):
    sy = C.system(name)
    return R1CS.from_csr(sy["n_constraints"], sy["n_wires"], *sy["csr"], ctx=ctx)


@pytest.fixture(scope="module")
def systems(zctx):
    out = {name: make_r1cs(name, zctx) for name in C.SYSTEM_NAMES}
    yield out
    for s in out.values():
        s.close()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("system_name,toxic_name", C.CASES, ids=C.CASE_IDS)
def test_device_scalars_equal_the_oracle_and_the_host_twin(zctx, systems, system_name, toxic_name):
    sy = C.system(system_name)
    toxic = C.toxic(toxic_name, sy["n"])
    want = C.expected_words(system_name, toxic_name)
    sc = setup_scalars_dev(zctx, systems[system_name], sy["n_public"], toxic)
    zctx.synchronize()
    assert sc.n == sy["n"]
    twin = setup_scalars_host(systems[system_name], sy["n_public"], toxic)
    for name, t, w, h in zip(("a_t", "b_t", "k", "z"), (sc.a_t, sc.b_t, sc.k, sc.z), want, twin):
        got = _host(t)
        assert got.shape == w.shape and np.array_equal(got, w), "%s differs from the oracle" % name
        assert np.array_equal(got, h), "%s differs from the host twin" % name
    assert sc.plan() == C.expected_plan(system_name, GS.SEG_TERMS) == GS.plan(systems[system_name])


def test_the_4000_constraint_system_goes_through_the_segment_split(zctx, systems):
    """the constant wire's C column (4000 general terms) is the one column cut into segments, two of them, by the DEVICE's own
    count; the other systems have none"""
    sy = C.system("chain4000")
    assert C.column_lengths("chain4000")[(2, 0)] == 4000 > GS.SEG_TERMS
    sc = setup_scalars_dev(zctx, systems["chain4000"], sy["n_public"], S.TOXIC)
    zctx.synchronize()
    p = sc.plan()
    assert p["cols_segmented"] == 1 and p["segments"] == -(-4000 // GS.SEG_TERMS) >= 2 and p["cols_64_lanes"] == 3
    assert p["cols_1_lane"] + p["cols_64_lanes"] + p["cols_segmented"] == 3 * sy["n_wires"]
    t = GS.last_timings()
    assert tuple(t) == GS.STAGES and all(v >= 0 for v in t.values())
    for name in ("chain100", "bits8192", "hand5"):
        assert GS.plan(systems[name])["cols_segmented"] == 0


def test_a_larger_domain_than_the_constraints_need(zctx, systems):
    sy = C.system("chain100")
    sc = setup_scalars_dev(zctx, systems["chain100"], sy["n_public"], S.TOXIC, n=256)
    zctx.synchronize()
    twin = setup_scalars_host(systems["chain100"], sy["n_public"], S.TOXIC, n=256)
    assert sc.z.shape == (255, 4)
    for t, h in zip((sc.a_t, sc.b_t, sc.k, sc.z), twin):
        assert np.array_equal(_host(t), h)


def test_malformed_calls_are_invalid_arguments_and_launch_nothing(zctx, systems):
    lib = _lib.load()
    dev = torch.device("cuda", zctx.device_id)
    sy = C.system("chain3")
    s, npub, n, nw = systems["chain3"], sy["n_public"], sy["n"], sy["n_wires"]
    ws_bytes = int(lib.zklc_groth16_setup_workspace_bytes(s._handle(), n))
    assert ws_bytes > 0
    fill = lambda words: torch.full((words,), 0x1111111111111111, dtype=torch.int64, device=dev)
    a_t, b_t, k, z, ws = fill(4 * nw + 2), fill(4 * nw + 2), fill(4 * nw + 2), fill(4 * (n - 1) + 2), fill(ws_bytes // 8 + 2)
    torch.cuda.synchronize(dev)
    good = GS.toxic_words(S.TOXIC)
    host_only = R1CS.from_csr(sy["n_constraints"], nw, *sy["csr"])

    def call(ctx=zctx, sys_=s, toxic=good, n_public=npub, n_=n, ptrs=None, ws_ptr=None, ws_len=ws_bytes):
        p = list(ptrs or [x.data_ptr() for x in (a_t, b_t, k, z)])
        return lib.zklc_groth16_setup_scalars_dev(ctx._h if ctx is not None else None, zctx.stream_ptr(), sys_._handle() if sys_ is not None
                                                  else None, toxic.ctypes.data if toxic is not None else None, n_public, n_, *p,
                                                  ws.data_ptr() if ws_ptr is None else ws_ptr, ws_len)

    def with_toxic(i, v):
        t = list(S.TOXIC)
        t[i] = v
        return GS.toxic_words(t)
    base = [x.data_ptr() for x in (a_t, b_t, k, z)]
    bad = {
        "gamma = 0": dict(toxic=with_toxic(3, 0)), "gamma = r": dict(toxic=with_toxic(3, R)), "delta = 0": dict(toxic=with_toxic(4, 0)),
        "n = 3": dict(n_=3), "n below the constraints": dict(n_=2), "n = 0": dict(n_=0), "n = 2^29": dict(n_=1 << 29),
        "n_public + 1 > n_wires": dict(n_public=nw), "no context": dict(ctx=None), "no system": dict(sys_=None),
        "a system without a context": dict(sys_=host_only), "no toxic waste": dict(toxic=None),
        "a workspace one byte short": dict(ws_len=ws_bytes - 1), "no workspace": dict(ws_ptr=0, ws_len=ws_bytes),
        "a misaligned workspace": dict(ws_ptr=ws.data_ptr() + 8),
    }
    for i, name in enumerate(("a_t", "b_t", "k", "z")):
        bad["no " + name] = dict(ptrs=base[:i] + [None] + base[i + 1:])
        bad["misaligned " + name] = dict(ptrs=base[:i] + [base[i] + 8] + base[i + 1:])
    try:
        for what, kw in bad.items():
            assert call(**kw) == INVALID, what
        zctx.synchronize()
        for x in (a_t, b_t, k, z, ws):
            assert bool((x == 0x1111111111111111).all()), "a refused call writes nothing"
        with pytest.raises(_lib.ZklcError) as e:
            setup_scalars_dev(zctx, s, npub, (1, 2, 3, 0, 5))
        assert e.value.code == INVALID
        assert call() == 0
        zctx.synchronize()
        assert np.array_equal(_host(a_t[:4 * nw]).reshape(-1, 4), C.expected_words("chain3", "base")[0])
        assert bool((a_t[4 * nw:] == 0x1111111111111111).all()) and bool((z[4 * (n - 1):] == 0x1111111111111111).all())
        # toxic needs 8-byte alignment only: the same words at 8 mod 16 are a GOOD call with the same scalars
        raw = np.zeros(24, dtype=np.uint64)
        off = (-raw.ctypes.data % 16) // 8 + 1
        shifted = raw[off:off + 20]
        shifted[:] = good.reshape(-1)
        assert shifted.ctypes.data % 16 == 8
        a_t[:4 * nw] = 0
        torch.cuda.synchronize(dev)
        assert call(toxic=shifted) == 0
        zctx.synchronize()
        assert np.array_equal(_host(a_t[:4 * nw]).reshape(-1, 4), C.expected_words("chain3", "base")[0])
    finally:
        host_only.close()


@pytest.fixture(scope="module", params=KEY_CASES, ids=["%s-2p%d" % c[:2] for c in KEY_CASES])
def key(request, zctx):
    """one system: KeySetup.run() on the GPU, the prover over its key with the constraint system resident, the oracle's scalars"""
    kind, log_n, name = request.param
    sy = dict(S.system(kind, log_n))
    sc = C.expected(name, "base")["scalars"]
    assert sc["n"] == 1 << log_n and sc["n_wires"] == len(sy["witness"]) and C.toxic("base", sc["n"]) == S.TOXIC
    sys_ = R1CS.from_rows(*sy["r1cs"], sc["n_wires"], ctx=zctx)
    ks = KeySetup(zctx, sys_, sy["n_public"], S.TOXIC, window_bits=16)
    pk, vk = ks.run(timings=True)
    prover = Groth16Prover(zctx, pk, sys_)
    sy.update(scalars=sc, ks=ks, pk=pk, vk=vk, prover=prover, name=name)
    yield sy
    prover.close()
    sys_.close()


def test_the_key_has_the_oracles_masks_and_lengths(key):
    sc, pk = key["scalars"], key["pk"]
    inf_a, inf_b = [x == 0 for x in sc["a_t"]], [x == 0 for x in sc["b_t"]]
    assert pk["infinity_a"].tolist() == inf_a and pk["infinity_b"].tolist() == inf_b
    assert sum(inf_a) >= 4 and sum(inf_b) >= 4 and (key["kind"] != "bits" or min(sum(inf_a), sum(inf_b)) >= 50)
    assert pk["n"] == sc["n"] and pk["n_public"] == key["n_public"]
    assert len(pk["A_dev"]) == len(inf_a) - sum(inf_a) and len(pk["B1_dev"]) == len(pk["B2_dev"]) == len(inf_b) - sum(inf_b)
    assert len(pk["K_dev"]) == len(sc["k_pk"]) == sc["n_wires"] - 1 - key["n_public"] and len(pk["Z_dev"]) == sc["n"] - 1
    assert pk["A_dev"].shape[1] == pk["B1_dev"].shape[1] == pk["K_dev"].shape[1] == pk["Z_dev"].shape[1] == 8 and pk["B2_dev"].shape[1] == 16
    # no point at infinity is left in the compacted arrays
    for name in ("A_dev", "B1_dev", "B2_dev"):
        assert bool((pk[name] != 0).any(dim=1).all()), name
    assert set(key["ks"].last_ms) == set(GS.STAGES) | {"points_" + k for k in ("A", "B1", "K", "Z", "B2")}


def test_the_verifying_key_is_the_closed_form(key):
    want = G.closed_form_vk(key["scalars"], S.TOXIC, key["n_public"])
    assert {k: key["vk"][k] for k in want} == want


def test_proofs_under_the_key_equal_the_closed_form(zctx, key):
    """Groth16Prover(ctx, pk, r1cs) takes the key as it is; prove_witness gives the closed form's eight words for the three (r, s)"""
    prover = key["prover"]
    for r, s in RS:
        want = G.closed_form_proof(key["scalars"], S.TOXIC, key["n_public"], key["witness"], r, s)
        assert prover.prove_witness(key["witness"], r, s) == want, "(r, s) = (%#x, %#x)" % (r, s)


def test_the_verifier_accepts_under_the_made_key_and_rejects_a_changed_input(zctx, key):
    proof = key["prover"].prove_witness(key["witness"], *RS[2])
    ver = Groth16Verifier(zctx, key["vk"])
    pubs = key["publics"]
    assert ver.verify(proof, pubs) is True
    assert ver.verify(proof, [pubs[0], (pubs[1] + 1) % R, pubs[2]]) is False


def test_clear_leaves_no_scalar_and_no_toxic_value(zctx, key):
    """after clear() every tensor of buffers() is all zero and the object holds no toxic value; the key is untouched"""
    ks = key["ks"]
    bufs = ks.buffers()
    # a_t, b_t, k, z, the scalar stage's workspace, the two batches with the single scalars appended and the single scalars themselves;
    # the fixed-base workspaces were zero-filled and released one by one during the run
    assert len(bufs) >= 9 and any(int(t.count_nonzero()) for t in bufs)
    assert all(any(t is b for b in bufs) for t in ks.scalars.tensors())
    assert sum(t.numel() * t.element_size() for t in bufs) > 4 * 32 * key["scalars"]["n_wires"]
    before = key["pk"]["K_dev"].clone()
    ks.clear()
    assert all(int(t.count_nonzero()) == 0 for t in bufs)
    assert ks.toxic is None and not any(isinstance(v, tuple) for v in vars(ks).values())
    assert torch.equal(before, key["pk"]["K_dev"]) and int(before.count_nonzero()) > 0
    with pytest.raises(ValueError):
        ks.run()


def test_setup_with_fresh_toxic_waste_yields_a_key_under_which_a_proof_verifies(zctx):
    """Setup(..., toxic=None): nobody knows the scalars, so the check is the pairing equation -- by the kernel verifier and by the
    native one -- with the right public inputs and with a changed one"""
    r1cs, wit = G.square_chain_r1cs(100, n_public=3)
    pubs = [11, 22, 33]
    w = wit(pubs, 5)
    sys_ = R1CS.from_rows(*r1cs, len(w), ctx=zctx)
    try:
        pk, vk = Setup(zctx, sys_, 3)
        pk2, vk2 = Setup(zctx, sys_, 3)
        assert vk["alpha1"] != vk2["alpha1"] and vk["K"] != vk2["K"], "two runs drew the same toxic waste"
        prover = Groth16Prover(zctx, pk, sys_)
        try:
            proof = prover.prove_witness(w, 12345, 67890)
        finally:
            prover.close()
        ver = Groth16Verifier(zctx, vk)
        assert ver.verify(proof, pubs) is True and ver.verify(proof, [11, 22, 34]) is False
        assert Groth16Verifier(zctx, vk2).verify(proof, pubs) is False
        native = NativeGroth16Verifier(zctx, vk)
        try:
            assert native.verify_batch([proof, proof], [pubs, [11, 23, 33]]) == [0, 5]
        finally:
            native.close()
    finally:
        sys_.close()
