"""Range proofs of different sizes in ONE combination, on the CPU: BatchRangeVerifier.merge_prefix and the host path of
MixedBatchRangeVerifier with the oracle's MSM and point decompression in place of the HIP engine.  The proofs are the oracle prover's, two
each of 2, 4 and 8 bits over the prefixes of ONE 8-generator list."""
import random

import pytest

import bulletproofs_amd  # noqa: F401
from bulletproofs_amd.rangeproofs import MixedBatchRangeVerifier
from bulletproofs_amd.rangeproofs.batch import BatchRangeVerifier
from bulletproofs_amd.rangeproofs.codec import proof_to_bytes

from helpers import Q
from test_batch_verify_cpu import make_batch, oracle_decompress, oracle_msm

ZERO64 = bytes(64)
SIZES = (2, 4, 8)


@pytest.fixture(scope="module")
def batches():
    """n -> the batch of two n-bit proofs; make_batch derives gs / hs index by index, so the lists of the smaller sizes are prefixes of n = 8's"""
    out = {n: make_batch(2, n=n) for n in SIZES}
    big = out[8]
    for n in SIZES:
        b = out[n]
        assert [p.to_le64() for p in b["gs"]] == [p.to_le64() for p in big["gs"][:n]] and [p.to_le64() for p in b["hs"]] == [p.to_le64() for p in big["hs"][:n]]
        assert (b["g"].to_le64(), b["h"].to_le64(), b["u"].to_le64()) == (big["g"].to_le64(), big["h"].to_le64(), big["u"].to_le64())
        b["blobs"] = [proof_to_bytes(pr) for pr in b["proofs"]]
    return out


def prefix_state(b, Vs=None, rng=None):
    bv = BatchRangeVerifier(b["g"], b["h"], b["gs"], b["hs"], b["u"], msm=oracle_msm, rng=rng)
    bv.add_wire_native(Vs or b["Vs"], b["blobs"], decompress=oracle_decompress, prepare="host", threads=2)
    return bv


def full_verifier(batches):
    big = batches[8]
    return BatchRangeVerifier(big["g"], big["h"], big["gs"], big["hs"], big["u"], msm=oracle_msm)


def test_merge_prefix_of_three_sizes_verifies_as_one_msm(batches):
    full = full_verifier(batches)
    for n in SIZES:
        full.merge_prefix(prefix_state(batches[n]).state())
    assert full.count == 6 and full.partial() == ZERO64 and full.verify() is True
    # merge (same generators) would put the constants of the 2-bit class on all eight generators: it refuses the shorter state
    with pytest.raises(AssertionError):
        full_verifier(batches).merge(prefix_state(batches[2]).state())


def test_one_swapped_commitment_is_rejected(batches):
    full = full_verifier(batches)
    for n in SIZES:
        b = batches[n]
        Vs = list(reversed(b["Vs"])) if n == 4 else b["Vs"]            # the two 4-bit proofs with each other's commitments
        full.merge_prefix(prefix_state(b, Vs).state())
    assert full.partial() != ZERO64
    with pytest.raises(Exception, match="Proof invalid"):
        full.verify()


def test_merge_prefix_folds_nonzero_constants_into_the_prefix_only(batches):
    st = prefix_state(batches[4]).state()
    c_g, c_h, c_u, gk, hk, c_gs, c_hs, pts, scs, nsc, count = st
    assert gk % Q != 0 and hk % Q != 0 and len(c_gs) == 4
    full = full_verifier(batches)
    full.merge_prefix(st)
    by_hand = full_verifier(batches)
    by_hand.merge((c_g, c_h, c_u, 0, 0, [v + gk for v in c_gs] + [0] * 4, [v + hk for v in c_hs] + [0] * 4, pts, scs, nsc, count))
    assert full._gs_const == 0 and full._hs_const == 0
    assert [v % Q for v in full.c_gs] == [v % Q for v in by_hand.c_gs] and [v % Q for v in full.c_hs] == [v % Q for v in by_hand.c_hs]
    assert all(v % Q == 0 for v in full.c_gs[4:] + full.c_hs[4:]) and any(v % Q for v in full.c_gs[:4])
    assert full.partial() == by_hand.partial() == ZERO64


def mixed_items(batches):
    return [(V, blob) for n in SIZES for V, blob in zip(batches[n]["Vs"], batches[n]["blobs"])]


def test_mixed_verifier_on_shuffled_items(batches):
    big = batches[8]
    items = mixed_items(batches)
    random.Random(3).shuffle(items)
    mv = MixedBatchRangeVerifier(big["g"], big["h"], big["gs"], big["hs"], big["u"], msm=oracle_msm, decompress=oracle_decompress)
    assert [(n, m, len(idx)) for n, m, _, idx in mv.classes(items)] == [(2, 1, 2), (4, 1, 2), (8, 1, 2)]
    assert mv.partial_wire(items) == ZERO64 and mv.verify_wire(items) is True and mv.partial_wire([]) == ZERO64
    # [V] is V
    assert mv.verify_wire([([V], blob) for V, blob in items]) is True
    swapped = list(items)
    (V0, b0), (V1, b1) = swapped[0], swapped[1]
    swapped[0], swapped[1] = (V1, b0), (V0, b1)
    with pytest.raises(Exception, match="Proof invalid"):
        mv.verify_wire(swapped)


def test_mixed_verifier_weights_follow_the_global_class_major_index(batches):
    """With an rng the host path draws 4 weights per proof in class-major order: the value of a REJECTED batch (never the identity, so the
    comparison says something) equals the one built by hand from per-class verifiers fed by the same stream."""
    big = batches[8]
    items = mixed_items(batches)
    items[2] = (items[3][0], items[2][1])                                 # a 4-bit proof with the other's commitment
    shuffled = list(items)
    random.Random(4).shuffle(shuffled)
    r1, r2 = random.Random(9), random.Random(9)
    mv = MixedBatchRangeVerifier(big["g"], big["h"], big["gs"], big["hs"], big["u"], msm=oracle_msm, rng=lambda: r1.getrandbits(320), decompress=oracle_decompress)
    got = mv.partial_wire(shuffled)
    full = full_verifier(batches)
    for n, m, _, idx in mv.classes(shuffled):
        b = batches[n]
        bv = BatchRangeVerifier(b["g"], b["h"], b["gs"], b["hs"], b["u"], msm=oracle_msm, rng=lambda: r2.getrandbits(320))
        bv.add_wire_native([shuffled[i][0] for i in idx], [shuffled[i][1] for i in idx], decompress=oracle_decompress, prepare="host", threads=1)
        full.merge_prefix(bv.state())
    assert got != ZERO64 and got == full.partial()


def test_sizes_that_do_not_fit_are_invalid_proofs(batches):
    big = batches[8]
    mv = MixedBatchRangeVerifier(big["g"], big["h"], big["gs"][:4], big["hs"][:4], big["u"], msm=oracle_msm, decompress=oracle_decompress)
    V, blob = batches[8]["Vs"][0], batches[8]["blobs"][0]
    for item in ((V, blob), ([V, V, V], batches[4]["blobs"][0]), (V, blob[:5]), (V, b"XXXX" + blob[4:])):
        with pytest.raises(Exception, match="Proof invalid"):
            mv.partial_wire([item])
