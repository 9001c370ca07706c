"""The Python side of the packed mixed batch verifier (MixedBatchInnerProductVerifier.verify_packed* / locate_packed*,
python-bulletproofs_amd/innerproduct/batch_mixed.py) without a GPU: the row sizes, the round count read from a class's rows (k = 0
included), a class beyond the capacity refused on the host, and the cutting of an oversized batch into consecutive native calls -- over
an engine that records what it is handed and answers from a set of "invalid" proofs."""
import pytest

import bulletproofs_amd  # noqa: F401
from bulletproofs_amd.innerproduct import MixedBatchInnerProductVerifier
from bulletproofs_amd.innerproduct.batch_mixed import CLASSES_MAX, PAIRS_MAX, packed_class_k, split_mixed_calls, split_mixed_ranges


class FakeEngine:
    """ipa_verify_batch_packed_mixed_dev over tagged rows: byte 0..3 of a proof's `ab` row is its tag; a tag in `flag` gets status 1, one
    in `silent` makes out non-zero."""

    def __init__(self, flag=(), silent=()):
        self.flag, self.silent, self.calls = set(flag), set(silent), []

    def upload(self, data):
        return object()

    def ipa_verify_batch_packed_mixed_dev(self, d_g, d_h, n_gens, protocol, classes, weights, seed, d_hscale):
        assert (weights is None) != (seed is None) and len(classes) <= 64
        tags, shapes = [], []
        for k, count, ab, xs, lr, trs, starts, u, P, c, head in classes:
            assert count >= 1 and len(ab) == 64 * count and len(xs) == 32 * k * count and len(lr) == 128 * k * count and len(trs) == count and len(P) == 64 * count
            assert len(u) == (64 if protocol == 1 else 64 * count) and len(c) == (32 * count if protocol == 1 else 0) and len(head) == (128 * count if protocol == 1 else 0)
            assert starts is None or len(starts) == count
            tags += [int.from_bytes(ab[64 * i: 64 * i + 4], "little") for i in range(count)]
            shapes.append((k, count))
        assert len(tags) <= 1 << 16 and sum(n * (2 * k + (4 if protocol == 1 else 2)) for k, n in shapes) <= 1 << 22
        if weights is not None:
            assert len(weights) == 32 * (3 if protocol == 1 else 1) * len(tags)
        self.calls.append((shapes, tags, weights))
        out = bytes(64) if not any(t in self.silent for t in tags) else b"\x01" + bytes(63)
        return out, bytes(1 if t in self.flag else 0 for t in tags)


def make_class(protocol, k, count, first_tag, starts=False):
    ab = b"".join((first_tag + i).to_bytes(4, "little") + bytes(60) for i in range(count))
    trs = [b"t%d" % (first_tag + i) for i in range(count)]
    if protocol == 2:
        cls = (bytes(64 * count), bytes(64 * count), ab, bytes(32 * k * count), bytes(128 * k * count), trs)
        return cls + ([1] * count,) if starts else cls
    return (bytes(64), bytes(64 * count), bytes(32 * count), ab, bytes(32 * k * count), bytes(128 * k * count), bytes(128 * count), trs)


def verifier(engine, K=6):
    from bulletproofs_amd.ec import Point
    n = 1 << K
    return MixedBatchInnerProductVerifier([Point.IDENTITY_ELEMENT] * n, [Point.IDENTITY_ELEMENT] * n, engine=engine)          # the fake engine never reads them


def test_k_is_read_from_the_rows():
    assert packed_class_k(5, bytes(32 * 3 * 5), bytes(128 * 3 * 5)) == 3
    assert packed_class_k(5, b"", b"") == 0 and packed_class_k(0, b"", b"") == 0
    for xs, lr in ((bytes(32 * 3 * 5 + 1), bytes(128 * 3 * 5)), (bytes(32 * 3 * 5), bytes(128 * 2 * 5)), (bytes(32 * 3 * 5), b"")):
        with pytest.raises(ValueError):
            packed_class_k(5, xs, lr)
    with pytest.raises(ValueError):
        packed_class_k(0, bytes(32), b"")


@pytest.mark.parametrize("protocol", [1, 2])
def test_classes_reach_the_engine_with_their_own_k(protocol):
    eng = FakeEngine()
    bv = verifier(eng)
    classes = [make_class(protocol, 1, 3, 0, starts=True), make_class(protocol, 6, 2, 3), make_class(protocol, 0, 1, 5), make_class(protocol, 3, 0, 6), make_class(protocol, 3, 4, 6)]
    call = bv.verify_packed2 if protocol == 2 else bv.verify_packed1
    assert call(classes) is True
    assert [c[0] for c in eng.calls] == [[(1, 3), (6, 2), (0, 1), (3, 4)]]          # the empty class is dropped, the order kept
    assert eng.calls[0][1] == list(range(10)) and eng.calls[0][2] is None
    nw = 3 if protocol == 1 else 1
    assert call(classes, weights=[[7] * nw if nw > 1 else 7] * 10) is True and len(eng.calls[1][2]) == 32 * nw * 10
    with pytest.raises(ValueError, match="one weight per proof"):
        call(classes, weights=[1] * 9)


def test_row_sizes_and_the_capacity_are_checked_on_the_host():
    eng = FakeEngine()
    bv = verifier(eng, K=3)
    with pytest.raises(ValueError, match="capacity"):
        bv.verify_packed2([make_class(2, 4, 2, 0)])
    good = make_class(2, 2, 3, 0)
    for i, short in ((0, bytes(64 * 2)), (1, bytes(64 * 3 + 1)), (2, bytes(64))):
        bad = list(good)
        bad[i] = short
        with pytest.raises(ValueError):
            bv.verify_packed2([tuple(bad)])
    with pytest.raises(ValueError):
        bv.verify_packed2([good[:4] + (bytes(128 * 2 * 3 - 1),) + good[5:]])          # lr disagrees with the k of xs
    with pytest.raises(ValueError):
        bv.verify_packed2([good + ([1, 1],)])                                         # one start per proof
    p1 = make_class(1, 2, 3, 0)
    with pytest.raises(ValueError):
        bv.verify_packed1([(bytes(128),) + p1[1:]])                                   # u is one point under Protocol 1
    assert eng.calls == []


def test_the_cuts_respect_every_cap():
    items = [(0, 6)] * 5 + [(1, 8)] * 5
    assert split_mixed_calls(items) == [(0, 10)] and split_mixed_calls([]) == []
    assert split_mixed_calls(items, proofs_max=4) == [(0, 4), (4, 8), (8, 10)]
    assert split_mixed_calls(items, pairs_max=30) == [(0, 5), (5, 8), (8, 10)]        # 5 x 6 = 30; then 3 x 8 = 24
    assert split_mixed_calls(items, classes_max=1) == [(0, 5), (5, 10)]
    many = [(c, 2) for c in range(130)]
    assert split_mixed_calls(many) == [(0, 64), (64, 128), (128, 130)] and CLASSES_MAX == 64 and PAIRS_MAX == 1 << 22
    # the form without a loop over proofs cuts at the same global indices
    for caps in ({}, {"proofs_max": 4}, {"pairs_max": 30}, {"classes_max": 1}, {"proofs_max": 3, "pairs_max": 20}):
        calls = split_mixed_ranges([5, 0, 5], [6, 4, 8], **caps)
        flat = [[(c, i) for c, lo, hi in call for i in range(lo, hi)] for call in calls]
        every = [(0, i) for i in range(5)] + [(2, i) for i in range(5)]
        want = split_mixed_calls([(c, (6, 4, 8)[c]) for c, _ in every], **caps)
        assert flat == [every[lo:hi] for lo, hi in want], caps
    assert [len(call) for call in split_mixed_ranges([1] * 130, [2] * 130)] == [64, 64, 2]


def test_an_oversized_batch_runs_as_consecutive_calls_cut_at_global_indices():
    """2^16 + 5 proofs in three classes: two calls, the second one starting inside class 2; verdicts and located indices are global."""
    total = (1 << 16) + 5
    sizes = [(1, 40000), (0, 25000), (2, total - 65000)]
    tag, classes = 0, []
    for k, count in sizes:
        classes.append(make_class(2, k, count, tag))
        tag += count
    eng = FakeEngine()
    bv = verifier(eng)
    assert bv.verify_packed2(classes) is True
    assert [c[0] for c in eng.calls] == [[(1, 40000), (0, 25000), (2, 536)], [(2, 5)]]
    assert eng.calls[0][1] + eng.calls[1][1] == list(range(total))
    ws = list(range(1, total + 1))
    eng.calls = []
    assert bv.verify_packed2(classes, weights=ws) is True
    assert eng.calls[1][2][:32] == (65537).to_bytes(32, "little")                     # the weights are cut at the same global index
    # a flagged proof in the second call, a silent one in the first
    eng = FakeEngine(flag={65540}, silent={39999})
    bv = verifier(eng)
    assert bv.verify_packed2(classes) is False
    assert bv.locate_packed2(classes) == [39999, 65540]
    # extra pairs: 2^16 proofs cannot reach 2^22 of them, so the cap is exercised through the function above; classes: 70 of one proof
    eng = FakeEngine(flag={66})
    bv = verifier(eng)
    small = [make_class(1, 1, 1, t) for t in range(70)]
    assert bv.verify_packed1(small) is False and [len(c[0]) for c in eng.calls] == [64, 6]
    assert bv.locate_packed1(small) == [66]
