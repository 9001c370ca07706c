"""The Python side of the grouped packed verifier (BatchInnerProductVerifier.group_values_packed*, default_group and the two-level
locate_packed*, python-bulletproofs_amd/innerproduct/batch.py) without a GPU: how many native calls a valid and a rejected batch cost,
what level 2 holds, that group = 0 keeps the bisection over verify calls, where an oversized batch is cut, and the capacity rule of
default_group -- over an engine that records what it is handed and answers from a set of "invalid" proofs."""
import pytest

import bulletproofs_amd  # noqa: F401
from bulletproofs_amd.innerproduct import BatchInnerProductVerifier

ZERO, NONZERO = bytes(64), b"\x01" + bytes(63)


class FakeEngine:
    """The two packed calls over tagged rows: bytes 0..3 of a proof's `ab` row are its tag; a tag in `flag` gets status 1 and takes part
    in no value, one in `silent` makes the value of whatever holds it non-zero.  calls: (name, tags, group, weights)."""

    def __init__(self, flag=(), silent=()):
        self.flag, self.silent, self.calls = set(flag), set(silent), []

    def upload(self, data):
        return object()

    def _tags(self, n, protocol, count, ab, xs, lr, trs, starts, u, P, c, head, weights, seed):
        k = n.bit_length() - 1
        assert 1 <= count <= 1 << 16 and (weights is None) != (seed is None)
        assert len(ab) == 64 * count and len(xs) == 32 * k * count and len(lr) == 128 * k * count and len(trs) == count and len(P) == 64 * count
        assert len(u) == (64 if protocol == 1 else 64 * count) and len(c) == (32 * count if protocol == 1 else 0) and len(head) == (128 * count if protocol == 1 else 0)
        assert starts is None or len(starts) == count
        if weights is not None:
            assert len(weights) == 32 * (3 if protocol == 1 else 1) * count
        return [int.from_bytes(ab[64 * i: 64 * i + 4], "little") for i in range(count)]

    def ipa_verify_batch_packed_dev(self, d_g, d_h, n, protocol, count, ab, xs, lr, trs, starts, u, P, c, head, weights, seed, d_hscale):
        tags = self._tags(n, protocol, count, ab, xs, lr, trs, starts, u, P, c, head, weights, seed)
        self.calls.append(("verify", tags, None, weights))
        live = [t for t in tags if t not in self.flag]
        return (NONZERO if any(t in self.silent for t in live) else ZERO), bytes(1 if t in self.flag else 0 for t in tags)

    def ipa_group_values_packed_dev(self, d_g, d_h, n, protocol, count, ab, xs, lr, trs, starts, u, P, c, head, weights, seed, d_hscale, group):
        tags = self._tags(n, protocol, count, ab, xs, lr, trs, starts, u, P, c, head, weights, seed)
        assert group >= 1
        self.calls.append(("group", tags, group, weights))
        group = min(group, count)                                        # the native clamp
        assert (count + group - 1) // group * 2 * n <= 1 << 26
        values = []
        for lo in range(0, count, group):
            live = [t for t in tags[lo: lo + group] if t not in self.flag]
            values.append(NONZERO if any(t in self.silent for t in live) else ZERO)
        return values, bytes(1 if t in self.flag else 0 for t in tags)


def batch(protocol, k, count):
    ab = b"".join(i.to_bytes(4, "little") + bytes(60) for i in range(count))
    trs = [b"t"] * count
    if protocol == 2:
        return (bytes(64 * count), bytes(64 * count), ab, bytes(32 * k * count), bytes(128 * k * count), trs)
    return (bytes(64), bytes(64 * count), bytes(32 * count), ab, bytes(32 * k * count), bytes(128 * k * count), bytes(128 * count), trs)


def verifier(engine, k=3):
    from bulletproofs_amd.ec import Point
    n = 1 << k
    return BatchInnerProductVerifier([Point.IDENTITY_ELEMENT] * n, [Point.IDENTITY_ELEMENT] * n, engine=engine)          # the fake engine never reads them


def locate(bv, protocol):
    return bv.locate_packed2 if protocol == 2 else bv.locate_packed1


@pytest.mark.parametrize("protocol", [1, 2])
def test_a_valid_batch_costs_one_group_call(protocol):
    eng = FakeEngine()
    bv = verifier(eng)
    assert locate(bv, protocol)(*batch(protocol, 3, 130)) == []
    assert [(name, len(tags), group) for name, tags, group, _ in eng.calls] == [("group", 130, 130)]          # default_group: 1 024 | 512 at n = 8, above the batch
    assert bv.default_group(protocol) == (1024 if protocol == 2 else 512)
    eng.calls = []
    assert locate(bv, protocol)(*batch(protocol, 3, 130), group=16) == []
    assert [(name, len(tags), group) for name, tags, group, _ in eng.calls] == [("group", 130, 16)]


@pytest.mark.parametrize("protocol", [1, 2])
def test_a_rejected_batch_costs_two_and_level_2_holds_the_unflagged_proofs_of_the_failing_groups(protocol):
    eng = FakeEngine(flag={5, 17, 129}, silent={1, 3, 17, 64, 128})        # 17 is flagged AND wrong: it is located by its flag alone
    bv = verifier(eng)
    assert locate(bv, protocol)(*batch(protocol, 3, 130), group=16) == [1, 3, 5, 17, 64, 128, 129]
    assert [(name, group) for name, _, group, _ in eng.calls] == [("group", 16), ("group", 1)]
    assert eng.calls[0][1] == list(range(130))
    # groups 0 (1, 3), 4 (64) and 8 (128; the short last group) fail; group 1 does not: its only wrong proof is flagged
    assert eng.calls[1][1] == [i for i in range(16) if i != 5] + list(range(64, 80)) + [128]
    assert all(w is None for _, _, _, w in eng.calls)                     # fresh seeds, never known weights


def test_a_group_of_one_needs_no_second_level():
    eng = FakeEngine(flag={2}, silent={7})
    bv = verifier(eng)
    assert bv.locate_packed2(*batch(2, 3, 20), group=1) == [2, 7]
    assert [(name, group) for name, _, group, _ in eng.calls] == [("group", 1)]


@pytest.mark.parametrize("protocol", [1, 2])
def test_group_0_keeps_the_bisection_over_verify_calls(protocol):
    eng = FakeEngine(flag={5}, silent={1, 64})
    bv = verifier(eng)
    assert locate(bv, protocol)(*batch(protocol, 3, 130), group=0) == [1, 5, 64]
    assert len(eng.calls) > 2 and {name for name, _, _, _ in eng.calls} == {"verify"}
    with pytest.raises(ValueError):
        locate(bv, protocol)(*batch(protocol, 3, 130), group=-1)


def test_group_values_never_return_a_verdict_and_pass_the_weights_on():
    eng = FakeEngine(flag={4}, silent={9})
    bv = verifier(eng)
    values, status = bv.group_values_packed2(*batch(2, 3, 10), group=4, weights=list(range(1, 11)))
    assert values == [ZERO, ZERO, NONZERO] and status == bytes([0, 0, 0, 0, 1, 0, 0, 0, 0, 0])
    assert eng.calls[0][3] == b"".join(w.to_bytes(32, "little") for w in range(1, 11))
    values, status = bv.group_values_packed1(*batch(1, 3, 10), group=500, weights=[(1, 2, 3)] * 10)          # the clamp
    assert values == [NONZERO] and eng.calls[1][2] == 10 and len(eng.calls[1][3]) == 96 * 10
    assert bv.group_values_packed2(*batch(2, 3, 0)) == ([], b"")
    with pytest.raises(ValueError, match="group must be at least 1"):
        bv.group_values_packed2(*batch(2, 3, 10), group=0)
    with pytest.raises(ValueError, match="one weight per proof"):
        bv.group_values_packed2(*batch(2, 3, 10), weights=[1] * 9)


def test_an_oversized_batch_is_cut_at_a_multiple_of_group():
    total = (1 << 16) + 5
    eng = FakeEngine(flag={65537}, silent={70, 65539})
    bv = verifier(eng, k=1)
    rows = batch(2, 1, total)
    ws = list(range(1, total + 1))
    values, status = bv.group_values_packed2(*rows, group=48, weights=ws)
    cut = (1 << 16) // 48 * 48                                           # 65 520: the largest multiple of 48 within one call
    assert [(name, len(tags), group) for name, tags, group, _ in eng.calls] == [("group", cut, 48), ("group", total - cut, 48)]
    assert eng.calls[0][1] + eng.calls[1][1] == list(range(total))
    assert eng.calls[1][3][:32] == (cut + 1).to_bytes(32, "little")        # the weights are cut at the same index
    assert len(values) == (total + 47) // 48 and len(status) == total
    assert [t for t, v in enumerate(values) if v != ZERO] == [70 // 48, 65539 // 48] and [i for i, s in enumerate(status) if s] == [65537]
    # the whole plan over it: two calls at level 1, one at level 2; global indices
    eng.calls = []
    assert bv.locate_packed2(*rows, group=48) == [70, 65537, 65539]
    assert [(len(tags), group) for _, tags, group, _ in eng.calls] == [(cut, 48), (total - cut, 48), (48 + 20, 1)]          # 48 .. 95, and 65 520 .. 65 540 without the flagged one
    assert 65537 not in eng.calls[2][1] and eng.calls[2][1][:48] == list(range(48, 96))


def test_the_row_cap_cuts_a_call_too():
    """ceil(count / group) x 2 n <= 2^26 per call: at n = 2^20, 32 groups."""
    eng = FakeEngine()
    bv = verifier(eng, k=0)
    bv.n, bv.k = 1 << 20, 20                                             # (the fake engine checks the row sizes against n)
    count = 70
    ab = b"".join(i.to_bytes(4, "little") + bytes(60) for i in range(count))
    rows = (bytes(64 * count), bytes(64 * count), ab, bytes(32 * 20 * count), bytes(128 * 20 * count), [b"t"] * count)
    values, status = bv.group_values_packed2(*rows, group=2)
    assert [(len(tags), group) for _, tags, group, _ in eng.calls] == [(64, 2), (6, 2)] and len(values) == 35 and len(status) == 70


def test_default_group_is_the_largest_power_of_two_that_fits_the_group_kernel():
    """2 n + group x per <= 8448 pairs (MID_NMAX), per = 2 k + 2 | 2 k + 4: the capacity rule, worked out here for the shapes of the
    measurement.  n = 64 under Protocol 2: (8448 - 128) // 14 = 594 -> 512; n = 1 024: (8448 - 2048) // 22 = 290 -> 256."""
    for k, protocol, want in ((6, 2, 512), (10, 2, 256), (6, 1, 512), (10, 1, 256), (3, 2, 1024), (0, 2, 4096), (12, 2, 8), (12, 1, 8)):
        bv = verifier(FakeEngine(), k=k)
        g = bv.default_group(protocol)
        per = 2 * k + (4 if protocol == 1 else 2)
        assert g == want and g & (g - 1) == 0 and 2 * (1 << k) + g * per <= 8448 < 2 * (1 << k) + 2 * g * per, (k, protocol)
    # not even one proof fits: every group is a multi-scalar multiplication of its own, sqrt(count) balances the two levels
    bv = verifier(FakeEngine(), k=13)
    assert [bv.default_group(2, c) for c in (1, 3, 4, 1000, 1024, 1 << 16)] == [1, 1, 2, 16, 32, 256] and bv.default_group(2) == 1
