"""The Python side of the grouped values of a list of packed classes (MixedBatchInnerProductVerifier.group_values_packed* /
locate_packed*(classes, group=...), locate_plan_groups, split_mixed_group_calls; python-bulletproofs_amd/innerproduct/batch_mixed.py)
without a GPU, over an engine that records what it is handed and answers from a set of "invalid" proofs: a valid batch costs one
native call and a rejected one two, level 2 holds exactly the unflagged proofs of the failing groups, the indices are global, an
oversized batch is cut at group boundaries at every cap, and locate_packed*(classes) with no `group` still makes only verify calls."""
import pytest

import bulletproofs_amd  # noqa: F401
from bulletproofs_amd.innerproduct.batch_mixed import MixedBatchInnerProductVerifier, locate_plan_groups, split_mixed_group_calls

from test_ipa_packed_mixed_api_cpu import FakeEngine as VerifyOnlyEngine
from test_ipa_packed_mixed_api_cpu import make_class, verifier

ZERO, ONE = bytes(64), b"\x01" + bytes(63)


class GroupEngine(VerifyOnlyEngine):
    """ipa_group_values_packed_mixed_dev over tagged rows, beside the verify call of the engine it extends: a group's value is non-zero
    iff it holds an unflagged proof whose tag is in `silent`."""

    def __init__(self, flag=(), silent=()):
        VerifyOnlyEngine.__init__(self, flag, silent)
        self.group_calls = []

    def ipa_group_values_packed_mixed_dev(self, d_g, d_h, n_gens, protocol, classes, groups, weights, seed, d_hscale):
        assert (weights is None) != (seed is None) and 1 <= len(classes) <= 64 and len(groups) == len(classes)
        values, value_off, status, shapes, tags_all, rows = [], [0], b"", [], [], 0
        for (k, count, ab, xs, lr, trs, starts, u, P, c, head), group in zip(classes, groups):
            assert count >= 1 and group >= 1 and len(ab) == 64 * count and len(xs) == 32 * k * count and len(lr) == 128 * k * count and len(trs) == count
            tags = [int.from_bytes(ab[64 * i: 64 * i + 4], "little") for i in range(count)]
            g = min(group, count)
            for t in range(0, count, g):
                values.append(ONE if any(x in self.silent and x not in self.flag for x in tags[t: t + g]) else ZERO)
            value_off.append(len(values))
            status += bytes(1 if x in self.flag else 0 for x in tags)
            shapes.append((k, count, group))
            tags_all += tags
            rows += (count + g - 1) // g * 2 * (1 << k)
        assert len(tags_all) <= 1 << 16 and sum(n * (2 * k + (4 if protocol == 1 else 2)) for k, n, _ in shapes) <= 1 << 22 and rows <= 1 << 26
        if weights is not None:
            assert len(weights) == 32 * (3 if protocol == 1 else 1) * len(tags_all)
        self.group_calls.append((shapes, tags_all, weights))
        return values, value_off, status


def batch(protocol=2):
    """Classes of k = 1, 6, 0, (empty), 3, 3 with 3, 20, 1, 0, 30, 8 proofs; tags = global indices."""
    sizes, tag, classes = [(1, 3), (6, 20), (0, 1), (3, 0), (3, 30), (3, 8)], 0, []
    for k, count in sizes:
        classes.append(make_class(protocol, k, count, tag))
        tag += count
    return classes, tag


@pytest.mark.parametrize("protocol", [1, 2])
def test_group_values_reach_the_engine_class_by_class(protocol):
    eng = GroupEngine(flag={4}, silent={4, 30, 61})
    bv = verifier(eng)
    classes, total = batch(protocol)
    call = bv.group_values_packed2 if protocol == 2 else bv.group_values_packed1
    values, value_off, status = call(classes, group=[2, 8, 1, 5, 7, 100])
    assert [c[0] for c in eng.group_calls] == [[(1, 3, 2), (6, 20, 8), (0, 1, 1), (3, 30, 7), (3, 8, 100)]]          # the empty class takes no part
    assert value_off == [0, 2, 5, 6, 6, 11, 12] and len(values) == 12 and len(status) == total
    assert [t for t, v in enumerate(values) if v != ZERO] == [6 + (30 - 24) // 7, 11]                                  # 4 is flagged: it is in no value
    assert [i for i, s in enumerate(status) if s] == [4]
    values, value_off, _ = call(classes)                                                                               # one proof per group
    assert value_off == [0, 3, 23, 24, 24, 54, 62] and [t for t, v in enumerate(values) if v != ZERO] == [30, 61]
    nw = 3 if protocol == 1 else 1
    call(classes, group=4, weights=[[7] * nw if nw > 1 else 7] * total)
    assert len(eng.group_calls[-1][2]) == 32 * nw * total and eng.group_calls[-1][0][1] == (6, 20, 4)
    for bad in (0, [1, 2], [1, 1, 1, 0, 1, 1]):
        with pytest.raises(ValueError):
            call(classes, group=bad)
    assert eng.calls == []                                                                                             # never a verify call


@pytest.mark.parametrize("group", [None, 1, 4, [2, 8, 1, 5, 7, 100]])
def test_a_valid_batch_costs_one_call_and_a_rejected_one_two(group):
    classes, total = batch()
    eng = GroupEngine()
    assert verifier(eng).locate_packed2(classes, group=group) == [] and len(eng.group_calls) == 1 and eng.calls == []
    eng = GroupEngine(flag={4, 58}, silent={0, 4, 30, 31, 61})
    bv = verifier(eng)
    assert bv.locate_packed2(classes, group=group) == [0, 4, 30, 31, 58, 61]
    assert len(eng.group_calls) == (1 if group == 1 else 2) and eng.calls == []
    if group == 4:
        # level 2: exactly the unflagged proofs of the failing groups, as sub-classes in group 1 -- class 0 [0, 3): one group; class 3
        # (base 24): the group [28, 32); class 4 (base 54): the group [58, 62) without the flagged 58
        shapes, tags, _ = eng.group_calls[1]
        assert tags == [0, 1, 2, 28, 29, 30, 31, 59, 60, 61] and shapes == [(1, 3, 1), (3, 4, 1), (3, 3, 1)]
    if group is None:
        assert [g for _, _, g in eng.group_calls[0][0]] == bv.default_groups(2, [(1, 0, 0, 3), (6, 0, 0, 20), (0, 0, 0, 1), (3, 0, 0, 30), (3, 0, 0, 8)])


def test_protocol_1_locates_too():
    classes, _ = batch(1)
    eng = GroupEngine(flag={23}, silent={5, 53})
    assert verifier(eng).locate_packed1(classes, group=None) == [5, 23, 53] and len(eng.group_calls) == 2 and eng.calls == []


def test_the_default_stays_the_bisection_over_verify_calls():
    """locate_packed*(classes) with no `group`, and group=0: only verify calls, on an engine that has nothing else."""
    classes, _ = batch()
    eng = VerifyOnlyEngine(flag={4}, silent={30})
    bv = verifier(eng)
    assert not hasattr(eng, "ipa_group_values_packed_mixed_dev")
    assert bv.locate_packed2(classes) == [4, 30] and bv.locate_packed2(classes, group=0) == [4, 30] and len(eng.calls) > 2
    eng = GroupEngine(flag={4}, silent={30})
    assert verifier(eng).locate_packed2(classes) == [4, 30] and eng.group_calls == [] and eng.calls


def test_default_groups_are_the_capacity_rules_per_class():
    bv = verifier(GroupEngine(), K=14)
    prepared = [(6, None, None, 65), (3, None, None, 0), (10, None, None, 9), (13, None, None, 100), (14, None, None, 3), (0, None, None, 7)]
    # 2 n + g per <= 8448: k = 6: (8448 - 128) // 14 = 594 -> 512; k = 3: 1054 -> 1024; k = 10: (8448 - 2048) // 22 = 290 -> 256; k = 13, 14: no proof fits -> sqrt(count)
    assert bv.default_groups(2, prepared) == [512, 1024, 256, 8, 1, 4096]
    assert bv.default_groups(1, prepared) == [512, 512, 256, 8, 1, 2048]


def test_locate_plan_groups_is_pure():
    calls = []
    bad = {(0, 1), (2, 0), (2, 5)}                         # (class, local index); class 1 is empty, class 3 has one proof per group
    counts, groups = [3, 0, 7, 2], [2, 9, 3, 1]

    def gv(sel, grp):
        calls.append((sel, grp))
        sel = [list(range(n)) for n in counts] if sel is None else sel
        values, off, status = [], [0], b""
        for c, (loc, g) in enumerate(zip(sel, grp)):
            g = min(g, len(loc)) if loc else 1
            for t in range(0, len(loc), g):
                values.append(ONE if any((c, i) in bad for i in loc[t: t + g]) else ZERO)
            off.append(len(values))
            status += bytes(1 if (c, i) == (3, 1) else 0 for i in loc)
        return values, off, status
    assert locate_plan_groups(counts, groups, gv) == [1, 3, 8, 11]          # global: class 2 starts at 3, class 3 at 10
    assert calls == [(None, [2, 9, 3, 1]), ([[0, 1], [], [0, 1, 2, 3, 4, 5], []], [1, 1, 1, 1])]
    calls.clear()
    bad.clear()
    assert locate_plan_groups(counts, groups, gv) == [11] and len(calls) == 1          # the flagged proof alone: no level 2
    assert locate_plan_groups([0, 0], [1, 1], gv) == [] and len(calls) == 1
    with pytest.raises(ValueError):
        locate_plan_groups(counts, [2, 9, 0, 1], gv)
    with pytest.raises(ValueError):
        locate_plan_groups(counts, groups, lambda sel, grp: ([ZERO], [0, 1, 1, 1, 1], bytes(12)))


def test_the_cuts_fall_on_group_boundaries_at_every_cap():
    counts, pairs, ns, groups = [10, 0, 5], [14, 4, 6], [64, 2, 4], [4, 1, 2]
    one = [[(0, 0, 10), (2, 0, 5)]]
    assert split_mixed_group_calls(counts, pairs, ns, groups) == one and split_mixed_group_calls([], [], [], []) == []
    assert split_mixed_group_calls(counts, pairs, ns, groups, proofs_max=6) == [[(0, 0, 4)], [(0, 4, 8)], [(0, 8, 10), (2, 0, 4)], [(2, 4, 5)]]
    assert split_mixed_group_calls(counts, pairs, ns, groups, pairs_max=120) == [[(0, 0, 8)], [(0, 8, 10), (2, 0, 5)]]       # 2 groups x 56 pairs; then 28 + 30
    assert split_mixed_group_calls(counts, pairs, ns, groups, classes_max=1) == [[(0, 0, 10)], [(2, 0, 5)]]
    assert split_mixed_group_calls(counts, pairs, ns, groups, rows_max=2 * 128 + 8) == [[(0, 0, 8)], [(0, 8, 10), (2, 0, 5)]]  # 2 rows of 128; then 128 + 3 x 8
    for caps in ({"proofs_max": 3}, {"pairs_max": 55}, {"rows_max": 127}):                                                  # one group of class 0 fits no call
        with pytest.raises(ValueError, match="class 0"):
            split_mixed_group_calls(counts, pairs, ns, groups, **caps)
    # every cut inside a class is a multiple of its group size, and the calls cover every proof once, in order
    for caps in ({"proofs_max": 7}, {"pairs_max": 100}, {"rows_max": 300}, {"proofs_max": 5, "rows_max": 260}):
        calls = split_mixed_group_calls(counts, pairs, ns, groups, **caps)
        assert [(c, i) for call in calls for c, lo, hi in call for i in range(lo, hi)] == [(0, i) for i in range(10)] + [(2, i) for i in range(5)]
        assert all(lo % groups[c] == 0 for call in calls for c, lo, _ in call)
        for call in calls:
            assert sum(hi - lo for _, lo, hi in call) <= caps.get("proofs_max", 1 << 16)
            assert sum((hi - lo) * pairs[c] for c, lo, hi in call) <= caps.get("pairs_max", 1 << 22)
            assert sum((hi - lo + groups[c] - 1) // groups[c] * 2 * ns[c] for c, lo, hi in call) <= caps.get("rows_max", 1 << 26)


def test_an_oversized_batch_runs_as_consecutive_group_calls():
    """2^16 + 5 proofs in three classes: two calls, cut inside class 2 at a multiple of its group; values, offsets and located
    indices are global.  70 classes of one proof: two calls of 64 and 6 classes."""
    total = (1 << 16) + 5
    sizes, tag, classes = [(1, 40000), (0, 25000), (2, total - 65000)], 0, []
    for k, count in sizes:
        classes.append(make_class(2, k, count, tag))
        tag += count
    eng = GroupEngine(flag={65540}, silent={39999, 65100})
    bv = verifier(eng)
    values, value_off, status = bv.group_values_packed2(classes, group=[16, 1000, 7])
    assert [c[0] for c in eng.group_calls] == [[(1, 40000, 16), (0, 25000, 1000), (2, 532, 7)], [(2, 9, 7)]]               # 536 fit: 76 whole groups = 532
    assert value_off == [0, 2500, 2525, 2525 + 78] and len(values) == 2603 and len(status) == total
    assert [t for t, v in enumerate(values) if v != ZERO] == [39999 // 16, 2525 + 100 // 7]
    ws = list(range(1, total + 1))
    bv.group_values_packed2(classes, group=[16, 1000, 7], weights=ws)
    assert eng.group_calls[-1][2][:32] == (65000 + 532 + 1).to_bytes(32, "little")                                        # the weights are cut at the same global index
    eng.group_calls = []
    assert bv.locate_packed2(classes, group=[16, 1000, 7]) == [39999, 65100, 65540] and len(eng.group_calls) == 3          # level 1 is two calls, level 2 one
    eng = GroupEngine(flag={66}, silent={3})
    small = [make_class(1, 1, 1, t) for t in range(70)]
    assert verifier(eng).locate_packed1(small, group=5) == [3, 66] and [len(c[0]) for c in eng.group_calls] == [64, 6]
