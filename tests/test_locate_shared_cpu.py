"""The pieces the locate paths share, without a GPU: packed_rows_cut (python-bulletproofs_amd/innerproduct/batch.py) -- the cut of a
packed class's rows into one native call's arguments -- against slices written out literally, and the two-level plan
(python-bulletproofs_amd/locate.py) swept exhaustively: locate_plan through its one-class adapter, and locate_plan_groups over one
class beside it."""
import functools
import itertools

import pytest

import bulletproofs_amd  # noqa: F401
from bulletproofs_amd.innerproduct.batch import packed_rows_cut
from bulletproofs_amd.locate import locate_plan, locate_plan_groups

ZERO, NONZERO = bytes(64), b"\x01" * 64
COUNT = 5

# idx, the literal slice of a byte array of s bytes per row, the literal pick of a five-item list
CUTS = [
    (range(0, 0), lambda b, s: b[0:0], lambda v: []),
    (range(0, 5), lambda b, s: b[0: 5 * s], lambda v: [v[0], v[1], v[2], v[3], v[4]]),
    (range(2, 4), lambda b, s: b[2 * s: 4 * s], lambda v: [v[2], v[3]]),
    ([0], lambda b, s: b[0: s], lambda v: [v[0]]),
    ([1, 3, 4], lambda b, s: b[s: 2 * s] + b[3 * s: 4 * s] + b[4 * s: 5 * s], lambda v: [v[1], v[3], v[4]]),
]


def rows_of(protocol, k, with_starts):
    """(rows, sizes) as BatchInnerProductVerifier._packed_rows returns them for five proofs; byte j of row i of an array is unique to
    (array, i) up to its position, so a cut that takes a wrong row or a wrong array cannot match."""
    sizes = {"ab": 64, "xs": 32 * k, "lr": 128 * k, "P": 64, "c": 32 if protocol == 1 else 0, "head": 128 if protocol == 1 else 0}
    if protocol == 2:
        sizes["u"] = 64
    rows = {name: b"".join(bytes([16 * t + i]) * s for i in range(COUNT)) for t, (name, s) in enumerate(sorted(sizes.items()))}
    if protocol == 1:
        rows["u"] = b"\xee" * 64
    rows["trs"] = [b"transcript %d" % i for i in range(COUNT)]
    rows["starts"] = [10, 11, 12, 13, 14] if with_starts else None
    return rows, sizes


@pytest.mark.parametrize("protocol", [1, 2])
@pytest.mark.parametrize("k", [0, 1, 3])
@pytest.mark.parametrize("with_starts", [False, True])
def test_packed_rows_cut_against_literal_slices(protocol, k, with_starts):
    rows, sizes = rows_of(protocol, k, with_starts)
    for idx, cut, pick in CUTS:
        ab, xs, lr, trs, starts, u, P, c, head = got = packed_rows_cut(protocol, rows, sizes, idx)
        assert ab == cut(rows["ab"], 64) and xs == cut(rows["xs"], 32 * k) and lr == cut(rows["lr"], 128 * k) and P == cut(rows["P"], 64)
        assert trs == pick(rows["trs"]) and isinstance(trs, list)
        if with_starts:
            assert starts == pick([10, 11, 12, 13, 14]) and isinstance(starts, list)
        else:
            assert starts is None
        if protocol == 1:
            assert u is rows["u"] and len(u) == 64                      # the ONE shared point, whatever the cut
            assert c == cut(rows["c"], 32) and head == cut(rows["head"], 128)
        else:
            assert u == cut(rows["u"], 64) and c == b"" and head == b""
        assert len(ab) == 64 * len(idx)
        assert packed_rows_cut(protocol, rows, sizes, list(idx)) == got             # a range and the equal list: equal bytes
        assert all(isinstance(v, bytes) for v in (ab, xs, lr, u, P, c, head))


def sweep():
    """(count, group, flagged, silently invalid) for count 0 .. 7, group 1 .. 8 and every pair of disjoint subsets of range(count)."""
    for count in range(8):
        for marks in itertools.product((0, 1, 2), repeat=count):
            flagged = frozenset(i for i, m in enumerate(marks) if m == 1)
            silent = frozenset(i for i, m in enumerate(marks) if m == 2)
            for group in range(1, 9):
                yield count, group, flagged, silent


class Stub:
    """group_values of locate_plan over a batch with the given flagged and silently invalid proofs; records its arguments."""

    def __init__(self, count, flagged, silent):
        self.count, self.flagged, self.silent, self.calls = count, flagged, silent, []

    def __call__(self, indices, group):
        self.calls.append((indices if indices is None else list(indices), group))
        idx = list(range(self.count)) if indices is None else indices
        status = bytes(1 if i in self.flagged else 0 for i in idx)
        values = [NONZERO if any(i in self.silent for i in idx[t: t + group]) else ZERO for t in range(0, len(idx), group)]
        return values, status


@functools.lru_cache(maxsize=None)
def plan_runs():
    """locate_plan over the whole sweep, once for both tests: (count, group, flagged, silent, located, the stub with its calls)."""
    runs = []
    for count, group, flagged, silent in sweep():
        stub = Stub(count, flagged, silent)
        runs.append((count, group, flagged, silent, locate_plan(count, group, stub), stub))
    return runs


def test_locate_plan_exhaustively():
    for count, group, flagged, silent, located, stub in plan_runs():
        assert located == sorted(flagged | silent)
        if count == 0:
            assert stub.calls == []
            continue
        g = min(group, count)                                            # level 1 sees the CLAMPED group
        hit = [i for i in range(count) if i not in flagged and any(j in silent for j in range(i // g * g, min((i // g + 1) * g, count)))]
        if g == 1 or not hit:                                            # one proof per group already, or every value the identity
            assert stub.calls == [(None, g)]
        else:
            assert stub.calls == [(None, g), (hit, 1)]                   # ascending indices, group 1


def test_locate_plan_groups_over_one_class_is_locate_plan():
    for count, group, flagged, silent, located, one in plan_runs():
        many = Stub(count, flagged, silent)

        def group_values(sel, groups):
            assert len(groups) == 1 and (sel is None or len(sel) == 1)
            values, status = many(None if sel is None else sel[0], groups[0])
            return values, [0, len(values)], status
        assert locate_plan_groups([count], [group], group_values) == located
        assert len(many.calls) == len(one.calls)
        assert [idx for idx, _ in many.calls] == [idx for idx, _ in one.calls]          # the same proofs, call by call
