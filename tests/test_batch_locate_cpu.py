"""The planning half of BatchRangeVerifier.locate_wire (rangeproofs/batch.py locate_plan) without a GPU: a stub stands in for
group_values_wire -- built from a chosen set of proofs whose equations fail and a chosen status -- and records every call, so the
tests see the exact level-2 sub-batch as well as the located indices."""
import pytest

import bulletproofs_amd  # noqa: F401
from bulletproofs_amd.rangeproofs.batch import locate_plan

ZERO = bytes(64)
NONZERO = b"\x01" + bytes(63)


class Stub:
    """group_values over a batch of `count` proofs: `bad` = proofs whose equations fail, `status` = {index: status byte} of the
    proofs that fail byte-level checks (they contribute to no group, as on the device)."""

    def __init__(self, count, bad=(), status=None):
        self.count, self.bad, self.status = count, set(bad), dict(status or {})
        self.calls = []

    def __call__(self, indices, group):
        self.calls.append((None if indices is None else list(indices), group))
        idx = list(range(self.count)) if indices is None else list(indices)
        status = bytes(self.status.get(i, 0) for i in idx)
        values = []
        for lo in range(0, len(idx), group):
            members = [i for i in idx[lo: lo + group] if not self.status.get(i, 0)]
            values.append(NONZERO if any(i in self.bad for i in members) else ZERO)
        return values, status


CASES = [
    # count, group, bad, status, located, level-2 sub-batch (None: no level-2 call)
    (9, 4, [], {}, [], None),                                                   # all valid
    (10, 4, [], {}, [], None),
    (1, 4, [], {}, [], None),
    (1, 4, [0], {}, [0], None),                                                 # group >= batch size: one group of one proof, nothing left to split
    (9, 4, [0], {}, [0], [0, 1, 2, 3]),                                         # the first group
    (9, 4, [8], {}, [8], [8]),                                                  # the short group (9 = 4 + 4 + 1)
    (10, 4, [9], {}, [9], [8, 9]),                                              # the last group
    (10, 4, [3, 9], {}, [3, 9], [0, 1, 2, 3, 8, 9]),                            # first and last
    (9, 4, [5, 6], {}, [5, 6], [4, 5, 6, 7]),                                   # two bad proofs share one group
    (10, 4, [1, 2, 4, 8], {}, [1, 2, 4, 8], list(range(10))),                   # every group fails
    (9, 4, [], {6: 1}, [6], None),                                              # a flagged proof in an otherwise valid group: no level 2
    (9, 4, [], {8: 2}, [8], None),                                              # ... alone in the short group
    (10, 4, [1], {6: 3}, [1, 6], [0, 1, 2, 3]),                                 # no level-2 call for the flagged proof's group
    (10, 4, [5], {6: 1}, [5, 6], [4, 5, 7]),                                    # flagged beside a bad one: located at level 1, not sent again
    (9, 16, [2, 7], {}, [2, 7], list(range(9))),                                # group >= batch size
    (10, 10, [], {0: 1, 9: 2}, [0, 9], None),
    (10, 1, [4, 7], {2: 1}, [2, 4, 7], None),                                   # group = 1: level 1 is already one proof per group
]


@pytest.mark.parametrize("count,group,bad,status,located,level2", CASES)
def test_locate_plan(count, group, bad, status, located, level2):
    stub = Stub(count, bad, status)
    assert locate_plan(count, group, stub) == located
    assert stub.calls[0] == (None, min(group, count))
    if level2 is None:
        assert len(stub.calls) == 1
    else:
        assert stub.calls[1:] == [(level2, 1)]


def test_locate_plan_level_two_may_flag_as_well_as_reject():
    """A level-2 position maps back to its batch index whether its value or its status names it."""
    def group_values(indices, group):
        if indices is None:
            return [ZERO, NONZERO, NONZERO], bytes(9)
        assert indices == [4, 5, 6, 7, 8] and group == 1
        return [ZERO, NONZERO, ZERO, ZERO, ZERO], bytes([0, 0, 0, 1, 0])
    assert locate_plan(9, 4, group_values) == [5, 7]


def test_locate_plan_arguments():
    assert locate_plan(0, 4, None) == []
    with pytest.raises(ValueError):
        locate_plan(3, 0, Stub(3))
    with pytest.raises(ValueError):                      # a group_values that answers for another batch
        locate_plan(9, 4, Stub(8))
