"""locate_by_bisection (python-bulletproofs_amd/innerproduct/batch.py): the search BatchInnerProductVerifier.locate runs over subset
probes, as a pure function -- exactly the invalid set comes back, within 1 + 2 bad ceil(log2 count) probes."""
import pytest

import bulletproofs_amd  # noqa: F401
from bulletproofs_amd.innerproduct.batch import locate_by_bisection

COUNTS = [0, 1, 2, 7, 64]


def bad_sets(count):
    if count == 0:
        return [set()]
    sets = [set(), {0}, {count - 1}, {count // 2}, set(range(count))]
    if count >= 2:
        sets += [{count // 2 - 1, count // 2}, {0, 1}, {count - 2, count - 1}]
    if count >= 7:
        sets += [{0, count - 1}, {1, 3, 4}]
    return sets


CASES = [(count, tuple(sorted(bad))) for count in COUNTS for bad in {frozenset(s) for s in bad_sets(count)}]


@pytest.mark.parametrize("count,bad", sorted(CASES))
def test_exactly_the_bad_set_within_the_probe_bound(count, bad):
    probes = []

    def subset_is_valid(indices):
        assert indices and list(indices) == sorted(set(indices)) and 0 <= indices[0] and indices[-1] < count
        probes.append(list(indices))
        return not any(i in bad for i in indices)

    assert locate_by_bisection(count, subset_is_valid) == list(bad)
    log2 = (count - 1).bit_length() if count else 0              # ceil(log2 count)
    assert len(probes) <= 1 + 2 * len(bad) * log2
    if count:
        assert probes[0] == list(range(count))                   # the first probe is the whole batch: a valid one costs one call
    else:
        assert probes == []
    if not bad:
        assert len(probes) == min(count, 1)
