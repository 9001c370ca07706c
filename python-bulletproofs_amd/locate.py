"""Naming the invalid proofs of a rejected batch, free of any GPU: the bisection over subset probes and the two-level plan over group
values, each ONCE.  rangeproofs.batch and innerproduct.batch / batch_mixed re-export them; this module imports neither package."""

_ZERO64 = bytes(64)


def locate_by_bisection(count, subset_is_valid):
    """The sorted indices in range(count) of the invalid items, found with subset probes: subset_is_valid(indices) is True iff
    every item of the (sorted, non-empty) index list is valid.  One probe over everything; then every subset known to hold an
    invalid item is halved: the left half is probed, and the right half only when the left one was invalid (a valid left half
    proves the right one invalid).  At most 1 + 2 bad ceil(log2 count) probes."""
    if count <= 0:
        return []
    everything = list(range(count))
    if subset_is_valid(everything):
        return []
    bad, todo = [], [everything]          # todo: subsets known to hold an invalid item
    while todo:
        sub = todo.pop()
        if len(sub) == 1:
            bad.append(sub[0])
            continue
        mid = (len(sub) + 1) // 2
        left, right = sub[:mid], sub[mid:]
        if subset_is_valid(left):
            todo.append(right)
        else:
            todo.append(left)
            if not subset_is_valid(right):
                todo.append(right)
    return sorted(bad)


def locate_plan_groups(counts, groups, group_values):
    """The two levels of locate_wire / locate_packed* over a list of classes with one group size each.  counts[c]: the proofs of class
    c; groups[c] >= 1: its group size.  group_values(sel, groups) -> (values, value_off, status) is group_values_packed* over the
    sub-batch sel: None = every proof, else per class the sorted list of its local indices (possibly empty); values and status
    class-major over sel, class c's groups at values[value_off[c]: value_off[c + 1]].
    Level 1 is group_values(None, groups) over everything; level 2 -- only when some group's value is not the identity -- is ONE call
    group_values(sub, [1, ...]) over the unflagged proofs of those groups, class by class (a flagged proof is already located and
    takes part in no value; a class whose level-1 groups were single proofs is already located too and takes no part).  Returns the
    sorted GLOBAL (class-major) indices of the proofs flagged at level 1 or with a non-identity value at level 2."""
    n_classes = len(counts)
    if len(groups) != n_classes or any(g < 1 for g in groups):
        raise ValueError("one group size >= 1 per class")
    total = sum(counts)
    if total <= 0:
        return []
    gbase = [0]
    for count in counts:
        gbase.append(gbase[-1] + count)
    eff = [min(g, count) if count else 1 for g, count in zip(groups, counts)]
    want = [0]
    for g, count in zip(eff, counts):
        want.append(want[-1] + (count + g - 1) // g)
    values, value_off, status = group_values(None, list(groups))
    if len(status) != total or len(values) != want[-1] or list(value_off) != want:
        raise ValueError("group_values returned %d values (offsets %r) and %d status bytes for %d proofs in %d groups" % (len(values), list(value_off), len(status), total, want[-1]))
    bad = [i for i in range(total) if status[i]]
    sub, flat = [[] for _ in counts], []           # level 2: per class its local indices; the same proofs' global ones (base 0: one list for both, no further pass)
    for c, (g, count) in enumerate(zip(eff, counts)):
        base = gbase[c]
        for t in range(want[c + 1] - want[c]):
            if values[want[c] + t] != _ZERO64:
                hit = [i for i in range(base + t * g, base + min((t + 1) * g, count)) if not status[i]]
                if g == 1:                         # level 1 was already one proof per group
                    bad += hit
                else:
                    flat += hit
                    sub[c] += [i - base for i in hit] if base else hit
    if flat:
        values2, value_off2, status2 = group_values(sub, [1] * n_classes)
        if len(values2) != len(flat) or len(status2) != len(flat):
            raise ValueError("group_values returned %d values for a sub-batch of %d proofs" % (len(values2), len(flat)))
        bad += [i for i, v, st in zip(flat, values2, status2) if v != _ZERO64 or st]
    return sorted(bad)


def locate_plan(count, group, group_values):
    """locate_plan_groups over ONE class of `count` proofs: group_values(indices, group) -> (values, status) over the sub-batch
    `indices`.  The callback sees (None, min(group, count)) at level 1 and (the ascending list of batch indices, 1) at level 2, and no
    second call when level 1 already had one proof per group."""
    if count <= 0:
        return []
    if group < 1:
        raise ValueError("group must be at least 1")
    group = min(group, count)

    def one_class(sel, groups):
        values, status = group_values(None if sel is None else sel[0], groups[0])
        if sel is None and (len(status) != count or len(values) != (count + group - 1) // group):          # (this function's own text, as it was)
            raise ValueError("group_values returned %d values and %d status bytes for %d proofs in groups of %d" % (len(values), len(status), count, group))
        return values, [0, len(values)], status
    return locate_plan_groups([count], [group], one_class)
