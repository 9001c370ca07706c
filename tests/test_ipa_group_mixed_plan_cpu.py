"""The plan of bpmi_ipa_group_values_packed_mixed_dev (python-bulletproofs_amd/csrc/ipa_group_mixed_plan_host.hpp) on the CPU: the header is
plain C++, so tests/csrc_host/ipa_group_mixed_plan_main.cpp -- a stand-alone program built with the host compiler and the address and
undefined-behaviour sanitizers -- prints what the call decides before its first HIP call: the argument errors with their messages, the
groups of every class with their clamp and numbering, the padded row offsets and the class of every block of the sum kernel, the
routes of the groups' MSMs, the tables the kernels read and the regions behind the unchanged ipa_packed_mixed_plan."""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "csrc_host", "ipa_group_mixed_plan_main.cpp")
INC = os.path.join(REPO, "python-bulletproofs_amd", "csrc")
E_ARG = -3
LIGHT, MID, MSM_RUN = 1, 2, 3
WINDOWS = 255 // 7 + 1                      # windows of MID_C = 7 bits over 256-bit scalars

P2, P1 = "axltoupd", "axltoupchd"           # every required array and a seed, per protocol


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ipa_group_mixed_plan") / "ipa_group_mixed_plan_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe])

    def go(*cases):
        r = subprocess.run([exe] + list(cases), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [json.loads(line) for line in r.stdout.splitlines()]
        assert len(lines) == len(cases)
        return lines
    return go


def case(classes, K=6, protocol=2, scale=0, budget=0, present=None, n_given=-1, outputs=1, group_given=1):
    """classes: [(k, P, tr_len, group[, flags])]"""
    present = present or (P1 if protocol == 1 else P2)
    return ";".join(["%d,%d,%d,%d,%s,%d,%d,%d" % (K, protocol, scale, budget, present, n_given, outputs, group_given)] + [":".join(str(v) for v in c) for c in classes])


def per_of(k, protocol):
    return 2 * k + (4 if protocol == 1 else 2)


def route_of(pairs):
    return LIGHT if pairs <= 512 else MID if pairs <= 8448 else MSM_RUN


# (k, proofs, group): k in mixed order (the sorted order of the proofs differs from the caller's), an empty class between two others,
# two classes of one k, a clamp (500 > 64), short last groups (65 = 4 x 16 + 1, 130 = 14 x 9 + 4)
ORDER = [(1, 3, 2), (6, 65, 16), (0, 1, 1), (5, 0, 7), (3, 130, 9), (3, 64, 500)]
ASCENDING = [(0, 5, 2), (1, 3, 2), (3, 130, 9), (6, 65, 16)]


def check(p, shape, protocol):
    """Everything the plan says about the classes `shape`, against the rules of the header."""
    assert p["err"] == 0 and not p["empty"]
    first_group = block = extra = gbase = 0
    class_tab, group_tab, lists = [], [], {LIGHT: [], MID: [], MSM_RUN: []}
    tab_base = {}
    at = 0
    for c in sorted(range(len(shape)), key=lambda c: -shape[c][0]):        # the mixed plan's order: descending k, stable
        k, P, _ = shape[c]
        tab_base[c] = at
        at += P * ((1 << (k // 2)) + (1 << (k - k // 2)))
    for c, (k, P, group) in enumerate(shape):
        q = p["classes"][c]
        assert p["value_off"][c] == first_group
        if not P:
            assert q["count"] == 0 and q["ngroups"] == 0 and "single" not in q
            continue
        n, per, g = 1 << k, per_of(k, protocol), min(group, P)
        ngroups = (P + g - 1) // g
        pairs = 2 * n + g * per
        assert (q["k"], q["kl"], q["per"], q["count"], q["group"], q["ngroups"], q["first_group"]) == (k, k // 2, per, P, g, ngroups, first_group)
        assert (q["pairs"], q["route"]) == (pairs, route_of(pairs))
        assert (q["tab_base"], q["tab_stride"]) == (tab_base[c], (1 << (k // 2)) + (1 << (k - k // 2)))
        assert q["layout_ok"] == 1 and q["gbase"] == gbase and q["extra_off"] == extra
        assert q["row_off"] == 256 * block and q["block_start"] == block and q["row_off"] % 256 == 0 and q["rows"] == ngroups * n
        s = q["single"]                                                    # the single-class plan decides the same for this class alone
        assert s["err"] == 0 and (s["group"], s["ngroups"], s["per"], s["pairs"], s["route"]) == (g, ngroups, per, pairs, q["route"])
        class_tab += [block, 256 * block, k, k // 2, tab_base[c], q["tab_stride"], P, g]
        for t in range(ngroups):
            cnt = min(g, P - t * g)
            group_tab += [n, 256 * block + t * n, extra + t * g * per, cnt * per]
            lists[q["route"]].append(first_group + t)
        block += (ngroups * n + 255) // 256
        p_rows_total = 256 * q["block_start"] + ngroups * n
        first_group, extra, gbase = first_group + ngroups, extra + P * per, gbase + P
    assert p["value_off"][len(shape)] == first_group == p["ngroups"]
    assert p["n_blocks"] == block and p["rows_total"] == p_rows_total and p["W"] == WINDOWS
    assert p["class_tab"] == class_tab and p["group_tab"] == group_tab
    assert (p["light"], p["mid"], p["run"]) == (lists[LIGHT], lists[MID], lists[MSM_RUN])
    # every block of the sum kernel maps to one class, by the rule the kernel uses: the last class whose block start is <= b
    starts = class_tab[0::8]
    assert starts == sorted(set(starts)) and starts[0] == 0
    live = [c for c, (_, P, _) in enumerate(shape) if P]
    for b in range(block):
        j = max(i for i, s0 in enumerate(starts) if s0 <= b)
        q = p["classes"][live[j]]
        assert q["block_start"] <= b < q["block_start"] + (q["rows"] + 255) // 256
    # the regions: the groups' behind the unchanged packed plan, in order, on 256-byte lines, disjoint
    reg = p["regions"]
    want = {"gsa": 32 * p_rows_total, "gsb": 32 * p_rows_total, "E": 144 * WINDOWS * first_group, "vals": 64 * first_group, "class_tab": 4 * len(class_tab),
            "group_tab": 4 * len(group_tab), "light": 4 * len(lists[LIGHT]), "mid": 4 * len(lists[MID])}
    for name, nbytes in want.items():
        assert reg[name][1] == nbytes, name
    spans = sorted([(o, o + b, name) for name, (o, b) in reg.items()] + [(o, o + b, "packed." + name) for name, (o, b) in p["packed_regions"].items()])
    assert all(o % 256 == 0 for o, _, _ in spans)
    for (_, end, a), (o, _, b) in zip(spans, spans[1:]):
        assert end <= o, (a, b)
    assert spans[-1][1] <= p["total_bytes"]
    assert max(o + b for o, b in p["packed_regions"].values()) <= p["packed_total"] == reg["gsa"][0]
    order = ["gsa", "gsb", "E", "vals", "class_tab", "group_tab", "light", "mid"]
    assert [reg[name][0] for name in order] == sorted(reg[name][0] for name in order)
    # indexing: the padded rows stay far below 2^32 scalars
    assert 256 * block < (1 << 25) + (1 << 14) < 1 << 32


@pytest.mark.parametrize("protocol", [1, 2])
@pytest.mark.parametrize("scale", [0, 1])
@pytest.mark.parametrize("shape", [ORDER, ASCENDING], ids=["mixed-order", "ascending"])
def test_groups_rows_tables_and_regions(plan, shape, scale, protocol):
    (p,) = plan(case([(k, P, 40 + 170 * k, g) for k, P, g in shape], protocol=protocol, scale=scale))
    check(p, shape, protocol)


def test_the_caller_order_differs_from_the_sorted_order(plan):
    (p,) = plan(case([(k, P, 40 + 170 * k, g) for k, P, g in ORDER]))
    firsts = [p["classes"][c]["first_sorted"] for c in (0, 1, 2, 4, 5)]
    assert firsts == [65 + 194, 0, 65 + 194 + 3, 65, 65 + 130] and firsts != sorted(firsts)
    assert p["value_off"] == [0, 2, 7, 8, 8, 23, 24]                      # 3 / 2, 65 / 16, 1, none, 130 / 9, 64 / 500 -> one group


def test_a_short_last_group_and_the_clamp(plan):
    (p,) = plan(case([(3, 130, 100, 9), (3, 64, 100, 500), (3, 64, 100, 64), (3, 64, 100, 1 << 40)]))
    assert [q["group"] for q in p["classes"]] == [9, 64, 64, 64] and [q["ngroups"] for q in p["classes"]] == [15, 1, 1, 1]
    assert p["group_tab"][4 * 14: 4 * 15] == [8, 14 * 8, 14 * 9 * 8, 4 * 8]        # the short group: 4 proofs of 8 extra pairs


# k = 3: 16 generator pairs, 8 extra pairs per proof under protocol 2 and 10 under protocol 1
ROUTES = [(2, 62, LIGHT, 512), (2, 63, MID, 520), (2, 1054, MID, 8448), (2, 1055, MSM_RUN, 8456),
          (1, 49, LIGHT, 506), (1, 50, MID, 516), (1, 843, MID, 8446), (1, 844, MSM_RUN, 8456)]


@pytest.mark.parametrize("protocol,group,route,pairs", ROUTES, ids=["p%d-g%d" % (r[0], r[1]) for r in ROUTES])
def test_the_routes_on_either_side_of_both_switches(plan, protocol, group, route, pairs):
    (p,) = plan(case([(0, 2, 100, 1), (3, 1100, 100, group)], protocol=protocol))
    q = p["classes"][1]
    assert (q["group"], q["pairs"], q["route"]) == (group, pairs, route) and q["single"]["route"] == route
    assert q["pairs"] == 16 + per_of(3, protocol) * group
    mine = list(range(2, 2 + q["ngroups"]))
    assert p["light"] == [0, 1] + (mine if route == LIGHT else []) and p["mid"] == (mine if route == MID else []) and p["run"] == (mine if route == MSM_RUN else [])


def test_all_three_routes_in_one_call(plan):
    shape = [(8, 5, 2), (9, 3, 2), (3, 1100, 1055), (3, 130, 16)]
    (p,) = plan(case([(k, P, 100, g) for k, P, g in shape], K=9))
    check(p, shape, 2)
    assert [q["route"] for q in p["classes"]] == [MID, MID, MSM_RUN, LIGHT]
    assert p["mid"] == [0, 1, 2, 3, 4] and p["run"] == [5, 6] and p["light"] == list(range(7, 16))


def test_one_class_has_the_region_sizes_of_the_single_class_plan(plan):
    for k, P, g, protocol in [(6, 300, 7, 2), (3, 130, 4, 1), (0, 5, 2, 2), (10, 9, 300, 2)]:
        (p,) = plan(case([(k, P, 100, g)], K=10, protocol=protocol))
        s, reg = p["classes"][0]["single"], p["regions"]
        assert (reg["gsa"][1], reg["gsb"][1], reg["E"][1], reg["vals"][1]) == (s["b_gsa"], s["b_gsb"], s["b_E"], s["b_vals"])


def test_a_transposition_budget_changes_the_rounds_and_nothing_else(plan):
    shape = [(3, 130, 100, 4), (6, 200, 100, 16)]
    whole, small = plan(case(shape), case(shape, budget=1000))
    assert whole["rounds"] == 1 and small["rounds"] == 4                   # 64 rows per round: ceil(200 / 64)
    assert [q["prep_rows"] for q in small["classes"]] == [64, 64]
    for key in ("value_off", "class_tab", "group_tab", "light", "mid", "run", "ngroups", "n_blocks"):
        assert whole[key] == small[key]


def test_every_class_empty(plan):
    (p,) = plan(case([(3, 0, 0, 1), (6, 0, 0, 0)]))
    assert p["err"] == 0 and p["empty"] == 1 and p["value_off"] == [0, 0, 0]


ERRORS = [
    # what the mixed packed verifier refuses, with its messages
    (case([(3, 4, 100, 1)], n_given=0), "between 1 and 64 classes"),
    (case([(3, 4, 100, 1)], n_given=65), "between 1 and 64 classes"),
    (case([], n_given=2), "between 1 and 64 classes"),
    (case([(3, 4, 100, 1)], protocol=3, present=P2), "protocol must be 1 or 2"),
    (case([(3, 4, 100, 1)], K=23), "n_gens must be 2^K, K <= 22"),
    (case([(3, 4, 100, 1), (7, 4, 100, 1)]), "class 1: k must be at most K"),
    (case([(3, 4, 100, 1), (3, 4, 100, 1, "a")]), "class 1: null argument"),
    (case([(3, 4, 100, 1, "x")]), "class 0: null argument (xs and LR may be NULL only at k = 0)"),
    (case([(0, 4, 100, 1, "xl"), (3, 4, 100, 1, "C")]), "class 1: c and head must be NULL under protocol 2"),
    (case([(3, 4, 100, 1), (3, 4, 100, 1, "c")], protocol=1), "class 1: protocol 1 needs c and head"),
    (case([(3, 4, 100, 1, "S")], protocol=1), "class 0: start must be NULL under protocol 1"),
    (case([(3, 4, 100, 1)], present=P2.replace("d", "")), "class 0: weights or a 32-byte seed"),
    (case([(3, 4, 100, 1), (2, 4, 100, 1, "D")]), "class 1: tr_off must not decrease"),
    (case([(1, 65537, 10, 65537)]), "class 0: between 1 and 2^16 proofs per call"),
    (case([(1, 65536, 65537, 65536)], K=22), "class 0: at most 4 GiB of transcripts per call"),
    (case([(1, 40000, 10, 40000), (2, 30000, 10, 30000)]), "between 1 and 2^16 proofs per call"),
    (case([(1, 40000, 60000, 40000), (2, 25000, 80000, 25000)]), "at most 4 GiB of transcripts per call"),
    (case([(22, 1000, 10, 1000), (22, 100, 10, 100)], K=22), "at most 2^32 elements"),
    (case([(16, 20000, 10, 20000), (16, 20000, 10, 20000)], K=22, protocol=1), "exceed 1 GiB"),
    (case([(22, 1025, 10, 1025)], K=22), "class 0: at most 2^32 elements (proofs x n) per call"),
    # its own
    (case([(3, 4, 100, 1)], group_given=0), "null argument (group)"),
    (case([(3, 4, 100, 1), (3, 0, 0, 0), (2, 4, 100, 0)]), "class 2: group must be at least 1"),
    (case([(3, 4, 100, 1)], outputs=0), "null argument (values, value_off and status)"),
    (case([(16, 1024, 10, 1), (0, 1, 10, 1)], K=16), "n_groups x 2 n must not exceed 2^26"),
    (case([(16, 500, 10, 1), (15, 24, 10, 1), (0, 1, 10, 1)], K=16), "n_groups x 2 n must not exceed 2^26"),
    (case([(22, 16, 10, 1)], K=22), "n_groups x 2 n must not exceed 2^26"),
]


@pytest.mark.parametrize("text,want", ERRORS, ids=[("%s-%d" % (t[:28].replace(" ", "_").replace(":", ""), i)) for i, (_, t) in enumerate(ERRORS)])
def test_argument_errors_and_their_messages(plan, text, want):
    (p,) = plan(text)
    assert p["err"] == E_ARG and want in p["msg"] and "classes" not in p and "value_off" not in p


def test_the_row_cap_is_inclusive(plan):
    """The sum over the classes of n_groups x 2 n = 2^26 exactly is accepted; one scalar pair more is not (ERRORS above)."""
    p, q, r = plan(case([(16, 1024, 10, 2)], K=16), case([(16, 500, 10, 1), (15, 24, 10, 1)], K=16), case([(22, 16, 10, 2)], K=22))
    assert p["err"] == 0 and p["ngroups"] * 2 * (1 << 16) == 1 << 26
    assert q["err"] == 0 and 2 * (500 * (1 << 16) + 24 * (1 << 15)) == 1 << 26
    assert r["err"] == 0 and r["ngroups"] * 2 * (1 << 22) == 1 << 26


def test_an_empty_class_needs_no_group_size(plan):
    (p,) = plan(case([(3, 4, 100, 2), (6, 0, 0, 0), (1, 3, 100, 1)]))
    assert p["err"] == 0 and p["value_off"] == [0, 2, 2, 5]
