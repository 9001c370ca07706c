"""The plan of bpmi_rp_batch_group_values_mixed_dev (python-bulletproofs_amd/csrc/rp_group_mixed_plan_host.hpp) on the CPU: the header is
plain C++, so tests/csrc_host/rp_group_mixed_plan_main.cpp prints what the call decides before its first HIP call -- the argument errors
with their messages, every class's group shape and route, value_off, the generator copies, every region behind the mixed plan's, the
group table and the three lists -- and the line is checked here.  The program runs under AddressSanitizer and UBSan."""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "csrc_host", "rp_group_mixed_plan_main.cpp")
INC = os.path.join(REPO, "python-bulletproofs_amd", "csrc")
E_ARG = -3
ALL = "cdogr"        # classes, a seed, d_gens / d_points / d_scalars, group, values / value_off / status
LIGHT, MID, MSM_RUN = 1, 2, 3
DIRECT = 0xFFFFFFFF
DECODE_BESIDE, DECODE_FIRST = 0, 1


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("rp_group_mixed_plan") / "rp_group_mixed_plan_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", path])
    return path


@pytest.fixture(scope="module")
def plan(exe):
    def go(classes, groups=None, n_gens_max=128, present=ALL, rp_overlap=1):
        groups = [1] * len(classes) if groups is None else groups
        args = [rp_overlap, n_gens_max, present or "-"] + ["%d:%d:%d:%d:%s" % (n, m, P, g, have) for (n, m, P, have), g in zip(classes, groups)]
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        return json.loads(r.stdout)
    return go


def k_of(n):
    return n.bit_length() - 1


def pairs_of(n, m, g):
    return 3 + 2 * n + g * (m + 6 + 2 * k_of(n))


def route_of(pairs):
    return LIGHT if pairs <= 512 else (MID if pairs <= 8448 else MSM_RUN)


# (n_gens, values_per_proof, n_proofs, what is present)
MIX = [(2, 1, 1, "bov"), (8, 1, 3, "bov"), (8, 2, 65, "bov"), (16, 4, 2, "bov"), (128, 2, 7, "bov")]
GROUPS = [1, 2, 8, 5, 3]


@pytest.fixture(scope="module")
def mix(plan):
    p = plan(MIX, GROUPS)
    assert p["err"] == 0 and p["msg"] == ""
    return p


def test_value_off_clamping_and_the_short_last_group(mix):
    assert [c["group"] for c in mix["classes"]] == [1, 2, 8, 2, 3]                 # group 5 on 2 proofs: one group of 2
    assert [c["ngroups"] for c in mix["classes"]] == [1, 2, 9, 1, 3]               # 65 / 8: 9 groups, the last of 1
    assert mix["value_off"] == [0, 1, 3, 12, 13, 16] and mix["ngroups"] == 16
    assert [c["first_group"] for c in mix["classes"]] == mix["value_off"][:-1]
    assert mix["W"] == 255 // 7 + 1
    rows = [mix["group_tab"][8 * t: 8 * t + 8] for t in range(mix["ngroups"])]
    assert rows[11][4] == 1 * 2 and rows[11][6] == 1 * (6 + 2 * 3) and rows[10][4] == 8 * 2          # the last group of class 2 holds one proof
    assert mix["pin_bytes"] >= 64 * 16 + mix["n_proofs"] and mix["n_proofs"] == 78


def test_every_group_table_row(mix):
    assert len(mix["group_tab"]) == 8 * mix["ngroups"]
    t = 0
    for (n, m, P, _), c in zip(MIX, mix["classes"]):
        per, g = 6 + 2 * k_of(n), c["group"]
        assert (c["n"], c["m"], c["per"], c["count"]) == (n, m, per, P)
        assert c["pairs"] == pairs_of(n, m, g) and c["route"] == route_of(c["pairs"])
        assert c["gfin_word"] == (c["gfin"][0] - mix["gfin_base"]) // 4 and (c["gfin"][0] - mix["gfin_base"]) % 4 == 0
        for j in range(c["ngroups"]):
            cnt = min(g, P - j * g)
            want = [c["gens_off"], 3 + 2 * n, c["gfin_word"] + 8 * (3 + 2 * n) * j, c["pair_off"] + m * j * g, cnt * m, c["pair_off"] + c["nv"] + per * j * g, cnt * per, 0]
            assert mix["group_tab"][8 * t: 8 * t + 8] == want, (t, want)
            t += 1
    assert t == mix["ngroups"]
    # every group is in exactly one list, in order, by its class's route
    lists = {LIGHT: mix["light"], MID: mix["mid"], MSM_RUN: mix["run"]}
    for r in lists:
        assert lists[r] == [c["first_group"] + j for c in mix["classes"] if c["route"] == r for j in range(c["ngroups"])]
    assert sorted(mix["light"] + mix["mid"] + mix["run"]) == list(range(mix["ngroups"]))
    assert mix["run"] == [] and mix["mid"] == []                                                # the largest: 3 + 256 + 3 x 22 = 325 pairs


def test_one_generator_copy_per_distinct_shorter_prefix_and_none_for_the_longest(mix):
    assert [k["n"] for k in mix["copies"]] == [2, 8, 16]                                        # two classes share n = 8; n = 128 = N has none
    for k in mix["copies"]:
        assert k["at"][1] == 64 * (3 + 2 * k["n"]) and k["pts_off"] == (k["at"][0] - mix["copies_base"]) // 64
    by_n = {k["n"]: k["pts_off"] for k in mix["copies"]}
    assert [c["gens_off"] for c in mix["classes"]] == [by_n[2], by_n[8], by_n[8], by_n[16], DIRECT]
    assert mix["copies_base"] == mix["copies"][0]["at"][0] and by_n[2] == 0


def test_regions_are_disjoint_on_256_byte_lines_behind_the_mixed_plan(mix):
    spans = []
    for i, c in enumerate(mix["classes"]):
        n = c["n"]
        assert c["gsum"][1] == 32 * (5 + 2 * n) * c["ngroups"] and c["gfin"][1] == 32 * (3 + 2 * n) * c["ngroups"] and c["ptflag"][1] == c["count"]
        spans += [(c[key][0], c[key][0] + c[key][1], "%s %d" % (key, i)) for key in ("gsum", "gfin", "ptflag")]
        assert c["o_verdict"] == mix["verdict"][0] + c["first"]                                 # slices of ONE region, by global index
    spans += [(k["at"][0], k["at"][0] + k["at"][1], "copy %d" % k["n"]) for k in mix["copies"]]
    spans += [(mix[key][0], mix[key][0] + mix[key][1], key) for key in ("verdict", "E", "vals", "gtab", "light_list", "mid_list") if mix[key][1]]
    assert mix["verdict"][1] == mix["n_proofs"] and mix["E"][1] == 144 * mix["W"] * mix["ngroups"] and mix["vals"][1] >= 64 * mix["ngroups"]
    assert mix["gtab"][1] == 4 * len(mix["group_tab"]) and mix["light_list"][1] == 4 * len(mix["light"]) and mix["mid_list"][1] == 4 * len(mix["mid"])
    spans.sort()
    assert all(o % 256 == 0 for o, _, _ in spans)
    assert all(e > o for o, e, _ in spans)
    for (_, end, a), (o, _, b) in zip(spans, spans[1:]):
        assert end <= o, (a, b)
    assert spans[0][0] >= mix["mixed_need"] > 0 and spans[-1][1] <= mix["need"]
    # the table and the two lists follow each other: one upload
    assert mix["gtab"][0] < mix["light_list"][0] <= mix["mid_list"][0] and mix["mid_list"][0] + mix["mid_list"][1] == mix["need"]
    assert mix["gfin_base"] == mix["classes"][0]["gfin"][0]


def test_routes_at_the_boundaries(exe, plan):
    """pairs <= 512: light; <= 8 448: mid; beyond: msm_run.  No class of range proofs has a full group of exactly 512 pairs
    (3 + 2 n + group (m + 6 + 2k) = 512 has no solution with m dividing n = 2^k), so the rule is asked directly as well."""
    for pairs, want in ((512, LIGHT), (513, MID), (8448, MID), (8449, MSM_RUN)):
        r = subprocess.run([exe, "route", str(pairs)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and json.loads(r.stdout)["route"] == want, pairs
    # through classes: (8, 1) x 38 = 513; (4, 1) x 767 = 8 448; (2, 1) x 938 = 8 449; the nearest light one, (8, 1) x 37 = 500
    assert pairs_of(8, 1, 38) == 513 and pairs_of(4, 1, 767) == 8448 and pairs_of(2, 1, 938) == 8449 and pairs_of(8, 1, 37) == 500
    p = plan([(8, 1, 40, "bov"), (8, 1, 40, "bov"), (4, 1, 800, "bov"), (2, 1, 1000, "bov"), (4, 1, 800, "bov")], [37, 38, 767, 938, 768], n_gens_max=8)
    assert p["err"] == 0
    assert [c["pairs"] for c in p["classes"]] == [500, 513, 8448, 8449, 8459]
    assert [c["route"] for c in p["classes"]] == [LIGHT, MID, MID, MSM_RUN, MSM_RUN]
    assert p["light"] == [0, 1] and p["mid"] == [2, 3, 4, 5] and p["run"] == [6, 7, 8, 9]
    assert [c["gens_off"] == DIRECT for c in p["classes"]] == [True, True, False, False, False]
    assert [k["n"] for k in p["copies"]] == [4, 2]


def test_decoding_in_front_of_the_rounds_without_overlap(plan):
    assert [c["decode"] for c in plan(MIX, GROUPS)["classes"]] == [DECODE_BESIDE] * 5
    assert [c["decode"] for c in plan(MIX, GROUPS, rp_overlap=0)["classes"]] == [DECODE_FIRST] * 5


OK1 = (8, 1, 3, "bov")
ERRORS = [
    (dict(classes=[OK1], present="cdog"), "null argument (values, value_off and status)"),
    (dict(classes=[OK1], present="cdor"), "null argument (group)"),
    (dict(classes=[OK1], present="dogr"), "null argument"),
    (dict(classes=[OK1], present="cogr"), "null argument"),                      # neither weights nor a seed
    (dict(classes=[OK1], present="cdgr"), "null argument"),                      # d_gens, d_points or d_scalars
    (dict(classes=[]), "n_classes must be in [1, 64]"),
    (dict(classes=[OK1] * 65), "n_classes must be in [1, 64]"),
    (dict(classes=[OK1, (8, 1, 3, "ov")]), "class 1: null argument"),
    (dict(classes=[OK1, (8, 1, 3, "bv")]), "class 1: null argument"),
    (dict(classes=[OK1, (8, 1, 3, "bo")]), "class 1: null argument"),
    (dict(classes=[OK1, OK1, (12, 1, 3, "bov")]), "class 2: n_gens must be a power of two in [2, 65536]"),
    (dict(classes=[(8, 3, 3, "bov"), OK1]), "class 0: values_per_proof must divide n_gens"),
    (dict(classes=[OK1, (8, 1, 0, "bov")]), "class 1: n_proofs must be in [1, 2^22]"),             # an empty class
    (dict(classes=[OK1, (8, 1, (1 << 22) + 1, "bov")]), "class 1: n_proofs must be in [1, 2^22]"),
    (dict(classes=[OK1, (256, 1, 3, "bov")]), "class 1: n_gens exceeds n_gens_max"),
    (dict(classes=[OK1], n_gens_max=1), "n_gens_max must be in [2, 65536]"),
    (dict(classes=[OK1], n_gens_max=65537), "n_gens_max must be in [2, 65536]"),
    (dict(classes=[(2, 1, 932064, "bov"), (4, 1, 2, "bov")], n_gens_max=4), "at most 2^23 points in the batch's MSM"),
    (dict(classes=[OK1, OK1, OK1], groups=[1, 4, 0]), "class 2: group must be at least 1"),
    (dict(classes=[OK1, (65536, 1, 512, "bov")], groups=[3, 1], n_gens_max=65536), "too many groups: the sum over the classes of n_groups x (3 + 2 n_gens) must not exceed 2^26"),
]


@pytest.mark.parametrize("case,text", ERRORS, ids=["%s-%d" % (t[:28].replace(" ", "_"), i) for i, (_, t) in enumerate(ERRORS)])
def test_argument_errors_their_messages_and_nothing_else_set(plan, case, text):
    p = plan(**case)
    assert p["err"] == E_ARG and p["msg"] == text
    for key in ("ngroups", "W", "need", "pin_bytes", "gfin_base", "copies_base", "mixed_need", "mixed_n_classes", "n_proofs"):
        assert p[key] == 0, key
    for key in ("verdict", "E", "vals", "gtab", "light_list", "mid_list"):
        assert p[key] == [0, 0], key
    for key in ("group_tab", "light", "mid", "run", "value_off", "copies", "classes"):
        assert p[key] == [], key


def test_the_cap_of_2_26_scalars_is_hit_by_counts_alone(plan):
    """sum_c ngroups_c (3 + 2 n_c) <= 2^26.  n = 65 536: a group brings 131 075 scalars; 511 of them and one (8, 1) group of 19 stay below,
    512 are above -- and the same 512 proofs in groups of two (256 groups) fit: the cap counts groups, not proofs."""
    assert 511 * 131075 + 19 <= 1 << 26 < 512 * 131075
    big = (65536, 1, 512, "bov")
    p = plan([OK1, (65536, 1, 511, "bov")], [3, 1], n_gens_max=65536)
    assert p["err"] == 0 and p["ngroups"] == 512 and p["classes"][1]["route"] == MSM_RUN and p["run"] == list(range(1, 512))
    assert plan([OK1, big], [3, 1], n_gens_max=65536)["err"] == E_ARG
    p = plan([OK1, big], [3, 2], n_gens_max=65536)
    assert p["err"] == 0 and p["value_off"] == [0, 1, 257]
    assert max(p["group_tab"][2::8]) == p["classes"][1]["gfin_word"] + 8 * 131075 * 255 < 1 << 32          # the gfin word offsets fit 32 bits
