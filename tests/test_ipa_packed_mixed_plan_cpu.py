"""The plan of a batch of packed inner-product proofs of DIFFERENT lengths (python-bulletproofs_amd/csrc/ipa_packed_mixed_plan_host.hpp) on
the CPU: the header is plain C++, so tests/csrc_host/ipa_packed_mixed_plan_main.cpp prints what bpmi_ipa_batch_prepare_mixed,
bpmi_ipa_batch_prepare_mixed_dev and bpmi_ipa_verify_batch_packed_mixed_dev decide before their first HIP call -- the argument errors with
their messages, the order of the classes' records, the regions, the rounds with their role units -- and the lines are checked here."""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "csrc_host", "ipa_packed_mixed_plan_main.cpp")
INC = os.path.join(REPO, "python-bulletproofs_amd", "csrc")
E_ARG = -3
DEFAULT = 1 << 28

P2, P1 = "axltoupd", "axltoupchd"           # every required array and a seed, per protocol


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ipa_packed_mixed_plan") / "ipa_packed_mixed_plan_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe])

    def go(*cases):
        r = subprocess.run([exe] + list(cases), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [json.loads(line) for line in r.stdout.splitlines()]
        assert len(lines) == len(cases)
        return lines
    return go


def case(classes, K=6, protocol=2, scale=0, budget=DEFAULT, present=None, n_given=-1):
    """classes: [(k, P, tr_len[, flags])]"""
    present = present or (P1 if protocol == 1 else P2)
    return ";".join(["%d,%d,%d,%d,%s,%d" % (K, protocol, scale, budget, present, n_given)] + [":".join(str(v) for v in c) for c in classes])


def pairs_of(k, protocol):
    return 2 * k + (4 if protocol == 1 else 2)


ORDER = [(1, 3), (6, 65), (0, 1), (3, 130), (3, 64)]            # k given as 1, 6, 0, 3, 3


@pytest.mark.parametrize("protocol", [1, 2])
def test_the_class_order(plan, protocol):
    """Records: descending k, stable among equal k; extra pairs and global bases: the caller's order."""
    (p,) = plan(case([(k, P, 40 + 170 * k) for k, P in ORDER], protocol=protocol))
    assert p["err"] == 0 and not p["empty"]
    total = sum(P for _, P in ORDER)
    assert p["n_proofs"] == total and p["n_top"] == 64
    assert p["perm_k"] == [6] * 65 + [3] * 194 + [1] * 3 + [0]
    rec = lambda k: 16 * k + 24
    want_sorted = {0: 65 + 194, 1: 0, 2: 65 + 194 + 3, 3: 65, 4: 65 + 130}          # class -> its first sorted position
    words, at = {}, 0
    for c in (1, 3, 4, 0, 2):                                                                   # the sorted order of the classes
        words[c] = at
        at += rec(ORDER[c][0]) * ORDER[c][1]
    assert p["rec_words"] == at
    gbase = extra = 0
    for c, (k, P) in enumerate(ORDER):
        m = p["classes"][c]
        assert (m["k"], m["n_proofs"], m["pairs"]) == (k, P, pairs_of(k, protocol))
        assert m["gbase"] == gbase and m["extra_off"] == extra
        assert m["first_sorted"] == want_sorted[c] and m["rec_off"] == words[c]
        gbase, extra = gbase + P, extra + P * pairs_of(k, protocol)
    assert p["n_extra"] == extra
    assert p["fin_cls"] == [0, 1, 2, 3, 4]
    assert p["pair_off"] == [0] + [p["classes"][c]["extra_off"] + ORDER[c][1] * pairs_of(ORDER[c][0], protocol) for c in range(5)]


def all_regions(p):
    spans = [(o, o + b, "base." + name) for name, (o, b) in p["base_regions"].items()]
    spans += [(o, o + b, name) for name, (o, b) in p["regions"].items()]
    for c, m in enumerate(p["classes"]):
        if m["n_proofs"]:
            spans += [(o, o + b, "c%d.%s" % (c, name)) for name, (o, b) in m["regions"].items()]
    return sorted(spans)


@pytest.mark.parametrize("protocol,scale,weights", [(2, 0, False), (2, 1, True), (1, 0, True), (1, 1, False)])
def test_regions_are_disjoint_on_256_byte_lines_and_inside_total_bytes(plan, protocol, scale, weights):
    present = (P1 if protocol == 1 else P2) + ("s" if protocol == 2 else "")
    if weights:
        present = present.replace("d", "w")
    (p,) = plan(case([(k, P, 40 + 170 * k) for k, P in ORDER], protocol=protocol, scale=scale, present=present))
    assert p["err"] == 0
    spans = all_regions(p)
    assert all(o % 256 == 0 for o, _, _ in spans)
    for (_, end, a), (o, _, b) in zip(spans, spans[1:]):
        assert end <= o, (a, b)
    assert spans[-1][1] <= p["total_bytes"]
    assert max(e for _, e, name in spans if name.startswith("base.")) <= p["base_total"] <= min(o for o, _, name in spans if not name.startswith("base."))
    nw = 3 if protocol == 1 else 1
    for c, (k, P) in enumerate(ORDER):
        reg = p["classes"][c]["regions"]
        want = {"ab": 64 * P, "xs": 32 * k * P, "lr": 128 * k * P, "tr": (40 + 170 * k) * P + 8, "troff": 8 * (P + 1), "start": 4 * P if protocol == 2 else 0,
                "u": 64 if protocol == 1 else 64 * P, "P": 64 * P, "c": 32 * P if protocol == 1 else 0, "head": 128 * P if protocol == 1 else 0,
                "w": 32 * nw * P if weights else 0, "roles": 4 * P}
        for name, nbytes in want.items():
            assert reg[name][1] == nbytes, (c, name)
    assert p["regions"]["status"][1] == sum(P for _, P in ORDER)
    assert p["regions"]["unit_table"][1] == 256 * len(p["units"]) and p["regions"]["fin"][1] == 256 * 5 and p["regions"]["pairoff"][1] == 4 * 6


GRID = [(k, P) for k in (0, 1, 6, 10, 22) for P in ((1, 64, 300) if k < 22 else (1, 5))]


@pytest.mark.parametrize("protocol", [1, 2])
def test_one_class_is_ipa_packed_plan_up_to_the_base_offset(plan, protocol):
    """The upload regions, the status and T -- offsets relative to the end of the embedded plan -- the record and extra layout."""
    lines = plan(*[case([(k, P, 3 + 169 * k + 7)], K=22, protocol=protocol, scale=1) for k, P in GRID])
    for (k, P), p in zip(GRID, lines):
        assert p["err"] == 0, (k, P, p["msg"])
        m = p["classes"][0]
        s = m["single"]
        assert (m["pairs"], m["W"], m["rows"], m["chunks"]) == (s["pairs"], s["W"], s["rows"], 1)
        assert (m["rec_off"], m["extra_off"], m["gbase"], m["first_sorted"]) == (0, 0, 0, 0)
        assert p["rec_words"] == s["rec_words"] * P and p["n_extra"] == s["pairs"] * P
        mine = dict(m["regions"], status=p["regions"]["status"])
        for name, (o, b) in s["regions"].items():
            assert (mine[name][0] - p["base_total"], mine[name][1]) == (o - s["base_total"], b), (k, P, name)
        assert p["regions"]["unit_table"][0] - p["base_total"] == s["total_bytes"] - s["base_total"]
        assert p["units"] == [[0, 0, 0]] and p["rounds"] == [[0, 1, 4 * ((P + 63) // 64), k * 9 * 64 * 4]]


def check_rounds(p, classes, budget):
    """Every proof of every class lies in exactly one (round, unit, lane); the unit firsts ascend from 0; LDS of the round's largest k."""
    seen = {c: [0] * P for c, (k, P, _) in enumerate(classes) if P}
    for first_unit, n_units, blocks, lds in p["rounds"]:
        units = p["units"][first_unit: first_unit + n_units]
        assert n_units >= 1 and units[0][2] == 0
        assert [u[0] for u in units] == sorted(u[0] for u in units)
        t_bytes, k_max = 0, 0
        for i, (c, chunk, first_block) in enumerate(units):
            m = p["classes"][c]
            lo = chunk * m["rows"]
            cnt = min(m["rows"], m["n_proofs"] - lo)
            assert cnt >= 1
            nblocks = 4 * ((cnt + 63) // 64)
            nxt = units[i + 1][2] if i + 1 < len(units) else blocks
            assert nxt - first_block == nblocks                         # the blocks of a unit: up to the next unit's first
            for blk in range(nblocks):
                if blk % 4 == 0:                                        # role 0's blocks name the proofs once
                    for lane in range(64):
                        g = (blk // 4) * 64 + lane
                        if g < cnt:
                            seen[c][lo + g] += 1
            t_bytes += 8 * m["W"] * cnt
            assert 8 * m["W"] * cnt <= m["regions"]["T"][1]
            k_max = max(k_max, m["k"])
        assert lds == k_max * 9 * 64 * 4
        assert t_bytes <= budget
    assert all(v == [1] * len(v) for v in seen.values())


def test_rounds_under_a_small_budget(plan):
    classes = [(1, 3, 210), (6, 300, 1060), (0, 0, 0), (3, 130, 550), (3, 64, 550), (2, 1000, 380)]
    live = 5
    W = lambda t: (t + 7) // 8 + 16
    budget = live * 64 * 8 * W(1060) + 5000          # every class's share holds 64 rows of the widest class, and a little more
    (p,) = plan(case(classes, budget=budget))
    assert p["err"] == 0 and p["fin_cls"] == [0, 1, 3, 4, 5]
    share = budget // live
    for c, (k, P, t) in enumerate(classes):
        m = p["classes"][c]
        if not P:
            assert m["n_proofs"] == 0 and m["rows"] == 0
            continue
        rows = min(P, max(64, share // (8 * W(t)) // 64 * 64))
        assert (m["W"], m["rows"], m["chunks"]) == (W(t), rows, -(-P // rows))
        assert rows == P or rows % 64 == 0
    assert len(p["rounds"]) == max(m["chunks"] for m in p["classes"]) >= 3
    assert len({p["classes"][c]["chunks"] for c in (0, 1, 3, 4, 5)}) >= 3                     # classes run out at different rounds
    assert all(len([u for u in p["units"] if u[0] == c]) == p["classes"][c]["chunks"] for c in (0, 1, 3, 4, 5))
    check_rounds(p, classes, budget)
    # the default budget: one round, one unit per non-empty class
    (q,) = plan(case(classes))
    assert len(q["rounds"]) == 1 and [u[:2] for u in q["units"]] == [[c, 0] for c in (0, 1, 3, 4, 5)]
    check_rounds(q, classes, DEFAULT)
    # a share below 64 rows: whole waves all the same
    (r,) = plan(case(classes, budget=1000))
    assert all(m["rows"] == min(64, m["n_proofs"]) for m in r["classes"] if m["n_proofs"])


def test_empty_classes_are_skipped(plan):
    p, e = plan(case([(9, 0, 0, "axltoup"), (2, 5, 400), (23, 0, 0), (2, 0, 0)]), case([(3, 0, 0), (4, 0, 0)]))
    assert p["err"] == 0 and p["fin_cls"] == [1] and p["n_proofs"] == 5 and p["n_top"] == 4
    assert p["classes"][1]["gbase"] == 0 and p["pair_off"] == [0, 30]
    assert e["err"] == 0 and e["empty"] == 1


ERRORS = [
    (case([(3, 4, 100)], n_given=0), "between 1 and 64 classes"),
    (case([(3, 4, 100)], n_given=65), "between 1 and 64 classes"),
    (case([], n_given=2), "between 1 and 64 classes"),
    (case([(3, 4, 100)], protocol=3, present=P2), "protocol must be 1 or 2"),
    (case([(3, 4, 100)], K=23), "n_gens must be 2^K, K <= 22"),
    (case([(3, 4, 100), (7, 4, 100)]), "class 1: k must be at most K"),
    (case([(3, 4, 100), (3, 4, 100, "a")]), "class 1: null argument"),
    (case([(3, 4, 100, "x")]), "class 0: null argument (xs and LR may be NULL only at k = 0)"),
    (case([(0, 4, 100, "xl"), (3, 4, 100, "C")]), "class 1: c and head must be NULL under protocol 2"),
    (case([(3, 4, 100), (3, 4, 100, "c")], protocol=1), "class 1: protocol 1 needs c and head"),
    (case([(3, 4, 100, "S")], protocol=1), "class 0: start must be NULL under protocol 1"),
    (case([(3, 4, 100)], present=P2.replace("d", "")), "class 0: weights or a 32-byte seed"),
    (case([(3, 4, 100), (2, 4, 100, "D")]), "class 1: tr_off must not decrease"),
    (case([(1, 65537, 10)]), "class 0: between 1 and 2^16 proofs per call"),
    (case([(1, 65536, 65537)], K=22), "class 0: at most 4 GiB of transcripts per call"),
    (case([(1, 40000, 10), (2, 30000, 10)]), "between 1 and 2^16 proofs per call"),
    (case([(1, 40000, 60000), (2, 25000, 80000)]), "at most 4 GiB of transcripts per call"),
    (case([(22, 1000, 10), (22, 100, 10)], K=22), "at most 2^32 elements"),
    (case([(16, 20000, 10), (16, 20000, 10)], K=22, protocol=1), "exceed 1 GiB"),
    (case([(22, 1025, 10)], K=22), "class 0: at most 2^32 elements (proofs x n) per call"),
]


@pytest.mark.parametrize("text,want", ERRORS, ids=[("%s-%d" % (t[:28].replace(" ", "_").replace(":", ""), i)) for i, (_, t) in enumerate(ERRORS)])
def test_argument_errors_and_their_messages(plan, text, want):
    (p,) = plan(text)
    assert p["err"] == E_ARG and want in p["msg"] and "classes" not in p


def test_the_extra_pair_bound_is_the_calls(plan):
    """2^16 proofs bring at most 2^16 x 48 pairs: no call inside the proof bound reaches 2^22 extra pairs (the check is the embedded
    plan's all the same); the largest call inside the bounds plans."""
    assert (1 << 16) * (2 * 22 + 4) < 1 << 22
    (p,) = plan(case([(0, 30000, 5), (1, 35536, 5)], K=1))
    assert p["err"] == 0 and p["n_extra"] == 30000 * 2 + 35536 * 4
