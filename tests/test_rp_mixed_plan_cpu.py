"""The plan of a mixed batch of range proofs (python-bulletproofs_amd/csrc/rp_mixed_plan_host.hpp) on the CPU: the header is plain C++, so
tests/csrc_host/rp_mixed_plan_main.cpp prints what bpmi_rp_batch_verify_mixed_dev decides before its first HIP call -- the argument errors
with their messages, every class's regions inside the two device buffers, the global first indices, the blocks of the point / scalar arrays
and the rounds of the fused launches -- and the line is checked here.  The program runs under AddressSanitizer and UBSan."""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "csrc_host", "rp_mixed_plan_main.cpp")
INC = os.path.join(REPO, "python-bulletproofs_amd", "csrc")
E_ARG = -3
ALL = "cdo"          # classes, a seed, the other pointers


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rp_mixed_plan") / "rp_mixed_plan_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe])

    def go(classes, n_gens_max=128, present=ALL, rp_rows=0, n_classes=-1):
        args = [rp_rows, n_gens_max, present or "-", n_classes] + ["%d:%d:%d:%d:%s" % c for c in classes]
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        return json.loads(r.stdout)
    return go


def k_of(n):
    return n.bit_length() - 1


# (n_gens, values_per_proof, n_proofs, proof length, what is present)
MIX = [(2, 1, 1, 700, "bov"), (8, 1, 3, 900, "bov"), (8, 2, 65, 901, "bov"), (16, 4, 2, 1100, "bov"), (128, 2, 7, 1900, "bov")]


def test_regions_are_disjoint_on_256_byte_lines_and_indices_are_running_sums(plan):
    for present in ("cdo", "cwo"):
        p = plan(MIX, present=present)
        assert p["err"] == 0 and p["msg"] == "" and p["n_classes"] == len(MIX) and p["N"] == 128
        first = pairs = nv = 0
        for (n, m, P, _, _), c in zip(MIX, p["classes"]):
            assert c["first"] == first and c["pair_off"] == pairs and c["v_off"] == nv            # running sums; blocks back to back
            assert c["nv"] == P * m and c["npts"] == P * (6 + 2 * k_of(n)) and c["k"] == k_of(n) and c["m"] == m and c["P"] == P
            first, pairs, nv = first + P, pairs + P * (m + 6 + 2 * k_of(n)), nv + P * m
        assert p["n_proofs"] == first and p["n_pairs"] == pairs and p["n_v"] == nv
        for key, extra, total in (("in", ["vstage"], "stage_bytes"), ("buf", ["merged", "bad", "units"], "need")):
            spans = sorted([(c[key][0], c[key][0] + c[key][1], "class %d" % i) for i, c in enumerate(p["classes"])] + [(p[e][0], p[e][0] + p[e][1], e) for e in extra])
            assert all(o % 256 == 0 for o, _, _ in spans), key
            assert all(e > o for o, e, _ in spans), key                     # no empty region here
            for (_, end, a), (o, _, b) in zip(spans, spans[1:]):
                assert end <= o, (key, a, b)
            assert spans[-1][1] <= p[total]
        assert p["merged"][1] == 32 * (3 + 2 * 128) and p["bad"][1] == 8 and p["units"][1] == p["unit_stride"] * len(MIX)
        assert p["pin_bytes"] >= 64
    # explicit weights take room in every class's staging region
    assert plan(MIX, present="cwo")["stage_bytes"] > plan(MIX, present="cdo")["stage_bytes"]


def test_one_round_without_rp_rows_and_its_lds_is_the_largest_class(plan):
    p = plan(MIX)
    assert [len(r["units"]) for r in p["rounds"]] == [len(MIX)]
    assert p["rounds"][0]["units"] == [[c, 0] for c in range(len(MIX))]
    assert p["rounds"][0]["lds"] == max(c["lds"] for c in p["classes"]) == (7 + 1) * 9 * 64 * 4


ROUND_CLASSES = [(8, 1, 1, 900, "bov"), (8, 2, 5, 901, "bov"), (16, 4, 6, 1100, "bov"), (2, 1, 11, 700, "bov")]


@pytest.mark.parametrize("rows", [1, 5])
def test_rounds_hold_the_rth_row_chunk_of_every_class_that_has_one(plan, rows):
    """Classes of 1, 5, 6 and 11 proofs.  Round r holds the r-th chunk of `rows` proofs of every class with more than r * rows proofs, so
    the rounds' sizes follow from the definition: rows = 1 gives 4, then 3 while the class of 5 lasts (rounds 1 .. 4), 2 in round 5, then
    1 up to round 10; rows = 5 gives 4, 2, 1."""
    p = plan(ROUND_CLASSES, rp_rows=rows)
    assert p["err"] == 0
    counts = [c[2] for c in ROUND_CLASSES]
    chunks = [-(-P // rows) for P in counts]
    assert [c["chunks"] for c in p["classes"]] == chunks and all(c["rows"] == min(rows, P) for c, P in zip(p["classes"], counts))
    want = [sum(1 for n in chunks if n > r) for r in range(max(chunks))]
    assert [len(r["units"]) for r in p["rounds"]] == want
    assert want == ([4, 3, 3, 3, 3, 2, 1, 1, 1, 1, 1] if rows == 1 else [4, 2, 1])
    seen = [tuple(u) for r in p["rounds"] for u in r["units"]]
    assert sorted(seen) == sorted((c, j) for c, n in enumerate(chunks) for j in range(n)) and len(set(seen)) == len(seen)      # every (class, chunk) exactly once
    for r, rd in enumerate(p["rounds"]):
        assert all(chunk == r for _, chunk in rd["units"]) and [c for c, _ in rd["units"]] == sorted(c for c, _ in rd["units"])
        assert rd["lds"] == max(p["classes"][c]["lds"] for c, _ in rd["units"])
    assert p["n_units"] == sum(chunks) and p["units"][1] == p["unit_stride"] * sum(chunks)


OK1 = (8, 1, 3, 900, "bov")
ERRORS = [
    (dict(classes=[OK1], present="do"), "null argument"),
    (dict(classes=[OK1], present="co"), "null argument"),                      # neither weights nor a seed
    (dict(classes=[OK1], present="cd"), "null argument"),                      # d_gens, d_points, d_scalars, out or first_bad
    (dict(classes=[OK1], n_classes=0), "n_classes must be in [1, 64]"),
    (dict(classes=[OK1], n_classes=65), "n_classes must be in [1, 64]"),
    (dict(classes=[OK1, (8, 1, 3, 900, "ov")]), "class 1: null argument"),
    (dict(classes=[OK1, (8, 1, 3, 900, "bv")]), "class 1: null argument"),
    (dict(classes=[OK1, (8, 1, 3, 900, "bo")]), "class 1: null argument"),
    (dict(classes=[OK1, OK1, (12, 1, 3, 900, "bov")]), "class 2: n_gens must be a power of two in [2, 65536]"),
    (dict(classes=[(8, 3, 3, 900, "bov"), OK1]), "class 0: values_per_proof must divide n_gens"),
    (dict(classes=[OK1, (8, 1, 0, 900, "bov")]), "class 1: n_proofs must be in [1, 2^22]"),
    (dict(classes=[OK1, (8, 1, (1 << 22) + 1, 0, "bov")]), "class 1: n_proofs must be in [1, 2^22]"),
    (dict(classes=[OK1, (8, 1, 3, 900, "bovd")]), "class 1: offset table leaves the buffer"),
    (dict(classes=[OK1, (256, 1, 3, 900, "bov")]), "class 1: n_gens exceeds n_gens_max"),
    (dict(classes=[OK1], n_gens_max=1), "n_gens_max must be in [2, 65536]"),
    (dict(classes=[OK1], n_gens_max=65537), "n_gens_max must be in [2, 65536]"),
]


@pytest.mark.parametrize("case,text", ERRORS, ids=["%s-%d" % (t[:28].replace(" ", "_"), i) for i, (_, t) in enumerate(ERRORS)])
def test_argument_errors_their_messages_and_nothing_else_set(plan, case, text):
    p = plan(**case)
    assert p["err"] == E_ARG and p["msg"] == text
    for key in ("n_classes", "N", "n_cls", "n_proofs", "n_pairs", "n_v", "stage_bytes", "need", "pin_bytes", "n_units"):
        assert p[key] == 0, key
    assert p["classes"] == [] and p["rounds"] == [] and p["merged"] == [0, 0] and p["bad"] == [0, 0] and p["units"] == [0, 0] and p["vstage"] == [0, 0]


def test_the_bound_of_2_23_points_at_the_bound_and_one_above(plan):
    """3 + 2 N + sum_c P_c (m_c + 6 + 2 k_c) with N = 4: a (2, 1) proof brings 9 pairs, a (4, 1) proof 11.  932 059 x 9 + 6 x 11 + 11 = 2^23 exactly;
    932 064 x 9 + 2 x 11 + 11 = 2^23 + 1."""
    assert 3 + 2 * 4 + 932059 * 9 + 6 * 11 == 1 << 23 and 3 + 2 * 4 + 932064 * 9 + 2 * 11 == (1 << 23) + 1
    p = plan([(2, 1, 932059, 0, "bov"), (4, 1, 6, 0, "bov")], n_gens_max=4)
    assert p["err"] == 0 and 3 + 2 * 4 + p["n_pairs"] == 1 << 23
    p = plan([(2, 1, 932064, 0, "bov"), (4, 1, 2, 0, "bov")], n_gens_max=4)
    assert p["err"] == E_ARG and p["msg"] == "at most 2^23 points in the batch's MSM" and p["classes"] == [] and p["need"] == 0
