"""The plan of bpmi_ipa_group_values_packed_dev (python-bulletproofs_amd/csrc/ipa_group_plan_host.hpp) on the CPU: the header is plain
C++, so tests/csrc_host/ipa_group_plan_main.cpp prints what the call decides before its first HIP call -- the argument errors with their
messages, the clamp of `group`, the regions of the groups behind the unchanged ipa_packed_plan, the route of the groups' MSMs and the
preparation rounds under a transposition budget -- and the lines are checked here."""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "csrc_host", "ipa_group_plan_main.cpp")
INC = os.path.join(REPO, "python-bulletproofs_amd", "csrc")
E_ARG = -3
LIGHT, MID, MSM_RUN = 1, 2, 3
WINDOWS = 255 // 7 + 1                      # windows of MID_C = 7 bits over 256-bit scalars

P2, P1 = "axltoupd", "axltoupchd"           # every required array and a seed, per protocol


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ipa_group_plan") / "ipa_group_plan_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe])

    def go(*cases):
        args = [str(v) for case in cases for v in case]
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [json.loads(line) for line in r.stdout.splitlines()]
        assert len(lines) == len(cases)
        return lines
    return go


def case(k, protocol, proofs, group, tr_len=100, scaled=0, present=None, offsets="up", outputs=1, budget=0):
    return (k, protocol, proofs, tr_len, scaled, present or (P1 if protocol == 1 else P2), offsets, group, outputs, budget)


SHAPES = [(k, protocol, scaled, group) for k in (0, 1, 3, 6, 10) for protocol in (1, 2) for scaled in (0, 1) for group in (1, 7, 300, 5000)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "k%d-p%d-%s-g%d" % (s[0], s[1], "scale" if s[2] else "plain", s[3]))
def test_regions_sit_on_256_byte_lines_and_do_not_overlap(plan, shape):
    k, protocol, scaled, group = shape
    P, n = 300, 1 << k
    (p,) = plan(case(k, protocol, P, group, tr_len=3 + 169 * k + 7, scaled=scaled, offsets="first"))
    assert p["err"] == 0
    g = min(group, P)                                            # the clamp
    ngroups = (P + g - 1) // g
    per = 2 * k + (4 if protocol == 1 else 2)
    assert (p["group"], p["ngroups"], p["per"], p["W"], p["pairs"], p["rows"]) == (g, ngroups, per, WINDOWS, 2 * n + g * per, P)
    reg = p["regions"]
    want = {"gsa": 32 * n * ngroups, "gsb": 32 * n * ngroups, "E": 144 * WINDOWS * ngroups, "vals": 64 * ngroups, "sa": 32 * n, "sb": 32 * n, "status": P}
    for name, nbytes in want.items():
        assert reg[name][1] == nbytes, name
    spans = sorted((o, o + b, name) for name, (o, b) in reg.items())
    assert all(o % 256 == 0 for o, _, _ in spans)
    for (_, end, a), (o, _, b) in zip(spans, spans[1:]):
        assert end <= o, (a, b)
    assert spans[-1][1] <= p["total_bytes"]
    # the regions of the unchanged packed plan come first, the groups' behind them in the order rows SA, rows SB, E, values
    old = [name for name in reg if name not in ("gsa", "gsb", "E", "vals")]
    assert max(reg[name][0] + reg[name][1] for name in old) <= p["packed_total"] == reg["gsa"][0]
    assert reg["gsa"][0] < reg["gsb"][0] < reg["E"][0] < reg["vals"][0]


@pytest.mark.parametrize("group", [300, 301, 65536, 1 << 40])
def test_a_group_above_the_batch_is_clamped_to_it(plan, group):
    (p,) = plan(case(6, 2, 300, group))
    assert p["err"] == 0 and (p["group"], p["ngroups"], p["pairs"]) == (300, 1, 128 + 300 * 14)


def test_a_short_last_group_is_a_group(plan):
    (p,) = plan(case(6, 2, 130, 9))
    assert p["err"] == 0 and (p["group"], p["ngroups"]) == (9, 15)


ROUTES = [                                   # k = 3: 16 generator pairs, 8 extra pairs per proof under protocol 2 and 10 under protocol 1
    (2, 62, LIGHT, 512), (2, 63, MID, 520), (2, 1054, MID, 8448), (2, 1055, MSM_RUN, 8456),
    (1, 49, LIGHT, 506), (1, 50, MID, 516), (1, 843, MID, 8446), (1, 844, MSM_RUN, 8456),
]


@pytest.mark.parametrize("protocol,group,route,pairs", ROUTES, ids=["p%d-g%d" % (r[0], r[1]) for r in ROUTES])
def test_the_routes_on_either_side_of_both_switches(plan, protocol, group, route, pairs):
    (p,) = plan(case(3, protocol, 1100, group))
    assert p["err"] == 0 and (p["group"], p["pairs"], p["route"]) == (group, pairs, route)


def test_one_proof_of_8192_elements_is_beyond_the_group_kernel(plan):
    p, q = plan(case(13, 2, 4, 1), case(12, 2, 4, 1))
    assert p["err"] == 0 and p["route"] == MSM_RUN and p["pairs"] == 2 * 8192 + 28
    assert q["err"] == 0 and q["route"] == MID and q["pairs"] == 2 * 4096 + 26


def test_a_transposition_budget_cuts_the_preparation_into_rounds_of_whole_waves(plan):
    whole, small, tiny, large = plan(case(3, 2, 130, 4), case(3, 2, 130, 4, budget=8 * (13 + 16) * 64), case(3, 2, 130, 4, budget=1000), case(3, 2, 130, 4, budget=1 << 40))
    assert whole["rows"] == 130 and large["rows"] == 130
    assert small["rows"] == 64 and tiny["rows"] == 64                 # never fewer than one wave of proofs
    for p in (small, tiny, large):
        assert p["regions"] == whole["regions"] and p["total_bytes"] == whole["total_bytes"]


ERRORS = [
    # what the packed verifier refuses
    (case(3, 0, 4, 1), "protocol must be 1 or 2"),
    (case(23, 2, 4, 1), "n must be 2^k, k <= 22"),
    (case(3, 2, 4, 1, present=P2.replace("a", "")), "null argument"),
    (case(3, 2, 4, 1, present=P2.replace("o", "")), "null argument"),
    (case(3, 2, 4, 1, present=P2.replace("x", "")), "xs and LR may be NULL only at k = 0"),
    (case(3, 1, 4, 1, present=P1.replace("c", "")), "protocol 1 needs c and head"),
    (case(3, 1, 4, 1, present=P1 + "s"), "start must be NULL under protocol 1"),
    (case(3, 2, 4, 1, present=P2 + "h"), "c and head must be NULL under protocol 2"),
    (case(3, 2, 4, 1, present=P2.replace("d", "")), "weights or a 32-byte seed"),
    (case(3, 2, 4, 1, offsets="down"), "tr_off must not decrease"),
    (case(1, 2, 65536, 1, tr_len=65537), "at most 4 GiB of transcripts per call"),
    (case(3, 2, 65537, 1), "between 1 and 2^16 proofs per call"),
    (case(22, 2, 1025, 1025), "at most 2^32 elements (proofs x n) per call"),
    (case(16, 1, 65536, 65536, tr_len=10), "exceed 1 GiB"),
    # its own
    (case(3, 2, 4, 0), "group must be at least 1"),
    (case(3, 2, 4, 1, outputs=0), "null argument (values and status)"),
    (case(16, 2, 1024, 1), "n_groups x 2 n must not exceed 2^26"),
    (case(22, 2, 16, 1), "n_groups x 2 n must not exceed 2^26"),
]


@pytest.mark.parametrize("args,text", ERRORS, ids=[("%s-%d" % (t[:24].replace(" ", "_"), i)) for i, (_, t) in enumerate(ERRORS)])
def test_argument_errors_and_their_messages(plan, args, text):
    (p,) = plan(args)
    assert p["err"] == E_ARG and text in p["msg"] and "regions" not in p


def test_the_row_cap_is_inclusive(plan):
    """ceil(n_proofs / group) x 2 n = 2^26 exactly is accepted; one group more is not (ERRORS above)."""
    p, q = plan(case(16, 2, 1024, 2), case(22, 2, 16, 2))
    assert p["err"] == 0 and p["ngroups"] * 2 * (1 << 16) == 1 << 26
    assert q["err"] == 0 and q["ngroups"] * 2 * (1 << 22) == 1 << 26
