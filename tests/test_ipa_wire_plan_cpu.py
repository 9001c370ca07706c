"""The plan of a batch of BPIP2 inner-product proofs (python-bulletproofs_amd/csrc/ipa_wire_plan_host.hpp) on the CPU: the header is
plain C++, so tests/csrc_host/ipa_wire_plan_main.cpp prints what bpmi_ipa_wire_expand, bpmi_ipa_wire_expand_dev and
bpmi_ipa_verify_batch_wire_dev decide before their first HIP call -- the argument errors with their messages, the wire region and the
regions of the expansion behind those of the unchanged ipa_batch_plan, the rows W of the word-major transcripts and the proofs per
launch -- and the lines are checked here."""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "csrc_host", "ipa_wire_plan_main.cpp")
INC = os.path.join(REPO, "python-bulletproofs_amd", "csrc")
E_ARG = -3
ALL = "boupd"                       # every required array and a seed
MAX_TRANSCRIPT = 1 << 17
T_MAX = 1 << 28


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ipa_wire_plan") / "ipa_wire_plan_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe])

    def go(*cases):
        args = [str(v) for case in cases for v in case]
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [json.loads(line) for line in r.stdout.splitlines()]
        assert len(lines) == len(cases)
        return lines
    return go


def case(k, P, prefix=1, protocol=2, verify=1, scale=0, budget=0, present=ALL, offsets="up"):
    return (k, protocol, P, prefix, verify, scale, budget, present, offsets)


@pytest.mark.parametrize("k", [0, 1, 6, 10, 22])
@pytest.mark.parametrize("verify", [0, 1])
def test_regions_sit_on_256_byte_lines_and_do_not_overlap(plan, k, verify):
    P, prefix = (5 if k == 22 else 300), 9
    p, pw = plan(case(k, P, prefix, verify=verify, offsets="first"), case(k, P, prefix, verify=verify, present="boupw"))
    assert p["err"] == 0 and pw["err"] == 0
    blob = 78 + 98 * k + prefix
    assert p["pairs"] == 2 * k + 2 and p["wire_bytes"] == blob * P
    bound = prefix + 169 * k
    assert p["longest"] == bound and p["text_bound"] == bound * P and p["W"] == (bound + 7) // 8 + 16 and p["rows"] == P
    reg = p["regions"]
    want = {"wire": blob * P + 8, "off": 8 * (P + 1), "ab": 64 * P, "xs": 32 * k * P, "lr": 128 * k * P, "tr": 8, "troff": 8 * (P + 1), "start": 4 * P,
            "u": 64 * P * verify, "P": 64 * P * verify, "w": 0, "roles": 4 * P * verify, "lens": 4 * P, "flags": 2 * P, "status": P, "T": 8 * p["W"] * P}
    assert {name: b for name, (_, b) in reg.items()} == want
    assert p["c_head"] == [0, 0]                                           # Protocol 2: no c, no head
    assert pw["regions"]["w"][1] == 32 * P * verify
    spans = sorted((o, o + b) for o, b in reg.values() if b)
    assert spans[0][0] == p["base_total"] and (p["base_total"] > 0) == bool(verify)      # behind the s-vector workspace, when there is one
    for (o, e), (o2, _) in zip(spans, spans[1:]):
        assert o % 256 == 0 and e <= o2
    assert spans[-1][0] % 256 == 0 and spans[-1][1] <= p["total_bytes"]


@pytest.mark.parametrize("k", [0, 3, 6])
def test_W_follows_the_longest_blob(plan, k):
    rounds = 169 * k
    for prefix in (0, 7, 8, MAX_TRANSCRIPT - rounds):
        (p,) = plan(case(k, 3, prefix))
        assert p["longest"] == prefix + rounds and p["W"] == (prefix + rounds + 7) // 8 + 16, prefix
    (p,) = plan(case(k, 3, MAX_TRANSCRIPT))                               # the bound is cut at the packed verifier's cap: such a proof is invalid
    assert p["longest"] == MAX_TRANSCRIPT and p["W"] == MAX_TRANSCRIPT // 8 + 16
    (p,) = plan(case(k, 3, 40, offsets="short"))                          # blobs shorter than their fixed part expand to nothing
    assert p["longest"] == 0 and p["text_bound"] == 0 and p["W"] == 16


def test_rows_under_a_small_T_budget(plan):
    k, P, prefix = 6, 130, 9
    W = (prefix + 169 * k + 7) // 8 + 16
    full, small, tiny, over = plan(case(k, P, prefix), case(k, P, prefix, budget=8 * W * 64), case(k, P, prefix, budget=1), case(k, P, prefix, budget=T_MAX * 4))
    assert full["rows"] == P and over["rows"] == P
    assert small["rows"] == 64 and small["regions"]["T"][1] == 8 * W * 64
    assert tiny["rows"] == 64                                             # never fewer than 64 proofs per launch
    (p,) = plan(case(k, P, prefix, budget=8 * W * 129))
    assert p["rows"] == 128                                               # a multiple of 64
    (big,) = plan(case(0, 1 << 16, 1 << 15))                              # the default budget: 2^28 bytes of T
    Wb = (1 << 15) // 8 + 16
    assert big["rows"] == T_MAX // (8 * Wb) // 64 * 64 and big["rows"] < (1 << 16)


def test_argument_errors_by_message(plan):
    k = 6
    table = [
        (case(k, 4, protocol=1), "the wire format holds Protocol-2 proofs only"),
        (case(k, 4, protocol=0), "the wire format holds Protocol-2 proofs only"),
        (case(23, 4), "n must be 2^k, k <= 22"),
        (case(k, 4, present="oupd"), "null argument"),
        (case(k, 4, present="bupd"), "null argument"),
        (case(k, 4, present="bopd"), "null argument"),
        (case(k, 4, present="boud"), "null argument"),
        (case(k, 4, present="boup"), "weights or a 32-byte seed"),
        (case(k, 0), "between 1 and 2^16 proofs per call"),
        (case(k, (1 << 16) + 1), "between 1 and 2^16 proofs per call"),
        (case(22, 2048), "at most 2^32 elements (proofs x n) per call"),
        (case(k, 4, offsets="down"), "off must not decrease"),
        (case(k, 4, offsets="huge"), "at most 4 GiB of blobs per call"),
    ]
    for line, (_, msg) in zip(plan(*[c for c, _ in table]), table):
        assert line["err"] == E_ARG and line["msg"] == msg
    # the expansion alone needs no statements and no weights, and has no s-vector workspace to refuse
    ok, null = plan(case(22, 2048, verify=0, present="bo"), case(k, 4, verify=0, present="b"))
    assert ok["err"] == 0 and ok["base_total"] == 0
    assert null["err"] == E_ARG and null["msg"] == "null argument"
