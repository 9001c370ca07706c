"""The plan of a batch of packed inner-product proofs (python-bulletproofs_amd/csrc/ipa_packed_plan_host.hpp) on the CPU: the header is
plain C++, so tests/csrc_host/ipa_packed_plan_main.cpp prints what bpmi_ipa_batch_prepare, bpmi_ipa_batch_prepare_dev and
bpmi_ipa_verify_batch_packed_dev decide before their first HIP call -- the argument errors with their messages, the extra pairs, the
upload regions behind those of the unchanged ipa_batch_plan -- and the lines are checked here."""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "csrc_host", "ipa_packed_plan_main.cpp")
INC = os.path.join(REPO, "python-bulletproofs_amd", "csrc")
E_ARG = -3

P2, P1 = "axltoupd", "axltoupchd"           # every required array and a seed, per protocol
KS = [0, 1, 6, 10, 22]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ipa_packed_plan") / "ipa_packed_plan_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe])

    def go(*cases):
        args = [str(v) for case in cases for v in case]
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [json.loads(line) for line in r.stdout.splitlines()]
        assert len(lines) == len(cases)
        return lines
    return go


def proofs_for(k):
    return 5 if k == 22 else 300


SHAPES = [(k, protocol, scaled, starts) for k in KS for protocol in (1, 2) for scaled in (0, 1) for starts in ((0, 1) if protocol == 2 else (0,))]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "k%d-p%d-%s-%s" % (s[0], s[1], "scale" if s[2] else "plain", "starts" if s[3] else "nostarts"))
def test_regions_sit_on_256_byte_lines_and_do_not_overlap(plan, shape):
    k, protocol, scaled, starts = shape
    P, tr_len = proofs_for(k), 3 + 169 * k + 7
    present = (P1 if protocol == 1 else P2) + ("s" if starts else "")
    explicit = present.replace("d", "w")
    p, pw = plan((k, protocol, P, tr_len, scaled, present, "first"), (k, protocol, P, tr_len, scaled, explicit, "up"))
    assert p["err"] == 0 and pw["err"] == 0
    pairs = 2 * k + (4 if protocol == 1 else 2)
    assert p["pairs"] == pairs and p["n_extra"] == pairs * P and p["rec_words"] == 16 * k + 24
    assert p["tr_bytes"] == tr_len * P and p["longest"] == tr_len and p["W"] == (tr_len + 7) // 8 + 16 and p["rows"] == P
    reg = p["regions"]
    want = {"ab": 64 * P, "xs": 32 * k * P, "lr": 128 * k * P, "tr": tr_len * P + 8, "troff": 8 * (P + 1), "start": 4 * P if starts else 0,
            "u": 64 if protocol == 1 else 64 * P, "P": 64 * P, "c": 32 * P if protocol == 1 else 0, "head": 128 * P if protocol == 1 else 0, "w": 0,
            "roles": 4 * P, "status": P, "T": 8 * p["W"] * P, "rec": 4 * (16 * k + 24) * P, "expt": 64 * pairs * P, "exsc": 32 * pairs * P, "sa": 32 << k, "sb": 32 << k}
    for name, nbytes in want.items():
        assert reg[name][1] == nbytes, name
    assert pw["regions"]["w"][1] == 32 * (3 if protocol == 1 else 1) * P
    spans = sorted((o, o + b, name) for name, (o, b) in reg.items())
    assert all(o % 256 == 0 for o, _, _ in spans)
    for (_, end, a), (o, _, b) in zip(spans, spans[1:]):
        assert end <= o, (a, b)
    assert spans[-1][1] <= p["total_bytes"]
    # the regions of the unchanged plan come first, the uploads behind them
    assert max(reg[name][0] + reg[name][1] for name in ("sa", "sb", "rec", "tab", "part", "expt", "exsc", "scale")) <= p["base_total"] <= reg["ab"][0]


def test_long_transcripts_run_as_launches_of_whole_waves(plan):
    (p,) = plan((1, 2, 65536, 60000, 0, P2, "up"))
    assert p["err"] == 0 and p["W"] == 7500 + 16
    assert p["rows"] % 64 == 0 and 64 <= p["rows"] < 65536 and 8 * p["W"] * p["rows"] <= 1 << 28 and p["regions"]["T"][1] == 8 * p["W"] * p["rows"]
    (p,) = plan((1, 2, 3, (1 << 17) + 1, 0, P2, "up"))           # a transcript beyond 2^17 bytes is an invalid PROOF, not an argument error
    assert p["err"] == 0 and p["longest"] == 1 << 17


ERRORS = [
    ((3, 0, 4, 100, 0, P2, "up"), "protocol must be 1 or 2"),
    ((3, 3, 4, 100, 0, P1, "up"), "protocol must be 1 or 2"),
    ((23, 2, 4, 100, 0, P2, "up"), "n must be 2^k, k <= 22"),
    ((3, 2, 4, 100, 0, P2.replace("a", ""), "up"), "null argument"),
    ((3, 2, 4, 100, 0, P2.replace("t", ""), "up"), "null argument"),
    ((3, 2, 4, 100, 0, P2.replace("o", ""), "up"), "null argument"),
    ((3, 2, 4, 100, 0, P2.replace("u", ""), "up"), "null argument"),
    ((3, 2, 4, 100, 0, P2.replace("p", ""), "up"), "null argument"),
    ((3, 2, 4, 100, 0, P2.replace("x", ""), "up"), "xs and LR may be NULL only at k = 0"),
    ((3, 1, 4, 100, 0, P1.replace("l", ""), "up"), "xs and LR may be NULL only at k = 0"),
    ((3, 1, 4, 100, 0, P1.replace("c", ""), "up"), "protocol 1 needs c and head"),
    ((3, 1, 4, 100, 0, P1.replace("h", ""), "up"), "protocol 1 needs c and head"),
    ((3, 1, 4, 100, 0, P1 + "s", "up"), "start must be NULL under protocol 1"),
    ((3, 2, 4, 100, 0, P2 + "c", "up"), "c and head must be NULL under protocol 2"),
    ((3, 2, 4, 100, 0, P2 + "h", "up"), "c and head must be NULL under protocol 2"),
    ((3, 2, 4, 100, 0, P2.replace("d", ""), "up"), "weights or a 32-byte seed"),
    ((3, 2, 4, 100, 0, P2, "down"), "tr_off must not decrease"),
    ((1, 2, 65536, 65537, 0, P2, "up"), "at most 4 GiB of transcripts per call"),
    ((3, 2, 0, 100, 0, P2, "up"), "between 1 and 2^16 proofs per call"),
    ((3, 2, 65537, 100, 0, P2, "up"), "between 1 and 2^16 proofs per call"),
    ((22, 2, 1025, 100, 0, P2, "up"), "at most 2^32 elements (proofs x n) per call"),
    ((16, 1, 65536, 10, 0, P1, "up"), "exceed 1 GiB"),
]


@pytest.mark.parametrize("case,text", ERRORS, ids=[("%s-%d" % (t[:24].replace(" ", "_"), i)) for i, (_, t) in enumerate(ERRORS)])
def test_argument_errors_and_their_messages(plan, case, text):
    (p,) = plan(case)
    assert p["err"] == E_ARG and text in p["msg"] and "regions" not in p


def test_k0_takes_no_xs_and_no_lr(plan):
    (p,) = plan((0, 2, 7, 1, 0, P2.replace("x", "").replace("l", ""), "up"))
    assert p["err"] == 0 and p["pairs"] == 2 and p["regions"]["xs"][1] == 0 and p["regions"]["lr"][1] == 0


def test_the_extra_pair_bound_cannot_be_reached_below_the_other_bounds():
    """2^16 proofs of Protocol 1 at k = 22 would bring 2^16 x 48 pairs, below 2^22: the bound of ipa_batch_plan is checked (a proof count
    above 2^16 is refused first) but no call inside the other bounds reaches it."""
    assert (1 << 16) * (2 * 22 + 4) < 1 << 22
