"""The per-thread body of the grouped s-vector sum (svb_group_element, python-bulletproofs_amd/csrc/svector_batch.hpp) checked on the CPU:
the header is plain C++, so tests/csrc_host/ipa_group_host_main.cpp -- a stand-alone program, built with the host compiler and the
address and undefined-behaviour sanitizers -- runs it under the flat (group, element) index of k_sc_svector_sum_groups, and the rows
are compared with Python integers (tests/ipa_batch_ref.py): row t is the weighted sum over the proofs of group t alone."""
import json
import os
import subprocess

import pytest

from ipa_batch_ref import Q, draw_proofs, draw_scale, ref_sums

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "csrc_host", "ipa_group_host_main.cpp")
INC = os.path.join(REPO, "python-bulletproofs_amd", "csrc")

KS = [0, 1, 2, 3, 6, 7]
PROOFS = [1, 2, 5]


def groups_of(proofs):
    return sorted({1, min(2, proofs), proofs})               # one proof per group, groups of 2 (5 proofs: 2, 2 and a short one), the whole batch


CASES = [(k, p, group, scaled) for k in KS for p in PROOFS for group in groups_of(p) for scaled in (False, True)]


def hex64(v):
    return "%064x" % v


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ipa_group_host") / "ipa_group_host_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe])
    text, inputs = [str(len(CASES))], {}
    for case in CASES:
        k, p, group, scaled = case
        proofs = draw_proofs(k, p, 1000 * k + p)
        scale = draw_scale(k, 77 + k) if scaled else None
        inputs[case] = (proofs, scale)
        text.append("%d %d %d %d" % (k, p, group, 1 if scaled else 0))
        for xs, a, b, w in proofs:
            text += [hex64(v) for x in xs for v in (x, pow(x, -1, Q))] + [hex64(a), hex64(b), hex64(w)]
        if scaled:
            text += [hex64(c) for c in scale]
    r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(lines) == len(CASES)
    return {case: (inputs[case], line) for case, line in zip(CASES, lines)}


def test_the_shapes_hold_a_short_last_group():
    assert (5, 2) in {(p, g) for _, p, g, _ in CASES} and 5 % 2


@pytest.mark.parametrize("case", CASES, ids=lambda c: "k%d-P%d-group%d-%s" % (c[0], c[1], c[2], "scale" if c[3] else "plain"))
def test_group_rows_equal_python_integers(results, case):
    k, p, group, scaled = case
    (proofs, scale), got = results[case]
    n, ngroups = 1 << k, (p + group - 1) // group
    assert len(got["sa"]) == len(got["sb"]) == n * ngroups
    for t in range(ngroups):
        sa, sb = ref_sums(k, proofs[t * group: (t + 1) * group], scale)
        assert got["sa"][n * t: n * (t + 1)] == [hex64(v) for v in sa], t
        assert got["sb"][n * t: n * (t + 1)] == [hex64(v) for v in sb], t
    assert all(int(v, 16) < Q for v in got["sa"] + got["sb"])          # canonical
