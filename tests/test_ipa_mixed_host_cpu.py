"""The per-thread bodies of the s-vector kernels of a batch of proofs of DIFFERENT lengths (python-bulletproofs_amd/csrc/svector_mixed.hpp)
checked on the CPU: the header is plain C++, so tests/csrc_host/ipa_mixed_host_main.cpp -- a stand-alone program, built with the host
compiler and the address and undefined-behaviour sanitizers -- runs them through every table record, every lane of every unit of the
plan (ipa_mixed_plan_host.hpp) and the finish, and the sums are compared with Python integers (ipa_mixed_ref.ref_sums_mixed: each proof's
ipa_batch_ref.ref_sums over its own prefix)."""
import json
import os
import subprocess

import pytest

from ipa_batch_ref import draw_proofs, ref_sums
from ipa_mixed_ref import LENGTH_LISTS, MORE_LISTS, Q, draw_mixed, draw_scale_mixed, n_gens_of, ref_sums_mixed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "csrc_host", "ipa_mixed_host_main.cpp")
INC = os.path.join(REPO, "python-bulletproofs_amd", "csrc")

LISTS = LENGTH_LISTS + MORE_LISTS
CASES = [(at, scaled) for at in range(len(LISTS)) for scaled in (False, True)]


def hex64(v):
    return "%064x" % v


def case_id(case):
    ks = LISTS[case[0]]
    return "%dx%s-%s" % (len(ks), "k%d" % ks[0] if len(set(ks)) == 1 else "mixed%d" % max(ks), "scale" if case[1] else "plain")


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ipa_mixed_host") / "ipa_mixed_host_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe])
    text, inputs = [str(len(CASES))], {}
    for case in CASES:
        at, scaled = case
        ks = LISTS[at]
        n_gens = n_gens_of(ks)
        proofs = draw_mixed(ks, 1000 + at)
        scale = draw_scale_mixed(ks, n_gens, 77 + at) if scaled else None
        inputs[case] = (ks, proofs, scale)
        text.append("%d %d %d" % (n_gens, len(ks), 1 if scaled else 0))
        text.append(" ".join(str(k) for k in ks))
        for xs, a, b, w in proofs:
            text += [hex64(v) for x in xs for v in (x, pow(x, -1, Q))] + [hex64(a), hex64(b), hex64(w)]
        if scaled:
            text += [hex64(c) for c in scale]
    r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(lines) == len(CASES)
    return {case: (inputs[case], line) for case, line in zip(CASES, lines)}


def test_the_reference_is_ref_sums_of_every_proof_over_its_prefix():
    ks = [3, 0, 1, 3, 2]
    proofs = draw_mixed(ks, 5)
    sa, sb = ref_sums_mixed(ks, proofs)
    assert len(sa) == len(sb) == 8
    # element 0 is covered by all five proofs, elements 4 .. 7 by the two of 8 elements alone
    assert sa[0] == sum(ref_sums(k, [p])[0][0] for k, p in zip(ks, proofs)) % Q
    assert (sa[4:], sb[4:]) == tuple(v[4:] for v in ref_sums(3, [proofs[0], proofs[3]]))
    # one length: ref_sums itself
    same = draw_proofs(4, 6, 9)
    assert ref_sums_mixed([4] * 6, same) == ref_sums(4, same)


def test_edge_values_are_among_the_inputs():
    proofs = draw_mixed(LISTS[2], 1002)              # [6] * 3 + [5] * 2
    assert proofs[0][1] == 0 and proofs[0][3] == 1 and proofs[1][2] == 0 and proofs[1][3] == Q - 1
    assert proofs[0][0][0] == 1 and proofs[1][0][-1] == Q - 1 and proofs[3][1] == 0 and proofs[4][0][-1] == Q - 1
    assert proofs[2][0][3] == Q - 1 and proofs[2][0][2] == 1
    long_one = draw_mixed([17, 3], 1)
    assert long_one[1][1] == 0 and long_one[0][1] != 0 and long_one[0][2] != 0           # the long proof alone fills elements 8 ..: neither sum is zero there
    sc = draw_scale_mixed([7] * 3, 1 << 10, 1)
    assert len(sc) == 1 << 10 and sc[0] == 1 and sc[127] == 0


def test_the_cases_reach_the_paths_of_the_plan(results):
    shape = {case_id(c): (line["units"], line["per_part"], line["direct"]) for c, (_, line) in results.items()}
    assert shape["3xk0-plain"] == (3, 1, 0) and shape["3xk7-plain"] == (3, 1, 0)
    assert shape["1xk4-plain"] == (1, 1, 1) and shape["1xk4-scale"] == (1, 1, 0)              # one unit: SA / SB directly, unless there is a scale
    assert shape["2xmixed17-plain"] == (512, 2, 1) and shape["2xmixed17-scale"] == (512, 2, 0)
    assert shape["201xmixed9-plain"] == (201 + 1, 1, 0)           # block 0: 201 units, block 1: the long proof alone
    assert shape["2056xmixed6-plain"] == (686, 3, 0)              # ranges of three proofs, the last one of one


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_sums_equal_python_integers(results, case):
    (ks, proofs, scale), got = results[case]
    assert got["n_top"] == 1 << max(ks)
    sa, sb = ref_sums_mixed(ks, proofs, scale)
    assert got["sa"] == [hex64(v) for v in sa]
    assert got["sb"] == [hex64(v) for v in sb]
