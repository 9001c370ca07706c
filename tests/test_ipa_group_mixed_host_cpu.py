"""The per-thread body of the grouped s-vector sum over classes of DIFFERENT lengths (svm_group_row_element,
python-bulletproofs_amd/csrc/svector_mixed.hpp) checked on the CPU: the header is plain C++, so
tests/csrc_host/ipa_group_mixed_host_main.cpp -- a stand-alone program, built with the host compiler and the address and
undefined-behaviour sanitizers -- runs it over every lane of every block of k_sc_svector_sum_groups_mixed, with the class table and the
packed half-table array of the real plan, and every element of every group's row is compared with Python integers
(tests/ipa_batch_ref.py): row t of a class is the weighted sum over the proofs of group t of that class alone, over the class's own
2^k elements, SB times the shared scale of the element."""
import json
import os
import subprocess

import pytest

from ipa_batch_ref import Q, draw_proofs, draw_scale, ref_sums

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "csrc_host", "ipa_group_mixed_host_main.cpp")
INC = os.path.join(REPO, "python-bulletproofs_amd", "csrc")

# (k, proofs, group) per class, the caller's order.  The issue's three classes (k = 0 and 2: several groups share a wave; short last
# groups 3 = 2 + 1, 5 = 2 + 2 + 1, 9 = 4 + 4 + 1); the same in another order, so that the caller's order is not the tables' order; a
# class whose rows take three blocks in front of a small one (the block-to-class lookup beyond block 0), two classes of one k
SHAPES = [
    [(0, 3, 2), (2, 5, 2), (6, 9, 4)],
    [(6, 9, 4), (0, 3, 2), (2, 5, 2)],
    [(6, 9, 1), (2, 5, 9), (6, 2, 1)],
]
CASES = [(s, scaled) for s in range(len(SHAPES)) for scaled in (False, True)]


def hex64(v):
    return "%064x" % v


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ipa_group_mixed_host") / "ipa_group_mixed_host_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe])
    text, inputs = [str(len(CASES))], {}
    for case in CASES:
        s, scaled = case
        shape = SHAPES[s]
        proofs = [draw_proofs(k, p, 1000 * k + p + 31 * c) for c, (k, p, _) in enumerate(shape)]
        scale = draw_scale(max(k for k, _, _ in shape), 77 + s) if scaled else None
        inputs[case] = (proofs, scale)
        text.append("%d %d" % (len(shape), 1 if scaled else 0))
        text += ["%d %d %d" % c for c in shape]
        for cls in proofs:
            for xs, a, b, w in cls:
                text += [hex64(v) for x in xs for v in (x, pow(x, -1, Q))] + [hex64(a), hex64(b), hex64(w)]
        if scaled:
            text += [hex64(c) for c in scale]
    r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(lines) == len(CASES)
    return {case: (inputs[case], line) for case, line in zip(CASES, lines)}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "shape%d-%s" % (c[0], "scale" if c[1] else "plain"))
def test_every_element_of_every_group_equals_python_integers(results, case):
    s, scaled = case
    (proofs, scale), got = results[case]
    assert got["pad_untouched"] == 1                       # pad lanes wrote nothing, and every scalar of every row was written once
    for c, (k, count, group) in enumerate(SHAPES[s]):
        n, g = 1 << k, min(group, count)
        ngroups = (count + g - 1) // g
        rows = got["classes"][c]
        assert len(rows["sa"]) == len(rows["sb"]) == n * ngroups
        for t in range(ngroups):
            sa, sb = ref_sums(k, proofs[c][t * g: (t + 1) * g], None if scale is None else scale[:n])
            assert rows["sa"][n * t: n * (t + 1)] == [hex64(v) for v in sa], (c, t)
            assert rows["sb"][n * t: n * (t + 1)] == [hex64(v) for v in sb], (c, t)
        assert all(int(v, 16) < Q for v in rows["sa"] + rows["sb"])          # canonical


def test_the_shapes_cover_the_lookup_and_the_clamp():
    assert any(sum(((p + min(g, p) - 1) // min(g, p)) << k for k, p, g in shape[:1]) > 256 for shape in SHAPES)     # a first class of several blocks
    assert any(g > p for shape in SHAPES for _, p, g in shape)                                                      # group > count
    assert any(len({k for k, _, _ in shape}) < len(shape) for shape in SHAPES)                                      # two classes of one k
