"""The plan of a batch of inner-product verifications (python-bulletproofs_amd/csrc/ipa_batch_plan_host.hpp) checked on the CPU: the
header is plain C++, so tests/csrc_host/ipa_batch_plan_main.cpp -- a stand-alone program -- is compiled with the host compiler (address
and undefined-behaviour sanitizers on) and prints the plan of every shape as JSON: the index split, the table and record sizes, the
ranges of the summing kernel, the workspace regions, the MSM's pair count and the error texts of the per-call caps."""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "csrc_host", "ipa_batch_plan_main.cpp")
INC = os.path.join(REPO, "python-bulletproofs_amd", "csrc")

PROOFS = [1, 2, 3, 5, 16, 17, 64, 65, 130, 1000, 1024, 4096, 1 << 16]
REGIONS = ["sa", "sb", "rec", "tab", "part", "expt", "exsc", "scale"]


def table_bytes(k, proofs):
    return proofs * 64 * ((1 << (k // 2)) + (1 << (k - k // 2)))


def allowed(k, proofs):
    return proofs << k <= 1 << 32 and table_bytes(k, proofs) <= 1 << 30


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ipa_batch_plan") / "ipa_batch_plan_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe])

    def run(shapes):
        args = [str(x) for shape in shapes for x in shape]
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-4000:]
        out = [json.loads(line) for line in r.stdout.splitlines()]
        assert len(out) == len(shapes)
        return out
    return run


@pytest.fixture(scope="module")
def grid(plans):
    shapes = [(1 << k, p, e, hs) for k in range(23) for p in PROOFS if allowed(k, p)
              for e, hs in ((0, 0), (p * (2 * k + 2), 1), (p * (2 * k + 7) + 3, 2))]
    out = plans(shapes)
    assert {s[0] for s in shapes} == {1 << k for k in range(23)}
    return list(zip(shapes, out))


def test_index_split_and_sizes(grid):
    for (n, proofs, extra, hs), p in grid:
        k = n.bit_length() - 1
        assert p["err"] == 0 and p["msg"] is None
        assert (p["k"], p["kl"], p["kh"]) == (k, k // 2, k - k // 2)
        assert p["tab_entries"] == (1 << (k // 2)) + (1 << (k - k // 2))
        assert p["rec_words"] == 16 * k + 24                       # k pairs (x, x^-1), then a, b, w
        assert p["msm_pairs"] == 2 * n + extra


def test_regions_are_aligned_disjoint_and_sized(grid):
    for (n, proofs, extra, hs), p in grid:
        k = n.bit_length() - 1
        want = {"sa": 32 * n, "sb": 32 * n, "rec": proofs * (64 * k + 96), "tab": table_bytes(k, proofs),
                "part": 0 if p["direct"] else 2 * 32 * n * p["parts"], "expt": 64 * extra, "exsc": 32 * extra, "scale": 32 * n if hs == 2 else 0}
        end = 0
        for name in REGIONS:                                       # this is the order of the layout
            off, size = p["regions"][name]
            assert off % 256 == 0 and off >= end and size == want[name], (n, proofs, name)
            end = off + size
        assert end <= p["total_bytes"] and p["total_bytes"] % 256 == 0
        assert p["total_bytes"] <= sum(want.values()) + 256 * len(REGIONS)


def test_parts_follow_the_rule_of_the_header(grid):
    """waves = ceil(n / 64); want = ceil(1024 / waves); per_part = ceil(P / min(want, P)); parts = ceil(P / per_part)."""
    seen_multi = False
    for (n, proofs, extra, hs), p in grid:
        assert p["simds"] == 1024
        waves = -(-n // 64)
        want = -(-1024 // waves)
        per_part = -(-proofs // min(want, proofs))
        parts = -(-proofs // per_part)
        assert (p["per_part"], p["parts"]) == (per_part, parts), (n, proofs)
        assert 1 <= p["parts"] <= proofs
        # the ranges [j per_part, min((j + 1) per_part, P)) partition [0, P): the last one is not empty and reaches P
        assert (p["parts"] - 1) * p["per_part"] < proofs <= p["parts"] * p["per_part"]
        assert p["direct"] == (1 if p["parts"] == 1 and hs == 0 else 0)
        if n >= 1 << 16:
            assert p["parts"] == 1                                 # the elements alone fill the chip
        if proofs % want == 0:
            assert p["parts"] == want and p["parts"] * waves >= 1024          # a wave per SIMD where the proofs allow it
        if proofs < want:
            assert p["parts"] == proofs and p["per_part"] == 1
        seen_multi |= p["parts"] > 1 and p["per_part"] > 1 and proofs % p["per_part"] != 0
    assert seen_multi                                              # a last range shorter than the others is among the shapes


def test_caps_at_the_bound_and_one_above(plans):
    ok = [(1 << 22, 1, 0, 0), (1, 1 << 16, 0, 0), (1 << 20, 1 << 12, 0, 0), (1 << 14, 1 << 16, 0, 0), (1 << 15, 43690, 0, 0), (1024, 4, 1 << 22, 1)]
    for shape, p in zip(ok, plans(ok)):
        assert p["err"] == 0 and p["msg"] is None, shape
    assert table_bytes(14, 1 << 16) == 1 << 30 and table_bytes(15, 43690) <= 1 << 30 < table_bytes(15, 43691)
    bad = [((1 << 23, 1, 0, 0), "k <= 22"), ((3, 1, 0, 0), "2^k"), ((0, 1, 0, 0), "2^k"), ((1 << 40, 1, 0, 0), "k <= 22"),
           ((1024, 0, 0, 0), "2^16 proofs"), ((1, (1 << 16) + 1, 0, 0), "2^16 proofs"),
           ((1 << 20, (1 << 12) + 1, 0, 0), "2^32"), ((1 << 22, 1025, 0, 0), "2^32"),
           ((1 << 15, 43691, 0, 0), "1 GiB"), ((1 << 15, 1 << 16, 0, 0), "1 GiB"),
           ((1024, 4, (1 << 22) + 1, 1), "2^22 extra")]
    for (shape, text), p in zip(bad, plans([b[0] for b in bad])):
        assert p["err"] != 0 and "k" not in p and text in p["msg"], (shape, p["msg"])
