"""The plan of a fixed-base MSM (python-bulletproofs_amd/csrc/msm_fixed_plan_host.hpp) checked on the CPU: the header is plain C++, so
tests/csrc_host/msm_fixed_plan_main.cpp -- a stand-alone program -- is compiled with the host compiler (address and undefined-behaviour
sanitizers on) and prints the plan of every shape as JSON: the windows W, the virtual windows Wv and the effective rows R of every
(window bits, rows), the map of the real windows onto (virtual window, row) slots, the virtual geometry against msm_pick_geometry's
for that size and width, the workspace against msm_layout's, the automatic rule at its bounds and every refusal with its text."""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "csrc_host", "msm_fixed_plan_main.cpp")
INC = os.path.join(REPO, "python-bulletproofs_amd", "csrc")

PAIRS_MAX = 1 << 23
MAX_N = 1 << 26
WIDTHS = range(10, 17)


def windows(c):
    return 255 // c + 1


def effective(c, rows):
    W = windows(c)
    Wv = -(-W // rows)
    return W, Wv, -(-W // Wv)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("msm_fixed_plan") / "msm_fixed_plan_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe])

    def run(shapes):
        """shapes: (accum_runs, chained, n, window_bits, rows)"""
        out = []
        for lo in range(0, len(shapes), 2000):          # (the argument list stays far below the system's limit)
            args = [str(x) for s in shapes[lo: lo + 2000] for x in s]
            r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-4000:]
            out += [json.loads(line) for line in r.stdout.splitlines()]
        assert len(out) == len(shapes)
        return out
    return run


@pytest.fixture(scope="module")
def grid(plans):
    """Every width, every rows value, and the sizes 1, 2, 511, 2^16, 2^19, 2^23 / R and 2^23 / R + 1 (R: the effective rows)."""
    shapes = []
    for c in WIDTHS:
        for rows in range(1, windows(c) + 1):
            R = effective(c, rows)[2]
            for n in (1, 2, 511, 1 << 16, 1 << 19, PAIRS_MAX // R, PAIRS_MAX // R + 1):
                for runs, chained in ((1, 0), (2, 0), (1, 1)):
                    shapes.append((runs, chained, n, c, rows))
    return list(zip(shapes, plans(shapes)))


def test_windows_rows_and_the_pair_bound(grid):
    refused = 0
    for (_, _, n, c, rows), p in grid:
        W, Wv, R = effective(c, rows)
        if n * R > PAIRS_MAX:
            assert p["err"] == -3 and "n x rows exceeds 2^23" in p["msg"], (n, c, rows)
            refused += 1
            continue
        assert p["err"] == 0 and p["msg"] is None
        assert (p["n"], p["c"], p["W"], p["Wv"], p["R"]) == (n, c, W, Wv, R), (n, c, rows)      # an explicit value is never overridden
        assert p["table_bytes"] == 64 * n * R and p["pairs_max"] == PAIRS_MAX
        assert Wv * R >= W > Wv * (R - 1)
    assert refused > 0


def test_rows_one_and_rows_w_are_the_two_ends(grid):
    for (_, _, n, c, rows), p in grid:
        if p["err"]:
            continue
        if rows == 1:
            assert p["R"] == 1 and p["Wv"] == p["W"]
        if rows == windows(c):
            assert p["R"] == p["W"] and p["Wv"] == 1


def test_window_map_is_a_bijection_onto_the_slots_below_w(grid):
    for (_, _, n, c, rows), p in grid:
        if p["err"]:
            continue
        W, Wv, R = p["W"], p["Wv"], p["R"]
        slots = [tuple(s) for s in p["map"]]
        assert len(slots) == W == len(set(slots))
        assert all(wv < Wv and r < R for wv, r in slots)
        # window w weighs 2^(c w) = 2^(c wv) x the row's 2^(c Wv r)
        assert all(c * w == c * wv + c * Wv * r for w, (wv, r) in enumerate(slots))
        free = {(wv, r) for wv in range(Wv) for r in range(R)} - set(slots)
        assert len(free) == Wv * R - W and all(r * Wv + wv >= W for wv, r in free)


def test_virtual_geometry_is_the_pipelines_own(grid):
    seen_runs, seen_inblock, seen_chained = set(), set(), set()
    for (runs, chained, n, c, rows), p in grid:
        if p["err"]:
            continue
        real = p["real"]
        assert (real["n"], real["c"], real["W"], real["w0"], real["top2"], real["B"]) == (n, c, p["W"], 0, 0, 1 << (c - 1))
        if p["R"] == 1:
            assert "virtual" not in p                        # the ordinary MSM: no virtual geometry at all
            continue
        v, o = p["virtual"], p["ordinary"]
        assert v == o
        assert (v["n"], v["c"], v["W"], v["w0"], v["top2"]) == (n * p["R"], c, p["Wv"], 0, 0)
        assert v["B"] == 1 << (c - 1) and v["G"] == p["Wv"] << (c - 1)
        assert p["family"] == [0, 0, 0]                       # the bucket pipeline: not the one-block kernels, not GLV
        assert p["ws"] == p["ws_ordinary"] and p["P"] == v["G"] >> 8 and 0 < p["P"] <= 2048
        assert p["dig16_codes"] == p["Wv"] * n * p["R"] and p["negs"] == n * p["R"]
        assert v["runs"] == (1 if runs == 2 and v["G"] >= 2048 else 0)          # "accum_runs" as for every window group
        # the in-block sort's bound counts VIRTUAL pairs
        assert v["inblock"] == (1 if v["n"] <= 1 << 15 or (c == 16 and v["n"] <= 1 << 17) else 0)
        seen_runs.add(v["runs"])
        seen_inblock.add(v["inblock"])
        seen_chained.add((chained, v["L"]))
    assert seen_runs == {0, 1} and seen_inblock == {0, 1} and len(seen_chained) > 2


def test_automatic_rule_keeps_the_pair_bound(plans):
    sizes = [1, 2, 511, 1 << 13, 1 << 14, 1 << 16, 1 << 18, 1 << 19, (1 << 19) + 1, 1 << 20, 1 << 22, (1 << 23) - 1, 1 << 23]
    shapes = [(1, 0, n, 0, 0) for n in sizes]
    shapes += [(1, 0, n, c, 0) for n in sizes for c in WIDTHS] + [(1, 0, n, 0, r) for n in sizes for r in (1, 2, 16)]
    for (_, _, n, c, rows), p in zip(shapes, plans(shapes)):
        if p["err"]:
            assert c == 0 and rows > 1 and n * effective(16, rows)[2] > PAIRS_MAX, (n, c, rows)      # only an explicit rows value can break the bound
            continue
        assert p["n"] == n and n * p["R"] <= PAIRS_MAX and p["R"] >= 1
        if c:
            assert p["c"] == c                                # explicit window bits stay
            # automatic rows: the most the bound allows
            best = max(effective(c, r)[2] for r in range(1, windows(c) + 1) if n * effective(c, r)[2] <= PAIRS_MAX)
            assert p["R"] == best
        if rows:
            assert p["c"] == 16 and p["R"] == effective(16, rows)[2]
        if not c and not rows and p["R"] == 1:
            assert (p["c"], p["W"], p["Wv"]) == (0, 0, 0)       # the ordinary MSM under the ctx's own options
    assert plans([(1, 0, (1 << 23) + 1, 0, 0)])[0]["err"] == -3
    # the measured bands (profiles/r14_msm_fixed.txt): a table from 2^13 to 2^18 pairs, the ordinary MSM on either side
    bands = [((1 << 13) - 1, (0, 1)), (1 << 13, (16, 16)), ((1 << 14) - 1, (16, 16)), (1 << 14, (16, 8)), ((1 << 16) - 1, (16, 8)), (1 << 16, (16, 4)),
             (1 << 18, (16, 4)), ((1 << 18) + 1, (0, 1)), (1 << 19, (0, 1)), (1 << 23, (0, 1))]
    for (n, want), p in zip(bands, plans([(1, 0, n, 0, 0) for n, _ in bands])):
        assert (p["c"], p["R"]) == want, n


def test_refusals_and_their_texts(plans):
    cases = [((1, 0, 0, 16, 16), "n must be at least 1"), ((1, 0, MAX_N + 1, 16, 1), "n exceeds BPMI_MAX_N"), ((1, 0, MAX_N + 1, 0, 0), "n exceeds BPMI_MAX_N"),
             ((1, 0, 100, 9, 1), "window_bits must be 0 or 10 .. 16"), ((1, 0, 100, 17, 1), "window_bits must be 0 or 10 .. 16"),
             ((1, 0, 100, 1, 0), "window_bits must be 0 or 10 .. 16"),
             ((1, 0, 100, 16, 17), "rows must be 0 or 1 .. W"), ((1, 0, 100, 13, 21), "rows must be 0 or 1 .. W"), ((1, 0, 100, 10, 27), "rows must be 0 or 1 .. W"),
             ((1, 0, 100, 0, 17), "rows must be 0 or 1 .. W"), ((1, 0, 100, 0, 27), "rows must be 0 or 1 .. W"),
             ((1, 0, (1 << 19) + 1, 16, 16), "n x rows exceeds 2^23"), ((1, 0, (1 << 23) + 1, 16, 1), "n x rows exceeds 2^23"), ((1, 0, 1 << 23, 13, 2), "n x rows exceeds 2^23")]
    for (shape, text), p in zip(cases, plans([s for s, _ in cases])):
        assert p["err"] == -3 and text in p["msg"], (shape, p)
        assert set(p) == {"err", "msg"}                       # nothing else is set
    ok = plans([(1, 0, 1 << 19, 16, 16), (1, 0, 1 << 23, 16, 1), (1, 0, 1, 10, 26)])
    assert [p["err"] for p in ok] == [0, 0, 0]
