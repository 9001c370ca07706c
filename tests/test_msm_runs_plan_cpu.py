"""The plan of the accumulation by runs -- MsmGeom.runs, the cap on the run length and the shape of the run table
(python-bulletproofs_amd/csrc/msm_plan_host.hpp) -- checked on the CPU: tests/csrc_host/msm_runs_plan_main.cpp, a stand-alone program, is
compiled with the host compiler (address and undefined-behaviour sanitizers on) and prints one JSON line per shape."""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "csrc_host", "msm_runs_plan_main.cpp")
INC = os.path.join(REPO, "python-bulletproofs_amd", "csrc")

SIZES = [1, 2560, 8448, 8449, 18999, 19000, 184999, 185000, (1 << 19) - 1, 1 << 19, (1 << 19) + 77, 1 << 20, (1 << 20) + 1, 1 << 22, 1 << 23, (1 << 23) + 1]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("msm_runs_plan") / "msm_runs_plan_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe])

    def run(shapes):
        """shapes: (accum_runs, accum_runs_cap, window_bits, glv, mode_bits, n, w0, wcount)"""
        r = subprocess.run([exe] + [str(x) for s in shapes for x in s], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-4000:]
        out = [json.loads(line) for line in r.stdout.splitlines()]
        assert len(out) == len(shapes)
        return out
    return run


def lds_sort(p):
    return not p["mid"] and not p["small"] and p["P"] != 0


def test_defaults_and_the_rule(plans):
    """accum_runs = 1 (the default): the LDS-sort pipeline at c = 16, not GLV, whole MSMs, from 2^19 pairs -- whatever the mode."""
    shapes = [(1, 0, 0, 0, mode, n, 0, 0) for n in SIZES for mode in (0, 1, 4)]
    seen = set()
    for s, p in zip(shapes, plans(shapes)):
        assert p["default_runs"] == 1 and p["default_cap"] == 0
        want = 1 if (lds_sort(p) and p["c"] == 16 and (1 << 19) <= s[5] <= (1 << 23)) else 0
        assert p["runs"] == want, s
        seen.add((s[5], want))
    assert {((1 << 19) - 1, 0), (1 << 19, 1), (1 << 20, 1), (1 << 23, 1), ((1 << 23) + 1, 0), (19000, 0), (185000, 0)} <= seen


def test_never_always_and_what_always_excludes(plans):
    shapes = [(v, 0, c, 0, 0, n, 0, 0) for v in (0, 2) for c in (0, 8, 10, 12, 13, 16) for n in SIZES]
    for s, p in zip(shapes, plans(shapes)):
        assert p["runs"] == (1 if s[0] == 2 and lds_sort(p) else 0), s
        if p["runs"]:
            assert p["c"] >= 10 and p["G"] >= 2048
    # GLV never; a window group only under 2; forced window bits other than 16 only under 2
    rows = plans([(2, 0, 0, 1, 0, 1 << 20, 0, 0), (1, 0, 0, 1, 0, 1 << 20, 0, 0), (1, 0, 16, 0, 0, 1 << 20, 0, 8), (2, 0, 16, 0, 0, 1 << 20, 8, 8),
                  (1, 0, 15, 0, 0, 1 << 20, 0, 0), (2, 0, 15, 0, 0, 1 << 20, 0, 0), (1, 0, 16, 0, 0, 1 << 20, 0, 0)])
    assert rows[0]["glv"] == 1 and [r["runs"] for r in rows] == [0, 0, 0, 1, 0, 1, 1]


def test_cap_rule_and_forced_cap(plans):
    """Twice the mean run length ceil(n W / G) plus 64; a forced cap is taken as it is."""
    shapes = [(2, 0, 0, 0, 0, n, 0, 0) for n in SIZES if n >= 8449] + [(2, 0, 10, 0, 0, 1 << 22, 0, 0)]
    for s, p in zip(shapes, plans(shapes)):
        mean = -(-(p["n"] * p["W"]) // p["G"])
        assert p["cap"] == 2 * mean + 64, s
    by_n = {s[5]: p for s, p in zip(shapes, plans(shapes))}
    assert by_n[1 << 20]["cap"] == 128 and by_n[1 << 19]["cap"] == 96 and by_n[8449]["cap"] == 72
    for cap in (1, 2, 40, 1023, 1024, 1 << 30):
        p = plans([(2, cap, 0, 0, 0, 1 << 20, 0, 0)])[0]
        assert p["cap"] == cap


def test_table_shape_fits_the_regions_it_borrows(plans):
    """order[] (at most G keys) in `cursor`, the per-block counts in `hist` (both 4 G bytes), the flag and the count in the spare words
    of coarse_hist between the last-block tickets (+1, +2) and the finish's (+8 ...)."""
    shapes = [(2, cap, c, 0, 0, n, 0, 0) for cap in (0, 1, 1022, 1023, 1024, 1 << 30) for c in (0, 10, 11, 14, 16) for n in SIZES if n >= 8449]
    seen_bins = set()
    for s, p in zip(shapes, plans(shapes)):
        if not p["runs"]:
            continue
        assert p["run_bins"] == 1024 and p["run_slice"] == 4096
        assert p["bins"] == min(p["cap"], p["run_bins"] - 1) + 1 and 2 <= p["bins"] <= p["run_bins"]
        assert p["blocks"] == -(-p["G"] // p["run_slice"]) and p["blocks"] * p["run_slice"] >= p["G"]
        assert p["blocks"] * p["bins"] <= p["G"], s                        # the counts fit `hist`
        assert p["order_off"] == p["cursor_off"] and p["counts_off"] == p["hist_off"] and p["flags_off"] == p["coarse_hist_off"]
        assert p["hist_off"] + 4 * p["G"] <= p["off_off"] and p["cursor_off"] != p["hist_off"]
        assert 2048 + 2 < p["flag_word"] < p["count_word"] < 2048 + 8 and p["count_word"] < p["coarse_hist_words"]
        seen_bins.add(p["bins"])
    assert {2, 1023, 1024} <= seen_bins
