"""The plan of a batched MSM -- many scalar vectors over one shared point set (python-bulletproofs_amd/csrc/msm_batch_plan_host.hpp) --
checked on the CPU: the header is plain C++, so tests/csrc_host/msm_batch_plan_main.cpp -- a stand-alone program -- is compiled with the
host compiler (address and undefined-behaviour sanitizers on) and prints the plan of every shape as JSON: the route at each bound and
under the forcing option, the blocks per window, the row ranges of a batch whose window sums exceed one launch, the workspace regions
and the error texts of the per-call caps."""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "csrc_host", "msm_batch_plan_main.cpp")
INC = os.path.join(REPO, "python-bulletproofs_amd", "csrc")

TOTALS = [0, 1, 2, 511, 512, 513, 8448, 8449, 16896, 16897, 33792, 33793, 1 << 20]
VECS = [1, 2, 63, 64, 65, 4096, 1 << 20]
NONE, LIGHT, MID, LOOP = 0, 1, 2, 3
LIGHT_NMAX, MID_NMAX, W = 512, 8448, 37
E_MAX = 256 << 20


def split(total, nseg, variant):
    """`total` pairs over nseg segments; variant 1 leaves one of them empty."""
    if nseg == 1:
        return (total, 0, 0)
    if nseg == 2:
        return (0, total, 0) if variant else (total // 2, total - total // 2, 0)
    return (total // 3, 0, total - total // 3) if variant else (total // 3, total // 3, total - 2 * (total // 3))


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("msm_batch_plan") / "msm_batch_plan_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe])

    def run(shapes):
        """shapes: (route, vecs, host_out, nseg, (n0, n1, n2), n_vec)"""
        args = [str(x) for r, v, h, nseg, ns, nv in shapes for x in (r, v, h, nseg) + tuple(ns) + (nv,)]
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-4000:]
        out = [json.loads(line) for line in r.stdout.splitlines()]
        assert len(out) == len(shapes)
        return out
    return run


@pytest.fixture(scope="module")
def grid(plans):
    shapes = [(0, 0, host_out, nseg, split(t, nseg, variant), nv) for t in TOTALS for nv in VECS if t * nv <= 1 << 30
              for nseg in (1, 2, 3) for variant in (0, 1) for host_out in (0, 1)]
    assert {sum(s[4]) for s in shapes} == set(TOTALS) and {s[5] for s in shapes} == set(VECS)
    return list(zip(shapes, plans(shapes)))


def want_parts(total):
    return -(-total // MID_NMAX)


def test_automatic_route_at_each_bound(grid):
    seen = set()
    for (_, _, _, nseg, ns, nv), p in grid:
        total = sum(ns)
        assert p["err"] == 0 and p["msg"] is None and p["total"] == total and p["n_vec"] == nv
        assert p["min_vecs_by_parts"] == [32, 32, 64, 64] and p["auto_parts_max"] == 3        # the measured bounds
        if total == 0:
            want = NONE
        elif total > p["auto_parts_max"] * MID_NMAX or nv < p["min_vecs_by_parts"][want_parts(total) - 1]:
            want = LOOP
        else:
            want = LIGHT if total <= LIGHT_NMAX else MID
        assert p["route"] == want, (ns, nv)
        seen.add((total, want))
        if want == LIGHT:
            assert (p["threads"], p["nmax"], p["parts"], p["W"]) == (256, LIGHT_NMAX, 1, W)
        elif want == MID:
            assert (p["threads"], p["nmax"], p["W"]) == (512, MID_NMAX, W)
            assert p["parts"] == want_parts(total) and 1 <= p["parts"] <= 4 and total <= p["parts"] * MID_NMAX
        else:
            assert p["launches"] == 0 and p["total_bytes"] == 0
    assert {(512, LIGHT), (513, MID), (8449, MID), (16897, MID), (33792, LOOP), (33793, LOOP), (1 << 20, LOOP), (0, NONE), (1, LOOP), (513, LOOP)} <= seen
    assert {want_parts(t) for t in (513, 8448, 8449, 16896, 16897, 33792)} == {1, 2, 3, 4}


def test_forced_routes(plans):
    shapes, want = [], []
    for total in (1, 512, 513, 8449, 33792, 33793, 1 << 20):
        for nv in (1, 5):
            if total * nv > 1 << 30:
                continue
            for route in (LIGHT, MID, LOOP):
                shapes.append((route, 0, 1, 1, (total, 0, 0), nv))
                ok = route == LOOP or total <= (LIGHT_NMAX if route == LIGHT else 4 * MID_NMAX)
                want.append(route if ok else None)
    for s, w, p in zip(shapes, want, plans(shapes)):
        if w is None:
            assert p["err"] == -3 and "route" not in p, s
            assert ("msm_batch_route = 1 (LIGHT) takes at most 512 pairs" if s[0] == LIGHT else "msm_batch_route = 2 (MID) takes at most 33792 pairs") in p["msg"]
        else:
            assert p["err"] == 0 and p["route"] == w, s                # one vector included: the forced route overrides min_vecs
            if w == MID:
                assert p["parts"] == want_parts(s[4][0])               # (a forced MID below 513 pairs is one part)


def check_ranges(p, nv):
    per_vec = 144 * p["W"] * p["parts"]
    assert 1 <= p["vecs"] <= nv and p["vecs"] * per_vec <= E_MAX
    assert p["launches"] == -(-nv // p["vecs"])
    rs = p["ranges"]
    if p["launches"] <= 512:
        assert [r[0] for r in rs] == list(range(p["launches"]))
        at = 0
        for _, v0, cnt in rs:                                      # consecutive, none empty, every row exactly once
            assert v0 == at and 1 <= cnt <= p["vecs"]
            at += cnt
        assert at == nv
    else:
        assert [r[0] for r in rs] == [0, 1, p["launches"] - 1]
        assert rs[0][1:] == [0, p["vecs"]] and rs[1][1:] == [p["vecs"], p["vecs"]]
        v0, cnt = rs[2][1:]
        assert v0 == (p["launches"] - 1) * p["vecs"] and 1 <= cnt <= p["vecs"] and v0 + cnt == nv


def test_vectors_per_launch_and_row_ranges(grid):
    split_seen = False
    for (_, _, _, nseg, ns, nv), p in grid:
        if p["route"] in (LIGHT, MID):
            check_ranges(p, nv)
            assert p["vecs"] == min(nv, E_MAX // (144 * W * p["parts"]))         # as many as fit
            split_seen |= p["launches"] > 1 and nv % p["vecs"] != 0
    assert split_seen                                                  # a batch of several launches with a short last one is among the shapes


def test_option_vecs_is_honoured(plans):
    shapes = [(LIGHT if nv < 32 else 0, v, 1, 2, (64, 65, 0), nv) for v, nv in ((3, 7), (1, 5), (5, 5), (7, 5), (1, 1 << 20), (1000, 1 << 20), (1 << 20, 1 << 20))]
    shapes += [(MID, v, 0, 1, (33792, 0, 0), nv) for v, nv in ((3, 7), (20000, 30000))]
    for s, p in zip(shapes, plans(shapes)):
        nv, cap = s[5], E_MAX // (144 * W * p["parts"])
        assert p["err"] == 0 and p["vecs"] == min(s[1], nv, cap), s     # never more than 256 MB of window sums
        check_ranges(p, nv)
    p = plans([(LIGHT, 3, 1, 1, (129, 0, 0), 7)])[0]
    assert p["ranges"] == [[0, 0, 3], [1, 3, 3], [2, 6, 1]]


def test_regions_are_aligned_disjoint_and_sized(grid):
    for (_, _, host_out, nseg, ns, nv), p in grid:
        if p["route"] not in (LIGHT, MID):
            continue
        want = {"E": 144 * p["W"] * p["parts"] * p["vecs"], "out": 64 * nv if host_out else 0}
        end = 0
        for name in ("E", "out"):                                     # this is the order of the layout
            off, size = p["regions"][name]
            assert off % 256 == 0 and off >= end and size == want[name], (ns, nv, name)
            end = off + size
        assert want["E"] <= E_MAX == p["e_bytes_max"]
        assert end <= p["total_bytes"] and p["total_bytes"] % 256 == 0 and p["total_bytes"] <= sum(want.values()) + 512


def test_caps_at_the_bound_and_one_above(plans):
    ok = [(0, 0, 1, 1, (1 << 26, 0, 0), 16), (0, 0, 1, 3, (1 << 25, 1 << 24, 1 << 24), 1), (0, 0, 0, 1, (1024, 0, 0), 1 << 20), (0, 0, 1, 2, (0, 0, 0), 1 << 20),
          (0, 0, 1, 3, (1 << 10, 1 << 9, 1 << 9), 1 << 19), (0, 0, 1, 1, (5, 0, 0), 0)]
    for shape, p in zip(ok, plans(ok)):
        assert p["err"] == 0 and p["msg"] is None, shape
    bad = [((0, 0, 1, 0, (1, 0, 0), 1), "nseg must be 1 .. 3"), ((0, 0, 1, 4, (1, 0, 0), 1), "nseg must be 1 .. 3"),
           ((0, 0, 1, 1, ((1 << 26) + 1, 0, 0), 1), "BPMI_MAX_N"), ((0, 0, 1, 3, (1 << 25, 1 << 25, 1), 1), "BPMI_MAX_N"),
           ((0, 0, 1, 2, (1 << 63, 1 << 63, 0), 1), "BPMI_MAX_N"),
           ((0, 0, 1, 1, (1, 0, 0), (1 << 20) + 1), "2^20 vectors"), ((0, 0, 1, 1, (0, 0, 0), (1 << 20) + 1), "2^20 vectors"),
           ((0, 0, 1, 1, (1025, 0, 0), 1 << 20), "2^30 pairs"), ((0, 0, 1, 2, (1 << 25, 1 << 25, 0), 17), "2^30 pairs")]
    for (shape, text), p in zip(bad, plans([b[0] for b in bad])):
        assert p["err"] == -3 and "route" not in p and text in p["msg"], (shape, p["msg"])
