"""The plan of a MIXED call of the batched range-proof prover (python-bulletproofs_amd/csrc/rp_prove_mixed_plan_host.hpp) checked on the
CPU: tests/csrc_host/rp_prove_mixed_plan_main.cpp -- a stand-alone program -- is compiled with the host compiler under the address and
undefined-behaviour sanitizers and prints base lists and plans as JSON.  Pinned here: the class base lists against rpp_plan's, every
argument error and cap, the classes' regions, class-major numbering, the launches of every step with their bounds, and the unit
tables."""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "tests", "csrc_host")
INC = os.path.join(REPO, "python-bulletproofs_amd", "csrc")

POW2 = [1 << e for e in range(0, 11)]
SHAPES = [(nb, m) for nb in POW2 if nb <= 128 for m in POW2 if 2 <= nb * m <= 1024]
ARRAYS = ("dig0", "dlen", "val", "gam", "tr", "trlen", "slr", "alpha", "chal", "tau", "tsc", "res", "xs", "xr", "a", "b", "cg", "hf", "jsc", "jout", "pts")
CHAINS = ("k_pv_chal_yz_mixed", "k_pv_final_chal_mixed", "k_pv_round_chal_mixed", "k_pv_emit_mixed")
WIDES = ("k_pv_poly_mixed", "k_pv_final_wide_mixed", "k_pv_round_wide_mixed")
THE_ISSUE_BLOCK = [(4, 3), (1, 65), (128, 2), (32, 1), (64, 2), (1, 2)]          # capacity (8, 128): (m, proofs), unsorted, m = 1 twice


def _build(tmp, name):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", INC,
                           os.path.join(CSRC, name + ".cpp"), "-o", exe])
    return exe


def _lines(exe, args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return [json.loads(line) for line in r.stdout.splitlines()]


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("rp_prove_mixed_plan"), "rp_prove_mixed_plan_main")


@pytest.fixture(scope="module")
def single(tmp_path_factory):
    """rpp_plan of every legal shape, from the single-class plan's own program."""
    exe = _build(tmp_path_factory.mktemp("rp_prove_plan_for_mixed"), "rp_prove_plan_main")
    return {(p["bits"], p["values"]): p for p in _lines(exe, [x for nb, m in SHAPES for x in (nb, m, 0)])}


def plan(mixed, nbits, M, classes, fmt=2, lanes=0):
    """classes: (m, count) or (m, count, seed total, longest seed)"""
    args = ["plan", nbits, M, fmt, lanes] + ["%d:%d:%d:%d" % (tuple(c) + (0, 0))[:4] for c in classes]
    (p,) = _lines(mixed, args)
    return p


def test_class_bases_equal_the_single_class_plan(mixed, single):
    """rpp_class_bases(n, n) == rpp_plan(..).bases, entry for entry, for every legal shape."""
    sizes = sorted({nb * m for nb, m in SHAPES})
    got = {b["n"]: b for b in _lines(mixed, ["bases"] + [x for n in sizes for x in (n, n)])}
    assert sizes == [1 << e for e in range(1, 11)]
    for (nb, m), p in single.items():
        assert got[nb * m]["bases"] == p["bases"] and got[nb * m]["len"] == len(p["bases"]), (nb, m)


def test_class_bases_under_a_capacity(mixed, single):
    """n_c < N: the gs entries stay at 3 + j, the hs entries sit at 3 + N + j, g / h / u stay 0 / 1 / 2, every index is below 3 + 2N,
    and the list is rpp_plan's with exactly the hs entries moved."""
    pairs = [(n, N) for N in (2, 8, 64, 1024) for n in (1 << e for e in range(1, 11)) if n < N] + [(512, 1024)]
    by_n = {p["n"]: p["bases"] for p in single.values()}
    for b in _lines(mixed, ["bases"] + [x for pr in pairs for x in pr]):
        n, N, bl = b["n"], b["N"], b["bases"]
        assert len(bl) == len(by_n[n]) and max(bl) < 3 + 2 * N
        for got, own in zip(bl, by_n[n]):
            assert got == (own if own < 3 + n else own - n + N), (n, N)
        assert bl[n: 2 * n] == [3 + N + j for j in range(n)] and bl[:n] == [3 + j for j in range(n)]


ERRORS = [
    ((8, 128), [(3, 1)], "class 0: the number of values must be a power of two"),
    ((8, 128), [(1, 1), (256, 1)], "class 1: the number of values must be a power of two, at most the prover's"),
    ((8, 128), [(0, 1)], "class 0: the number of values"),
    ((1, 2), [(1, 1)], "class 0: the number of values must be a power of two, at most the prover's, with bits x values >= 2"),
    ((8, 128), [(4, 2), (4, 0)], "class 1: n_proofs must be at least 1"),
    ((8, 128), [(1, 1)] * 65, "n_classes must be at most 64"),
    ((8, 128), [(1, 1 << 19), (2, 1 << 19), (1, 1)], "at most 2^20 proofs per call"),
    ((8, 128), [(1, (1 << 20) + 1)], "at most 2^20 proofs per call"),
    ((8, 128), [(1, (1 << 64) - 1)], "at most 2^20 proofs per call"),
    ((8, 128), [(128, 1 << 16), (64, 1 << 17), (1, 1)], "at most 2^27 elements (proofs x bits x values) per call"),
    ((8, 128), [(128, (1 << 17) + 1)], "at most 2^27 elements"),
    ((8, 128), [(4, 2, 70000, 65536)], "class 0: a seed is longer than 65535 bytes"),
    ((8, 256), [(4, 2)], "powers of two with 2 <= bits x values <= 1024"),
    ((3, 4), [(4, 2)], "powers of two"),
]


@pytest.mark.parametrize("cap,classes,text", ERRORS)
def test_argument_errors_and_caps(mixed, cap, classes, text):
    p = plan(mixed, cap[0], cap[1], classes)
    assert p["err"] != 0 and text in p["msg"] and "classes" not in p and "launches" not in p


def test_the_caps_themselves_are_legal(mixed):
    """Exactly 2^20 proofs, exactly 2^27 elements, 64 classes, a 65 535-byte seed, two classes of the same m; zero classes: an empty plan."""
    for classes in ([(1, 1 << 19), (2, 1 << 19)], [(128, 1 << 16), (64, 1 << 17)], [(1, 1)] * 64, [(4, 2, 65535 + 3, 65535)], [(2, 5), (2, 7)]):
        p = plan(mixed, 8, 128, classes)
        assert p["err"] == 0 and p["msg"] == "" and len(p["classes"]) == len(classes)
    p = plan(mixed, 8, 128, [(2, 5), (2, 7)])
    assert [c["m"] for c in p["classes"]] == [2, 2] and [c["count"] for c in p["classes"]] == [5, 7]
    e = plan(mixed, 8, 128, [])
    assert e["err"] == 0 and e["classes"] == [] and e["launches"] == [] and e["n_proofs"] == 0 and e["total_out"] == 0 and e["nsteps"] == 0


def _check_regions(p):
    """Every region of every class and of the call: 256-byte aligned, pairwise disjoint, inside `need`; the uploaded ones inside in_bytes."""
    spans = []
    for c, q in enumerate(p["classes"]):
        assert sorted(q["regions"]) == sorted(ARRAYS)
        for name, (off, size) in q["regions"].items():
            spans.append((off, off + size, "class %d %s" % (c, name)))
            assert off % 256 == 0
            assert (off + size <= p["in_bytes"]) if name in q["input"] else (off >= p["in_bytes"])
    for name, (off, size) in p["call_regions"].items():
        spans.append((off, off + size, name))
        assert off % 256 == 0
        assert (off >= p["in_bytes"]) if name == "out" else (off + size <= p["in_bytes"])
    spans.sort()
    for (a0, a1, an), (b0, b1, bn) in zip(spans, spans[1:]):
        assert a1 <= b0, (an, bn)
    assert spans[-1][1] <= p["need"] and spans[0][0] >= 0


def _blocks(kind, q, L, jobs):
    """blocks of class q in launch L, by the single-class call's grid of the same kernel"""
    P, n = q["count"], q["n"]
    if kind == "k_pv_blind_mixed":
        return -(-P * (2 * n + 2) // 256)
    if kind == "k_pv_commit_A_mixed":
        return -(-P * 16 // 256)
    if kind == "k_pv_affine_mixed":
        return -(-P * L["per"] // 256)
    if kind == "k_pv_msm_mixed":
        return -(-(jobs << L["gl"]) // 256)
    if kind in CHAINS:
        return -(-P // 64)
    return -(-P // q["per_block"])


def _check_plan(p, nbits, M, classes, single, lanes=0):
    cls = p["classes"]
    C = len(cls)
    # geometry by rpp_plan's rules; class-major numbering in the caller's order; strides; output slices
    first = out_at = seed_at = 0
    for q, c in zip(cls, classes):
        m, count = c[0], c[1]
        s = single[(nbits, m)]
        assert (q["m"], q["count"], q["n"], q["k"], q["NT"], q["per_block"]) == (m, count, s["n"], s["k"], s["NT"], s["per_block"])
        assert q["npt"] == 6 + 2 * q["k"] and q["first"] == first
        n, k = q["n"], q["k"]
        r = q["regions"]
        strides = {"slr": 32 * (2 * n + 1), "a": 32 * n, "b": 32 * n, "cg": 32 * n, "hf": 32 * n, "jsc": 32 * (2 * n + 2), "xs": 32 * k, "pts": 64 * (6 + 2 * k),
                   "val": 32 * m, "gam": 32 * m, "tr": q["tr_stride"], "dig0": q["dig0_stride"]}
        for name, st in strides.items():
            assert r[name][1] == count * st, name
        smax, stot = (c[3], c[2]) if len(c) > 2 else (0, 0)
        assert q["dig0_stride"] == ((smax + 2) // 3 * 4 + 1 + 15) // 16 * 16                                   # the formulas of rp_prove_batch_impl
        assert q["tr_stride"] == (max(q["dig0_stride"] + 4 * 45 + 3 * 80, 81 + k * 170) + 64 + 15) // 16 * 16
        fixed = 6 + 32 * (5 + k) + 33 * (6 + 2 * k) + 128 + 2 + 2
        assert q["fixed_bytes"] in (fixed, fixed + 32 * (6 + 2 * k))
        assert (q["out_at"], q["out_bytes"], q["seed_at"]) == (out_at, count * q["fixed_bytes"] + stot, seed_at)
        # base lists: the capacity's array holds the classes m = 1, 2, 4 .. (bits x m >= 2) one after the other
        assert q["bases_off"] == sum(len(single[(nbits, mm)]["bases"]) for mm in (1 << e for e in range(11)) if mm < m and nbits * mm >= 2)
        first, out_at, seed_at = first + count, out_at + q["out_bytes"], seed_at + stot
    assert (p["n_proofs"], p["total_out"], p["seed_bytes"]) == (first, out_at, seed_at)
    k_max = max(q["k"] for q in cls)
    assert p["k_max"] == k_max and p["nsteps"] == 4 + k_max and p["N"] == nbits * M
    _check_regions(p)
    # ---- the launches
    steps = {}
    for L in p["launches"]:
        steps.setdefault(L["step"], []).append(L)
    assert sorted(steps) == list(range(4 + k_max))
    assert [L["step"] for L in p["launches"]] == sorted(L["step"] for L in p["launches"])
    jobs = p["jobs"]
    assert len(jobs) == (3 + k_max) * C
    for s, Ls in steps.items():
        names = [L["name"] for L in Ls]
        r = s - 3
        members = [c for c in range(C) if s < 3 or s == 3 + k_max or cls[c]["k"] > r]      # a round lists exactly the classes with k_c > r
        assert members
        # the launch bounds: one launch per one-lane-per-proof kernel, per k_pv_blind / k_pv_commit_A; affine: one per point kind;
        # at most one per block size for a wide kernel (two kinds in step 2: the vectors, then round 0's scalars); one msm per lane width
        for name in CHAINS + ("k_pv_blind_mixed", "k_pv_commit_A_mixed"):
            assert names.count(name) <= 1
        assert names.count("k_pv_affine_mixed") == (2 if s == 0 else 0 if s == 3 + k_max else 1)
        for name in WIDES:
            sizes = [(L["threads"], L["first"]) for L in Ls if L["name"] == name]
            assert len(sizes) == len(set(sizes)) <= 3 and {t for t, _ in sizes} <= {256, 512, 1024}
        widths = [L["gl"] for L in Ls if L["name"] == "k_pv_msm_mixed"]
        assert len(widths) == len(set(widths)) and set(widths) <= {1, 4, 6} and (s == 3 + k_max) == (not widths)
        want = {0: ["k_pv_blind_mixed", "k_pv_commit_A_mixed", "k_pv_affine_mixed", "k_pv_msm_mixed", "k_pv_affine_mixed"],
                1: ["k_pv_chal_yz_mixed", "k_pv_poly_mixed", "k_pv_msm_mixed", "k_pv_affine_mixed"],
                2: ["k_pv_final_chal_mixed", "k_pv_final_wide_mixed", "k_pv_msm_mixed", "k_pv_affine_mixed", "k_pv_round_wide_mixed"]}.get(
                    s, ["k_pv_emit_mixed"] if s == 3 + k_max else ["k_pv_msm_mixed", "k_pv_affine_mixed", "k_pv_round_chal_mixed", "k_pv_round_wide_mixed"])
        assert [n for i, n in enumerate(names) if i == 0 or names[i - 1] != n] == want, (s, names)      # (a kernel's launches are consecutive)
        # the jobs of the step's multiplication, and a class's lane width by the jobs of the WHOLE launch
        if s < 3 + k_max:
            row = jobs[s * C: (s + 1) * C]
            total = sum(j[0] for j in row)
            for c, j in enumerate(row):
                q = cls[c]
                n = q["n"]
                if c not in members:
                    assert j[0] == 0
                    continue
                if s in (0, 2):
                    assert j[:5] == [q["count"], 1, 2 * n + 1, 2 * n + 1, 0 if s == 0 else 2 * n + 3] and j[5:] == [1 if s == 0 else 0, 0]
                elif s == 1:
                    assert j == [2 * q["count"], 1, 2, 2, 2 * n + 1, 0, 1]
                else:
                    assert j == [2 * q["count"], 2, n + 1, n + 1, 4 * n + 4 + r * 2 * (n + 1), 0, 0]
        # every unit table covers each member class's blocks exactly once, in the caller's order, padded to whole blocks per class
        by_kernel = {}
        for L in Ls:
            key = (L["name"], L["slot0"], L["first"]) if L["name"] != "k_pv_msm_mixed" else ("k_pv_msm_mixed",)
            by_kernel.setdefault(key, []).append(L)
        for key, group in by_kernel.items():
            seen = []
            for L in group:
                at = 0
                assert L["units"] and [u[0] for u in L["units"]] == sorted(u[0] for u in L["units"])
                for c, ufirst in L["units"]:
                    q = cls[c]
                    assert ufirst == at
                    if key[0] in WIDES:
                        assert L["threads"] == q["NT"]
                    elif key[0] == "k_pv_msm_mixed":
                        j = jobs[s * C + c]
                        width = 1 if s == 1 else {16: 4, 64: 6}.get(lanes, 6 if q["n"] > 128 and sum(x[0] for x in jobs[s * C: (s + 1) * C]) <= 4096 else 4)
                        assert L["gl"] == width and L["threads"] == 256
                    else:
                        assert L["threads"] == (64 if key[0] in CHAINS else 256)
                    at += _blocks(key[0], q, L, jobs[s * C + c][0] if s < 3 + k_max else 0)
                    seen.append(c)
                assert L["blocks"] == at
                if key[0] in ("k_pv_round_chal_mixed", "k_pv_round_wide_mixed") and s >= 3:
                    assert L["round"] == r and L["first"] == 0
            assert sorted(seen) == members, (s, key)
        for L in Ls:
            if L["name"] == "k_pv_affine_mixed":
                assert (L["per"], L["slot0"], L["slot_step"], L["step_k"]) == {0: (1, L["slot0"], 0, 0), 1: (2, 0, 1, 0), 2: (1, 5, 0, 0)}.get(s, (2, 6 + r, 0, 1))
        if s == 0:
            assert [L["slot0"] for L in Ls if L["name"] == "k_pv_affine_mixed"] == [2, 3]
        if s == 2:
            assert all(L["first"] == 1 and L["round"] == 0 for L in Ls if L["name"] == "k_pv_round_wide_mixed")


@pytest.mark.parametrize("lanes", [0, 16, 64])
def test_the_issue_block(mixed, single, lanes):
    """Capacity (8, 128) with the classes of the GPU test -- unsorted, m = 1 twice, 65 proofs in one class: all three block sizes."""
    classes = [(m, cnt, 301 * cnt, 300) for m, cnt in THE_ISSUE_BLOCK]
    p = plan(mixed, 8, 128, classes, lanes=lanes)
    assert p["err"] == 0
    _check_plan(p, 8, 128, classes, single, lanes)
    assert {q["NT"] for q in p["classes"]} == {256, 512, 1024} and {q["per_block"] for q in p["classes"]} == {32, 8, 1}
    chal = next(L for L in p["launches"] if L["name"] == "k_pv_chal_yz_mixed")
    assert chal["units"] == [[0, 0], [1, 1], [2, 3], [3, 4], [4, 5], [5, 6]] and chal["blocks"] == 7         # the 65 proofs: two chain blocks
    rounds = {L["round"]: [u[0] for u in L["units"]] for L in p["launches"] if L["name"] == "k_pv_round_chal_mixed"}
    ks = [q["k"] for q in p["classes"]]
    assert ks == [5, 3, 10, 8, 9, 3]
    assert rounds == {r: [c for c in range(6) if ks[c] > r] for r in range(10)}


@pytest.mark.parametrize("n_classes", [1, 5, 64])
def test_launch_bounds_for_1_5_and_64_classes(mixed, single, n_classes):
    """The launches of a step do not grow with the classes: 64 classes over every m of capacity (64, 16) launch what 5 launch."""
    ms = [1, 2, 4, 8, 16]
    classes = [(ms[(7 * c) % 5], 1 + (c * 37) % 70) for c in range(n_classes)]
    p = plan(mixed, 64, 16, classes, fmt=3)
    assert p["err"] == 0
    _check_plan(p, 64, 16, classes, single)
    assert all(q["fixed_bytes"] == 6 + 32 * (5 + q["k"]) + 33 * q["npt"] + 132 + 32 * q["npt"] for q in p["classes"])
    per_step = {}
    for L in p["launches"]:
        per_step[L["step"]] = per_step.get(L["step"], 0) + 1
    # step 0: 5; step 1: chain + <= 3 + 1 + 1; step 2: chain + <= 3 + <= 2 + 1 + <= 3; a round: <= 2 + 1 + 1 + <= 3; emit: 1
    assert per_step[0] <= 6 and per_step[1] <= 6 and per_step[2] <= 10 and per_step[max(per_step)] == 1
    assert all(v <= 7 for s, v in per_step.items() if 3 <= s < max(per_step))


def test_short_rounds_and_the_smallest_capacity(mixed, single):
    for nbits, M, classes in ((2, 4, [(1, 3), (2, 2), (4, 1)]), (1, 2, [(2, 4)]), (8, 128, [(128, 3)])):
        p = plan(mixed, nbits, M, classes)
        assert p["err"] == 0
        _check_plan(p, nbits, M, classes, single)
    p = plan(mixed, 2, 4, [(1, 3), (2, 2), (4, 1)])
    assert [q["k"] for q in p["classes"]] == [1, 2, 3] and p["nsteps"] == 7
