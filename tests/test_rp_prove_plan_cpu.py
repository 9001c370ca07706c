"""The plan of the batched range-proof prover (python-bulletproofs_amd/csrc/rp_prove_plan_host.hpp) checked on the CPU: the header is
plain C++, so tests/csrc_host/rp_prove_plan_main.cpp -- a stand-alone program -- is compiled with the host compiler and prints the plan
of every shape as JSON: block sizes, table windows, per-call caps, error texts and the base lists the kernels index."""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "csrc_host", "rp_prove_plan_main.cpp")
INC = os.path.join(REPO, "python-bulletproofs_amd", "csrc")

POW2 = [1 << e for e in range(0, 11)]
SHAPES = [(nb, m) for nb in POW2 if nb <= 128 for m in POW2 if 2 <= nb * m <= 1024]


def table_bytes(elems, w):
    """(3 + 2 n m) x ceil(256 / w) x 2^(w-1) x 64 B"""
    return (3 + 2 * elems) * -(-256 // w) * (1 << (w - 1)) * 64


BOUND = table_bytes(128, 16)                 # the largest default table of a proof of up to 128 elements: 8.7 GB


def _build(tmp, src):
    exe = str(tmp / os.path.basename(src)[:-4])
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", INC, src, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("rp_prove_plan"), SRC)


@pytest.fixture(scope="module")
def plans(exe):
    def run(shapes):
        args = [str(x) for shape in shapes for x in shape]
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-4000:]
        out = [json.loads(line) for line in r.stdout.splitlines()]
        assert len(out) == len(shapes)
        return out
    return run


@pytest.fixture(scope="module")
def defaults(plans):
    return {(p["bits"], p["values"]): p for p in plans([(nb, m, 0) for nb, m in SHAPES])}


def test_block_size_and_proofs_per_block(defaults):
    """NT = 256 up to 256 elements (the kernels of the narrow shapes; 256 elements: one proof per block), else one proof per block of n."""
    seen = set()
    for (nb, m), p in defaults.items():
        n = nb * m
        seen.add(n)
        assert p["err"] == 0 and p["n"] == n and 1 << p["k"] == n and p["nbases"] == 3 + 2 * n
        assert p["NT"] == (256 if n <= 256 else n) and p["NT"] in (256, 512, 1024)
        assert p["per_block"] == p["NT"] // n and p["per_block"] * n == p["NT"]
    assert seen == {1 << e for e in range(1, 11)}


def test_default_table_windows(defaults):
    """16 bits for every shape of up to 128 elements; above, the widest width in 4 .. 16 whose table stays within the 8.7 GB of 128
    elements at 16 bits, recomputed here from the size formula."""
    assert BOUND == 259 * 16 * 32768 * 64
    for (nb, m), p in defaults.items():
        n = nb * m
        want = 16 if n <= 128 else max(w for w in range(4, 17) if table_bytes(n, w) <= BOUND)
        assert p["tw"] == want, (nb, m)
        assert p["wt"] == -(-256 // want) and p["bt"] == 1 << (want - 1) and p["table_bytes"] == table_bytes(n, want)
        assert p["table_bytes"] <= BOUND
    assert defaults[(64, 4)]["tw"] == 14 and round(defaults[(64, 4)]["table_bytes"] / 1e9, 1) == 5.1
    assert defaults[(64, 8)]["tw"] < 14 and defaults[(64, 16)]["tw"] < defaults[(64, 8)]["tw"]


def test_explicit_table_windows_are_honoured(plans):
    shapes = [(64, 16, w) for w in range(4, 17)] + [(64, 1, 6), (16, 4, 12)]
    for (nb, m, w), p in zip(shapes, plans(shapes)):
        assert p["err"] == 0 and p["tw"] == w and p["table_bytes"] == table_bytes(nb * m, w)
    assert table_bytes(1024, 6) < 200e6            # what the GPU tests of the wide shapes build


def test_per_call_caps(defaults):
    """n_proofs <= 2^20 and n_proofs x n m <= 2^27 (what 2^20 proofs of 128 elements are), each with its bound in the text."""
    for (nb, m), p in defaults.items():
        n = nb * m
        assert p["max_proofs"] == min(1 << 20, (1 << 27) // n)
        e = p["batch_errors"]
        assert e["1"] is None and e[str(p["max_proofs"])] is None
        assert "2^20 proofs" in e[str((1 << 20) + 1)]
        over = e[str(p["max_proofs"] + 1)]
        assert over is not None and ("2^27" in over if n > 128 else "2^20" in over)
        if n > 128:
            assert "2^27" in e[str(1 << 20)]
    assert defaults[(64, 16)]["max_proofs"] == 1 << 17


def test_argument_errors(plans):
    bad = [(64, 32, 0), (128, 16, 0), (256, 1, 0), (256, 4, 0), (3, 1, 0), (64, 3, 0), (1, 1, 0), (0, 4, 0), (64, 0, 0), (1, 2048, 0), (1 << 31, 2, 0)]
    for shape, p in zip(bad, plans(bad)):
        assert p["err"] != 0 and "n" not in p, shape
        assert "powers of two" in p["msg"] and "1024" in p["msg"] and "128" in p["msg"]
    good = [(1, 2, 0), (1, 1024, 0), (128, 8, 0), (2, 1, 0), (128, 1, 0)]
    for shape, p in zip(good, plans(good)):
        assert p["err"] == 0 and p["msg"] is None, shape


def test_job_lanes(defaults):
    """16 lanes per job for every shape of up to 128 elements; above, a wave per job up to the measured crossover (launches of
    4 096 jobs); the option forces either."""
    for (nb, m), p in defaults.items():
        n = nb * m
        for njobs, opt, lanes in p["job_lanes"]:
            if opt:
                assert lanes == opt
            elif n <= 128:
                assert lanes == 16
            else:
                assert lanes == (64 if njobs <= p["wave_jobs_max"] else 16)


def test_base_lists(defaults):
    """S, T, P_new, and L and R of every round: L holds the gs_j with (j mod len) >= half, then the hs_j with (j mod len) < half, then u;
    R the complements (the comment of k_pv_round_wide) -- and the kernel's rank (j / len) * half + (i mod half) addresses every position
    of a list once."""
    for (nb, m), p in defaults.items():
        n, k, bl = nb * m, p["k"], p["bases"]
        gs, hs = [3 + j for j in range(n)], [3 + n + j for j in range(n)]
        assert max(bl) == 2 + 2 * n < 1 << 16
        assert p["off_S"] == 0 and bl[:2 * n + 1] == gs + hs + [1]
        assert p["off_T"] == 2 * n + 1 and bl[p["off_T"]: p["off_T"] + 2] == [0, 1]
        assert p["off_P"] == 2 * n + 3 and bl[p["off_P"]: p["off_P"] + 2 * n + 1] == gs + hs + [2]
        assert p["off_round"] == 4 * n + 4 and len(bl) == p["off_round"] + k * 2 * (n + 1)
        for r in range(k):
            ln = n >> r
            half = ln // 2
            at = p["off_round"] + r * 2 * (n + 1)
            L, R = bl[at: at + n + 1], bl[at + n + 1: at + 2 * (n + 1)]
            assert L[n] == 2 and R[n] == 2
            assert sorted(L[:n] + R[:n]) == gs + hs                                   # a partition of the generators
            assert L[:n // 2] == [3 + j for j in range(n) if j % ln >= half] and L[n // 2: n] == [3 + n + j for j in range(n) if j % ln < half]
            assert R[:n // 2] == [3 + j for j in range(n) if j % ln < half] and R[n // 2: n] == [3 + n + j for j in range(n) if j % ln >= half]
            hit = {"L": set(), "R": set()}
            for j in range(n):
                i = j % ln
                up = i >= half
                rank = (j // ln) * half + (i % half)
                g_list, h_list = ("L", "R") if up else ("R", "L")                     # where the kernel writes the scalars of gs_j and hs_j
                assert (L if up else R)[rank] == 3 + j and (R if up else L)[n // 2 + rank] == 3 + n + j
                hit[g_list].add(rank)
                hit[h_list].add(n // 2 + rank)
            assert hit["L"] == set(range(n)) and hit["R"] == set(range(n))


# every array of rpp::Batch, inputs first: tests/test_rp_prove_mixed_plan_cpu.py ARRAYS
ARRAYS = ("dig0", "dlen", "val", "gam", "tr", "trlen", "slr", "alpha", "chal", "tau", "tsc", "res", "xs", "xr", "a", "b", "cg", "hf", "jsc", "jout", "pts")
INPUTS = ARRAYS[:4]
LAYOUT_PROOFS = (1, 3, 64, 65)
LAYOUT_SEEDS = ((0, 0), (7, 3), (65535, 65535))                  # total, longest


def test_single_class_layout(exe, tmp_path_factory):
    """rpp_layout, the device buffer of bpmi_rp_prove_batch, for every legal shape: aligned, disjoint, inside `need`, the upload inside
    in_bytes, every array of the stated size -- and region for region the one-class mixed plan without its three device tables."""
    mixed = _build(tmp_path_factory.mktemp("rp_prove_mixed_plan_for_layout"), os.path.join(os.path.dirname(SRC), "rp_prove_mixed_plan_main.cpp"))
    cases = [(nb, m, P, st, sm) for nb, m in SHAPES for P in LAYOUT_PROOFS for st, sm in LAYOUT_SEEDS]
    r = subprocess.run([exe, "layout"] + [str(x) for c in cases for x in c], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    layouts = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(layouts) == len(cases)
    up = lambda x: (x + 255) // 256 * 256
    for (nb, m, P, st, sm), L in zip(cases, layouts):
        n = nb * m
        k = n.bit_length() - 1
        assert list(L["regions"]) == list(ARRAYS)
        sizes = {"dig0": P * L["dig0_stride"], "dlen": 4 * P, "val": 32 * P * m, "gam": 32 * P * m, "tr": P * L["tr_stride"], "trlen": 4 * P, "slr": 32 * P * (2 * n + 1), "alpha": 32 * P,
                 "chal": 128 * P, "tau": 64 * P, "tsc": 128 * P, "res": 160 * P, "xs": 32 * P * k, "xr": 64 * P, "a": 32 * P * n, "b": 32 * P * n, "cg": 32 * P * n, "hf": 32 * P * n,
                 "jsc": 32 * P * (2 * n + 2), "jout": 288 * P, "pts": 64 * P * (6 + 2 * k)}
        assert {name: size for name, (_, size) in L["regions"].items()} == sizes
        assert {name: size for name, (_, size) in L["call_regions"].items()} == {"seeds": st + 16, "soff": 8 * (P + 1), "ooff": 8 * (P + 1), "out": L["total_out"] + 16}
        spans = []
        for name, (off, size) in list(L["regions"].items()) + list(L["call_regions"].items()):
            assert off % 256 == 0
            assert (off + size <= L["in_bytes"]) if name in INPUTS + ("seeds", "soff", "ooff") else (off >= L["in_bytes"]), name
            spans.append((off, off + size, name))
        spans.sort()
        for (a0, a1, an), (b0, b1, bn) in zip(spans, spans[1:]):
            assert a1 <= b0, (an, bn)
        assert spans[0][0] == 0 and spans[-1][1] <= L["need"]
        assert [name for _, _, name in spans] == list(INPUTS) + ["seeds", "soff", "ooff"] + list(ARRAYS[4:]) + ["out"]          # the order in the buffer
        # the one-class mixed plan of the same shape (capacity = the class)
        mr = subprocess.run([mixed, "plan", str(nb), str(m), "2", "0", "%d:%d:%d:%d" % (m, P, st, sm)], capture_output=True, text=True, timeout=300)
        assert mr.returncode == 0, mr.stderr[-4000:]
        mp = json.loads(mr.stdout)
        assert mp["err"] == 0 and len(mp["classes"]) == 1 and mp["total_out"] == L["total_out"]
        q = mp["classes"][0]
        assert (q["dig0_stride"], q["tr_stride"]) == (L["dig0_stride"], L["tr_stride"])
        assert sorted(q["regions"], key=lambda name: q["regions"][name][0]) == list(ARRAYS)          # (the same order)
        tables = sum(up(mp["call_regions"][t][1]) for t in ("batch", "jobs", "units"))
        assert tables > 0 and mp["in_bytes"] == L["in_bytes"] + tables and mp["need"] == L["need"] + tables
        for name in ARRAYS:
            assert q["regions"][name] == [L["regions"][name][0] + (0 if name in INPUTS else tables), L["regions"][name][1]], name
        for name in ("seeds", "soff", "ooff"):
            assert mp["call_regions"][name] == L["call_regions"][name]
        assert mp["call_regions"]["out"] == [L["call_regions"]["out"][0] + tables, L["call_regions"]["out"][1]]
