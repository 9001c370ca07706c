"""The plan of the batched inner-product prover's statements (bpmi_ipa_batch_prover_commit_batch) checked on the CPU: the functions
appended to python-bulletproofs_amd/csrc/ipa_prove_plan_host.hpp are plain C++, so tests/csrc_host/ipa_commit_plan_main.cpp -- a
stand-alone program -- is compiled with the host compiler (and the address and undefined-behaviour sanitizers) and prints, as JSON,
every text of ipp_commit_error and the base lists of ipp_commit_bases for every vector length 1 .. 1 024 and every NULL / u
combination, beside what ipp_plan gives for the same n: the proving plan must not have moved."""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "csrc_host", "ipa_commit_plan_main.cpp")
INC = os.path.join(REPO, "python-bulletproofs_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ipa_commit_plan") / "ipa_commit_plan_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", path])
    return path


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return [json.loads(line) for line in r.stdout.splitlines()]


@pytest.fixture(scope="module")
def lines(exe):
    out = run(exe, "bases", 1, 1024)
    assert [ln["n"] for ln in out] == list(range(1, 1025))
    return out


def test_base_lists_of_every_length_and_combination(lines):
    """g_0 .. g_(n-1) (bases 1 + j) when a is given, h_0 .. (1 + n + j) when b is, u (0) last: n (have_a + have_b) + have_u entries."""
    for ln in lines:
        n = ln["n"]
        gs, hs = [1 + j for j in range(n)], [1 + n + j for j in range(n)]
        assert sorted(ln["lists"]) == sorted("%d%d%d" % (a, b, u) for a in (0, 1) for b in (0, 1) for u in (0, 1))
        for key, got in ln["lists"].items():
            a, b, u = (ch == "1" for ch in key)
            assert got == (gs if a else []) + (hs if b else []) + ([0] if u else []), (n, key)
            assert len(got) == n * (a + b) + u and max(got, default=0) <= 2 * n < 1 << 16


def test_device_copy_holds_every_list_a_call_can_take(lines):
    """The one upload: (a, b, u), (a, u), (b, u) in a row; the list of a call is the slice at its offset, one entry short without u."""
    for ln in lines:
        n, both = ln["n"], ln["all"]
        assert both == ln["lists"]["111"] + ln["lists"]["101"] + ln["lists"]["011"] and len(both) == 4 * n + 3
        assert ln["offsets"] == {"11": 0, "10": 2 * n + 1, "01": 3 * n + 2}
        for ab in ("11", "10", "01"):
            for u in (0, 1):
                want = ln["lists"][ab + str(u)]
                at = ln["offsets"][ab]
                assert both[at: at + len(want)] == want, (n, ab, u)


def test_argument_errors(exe):
    """Every text of ipp_commit_error, in the order the entry refuses: pv, out, u_mode, t, a and b."""
    (errs,) = run(exe, "errors")
    assert len(errs) == 32 * 5
    for key, text in errs.items():
        flags, mode = key.split()
        pv, out, a, b, t = (ch == "1" for ch in flags)
        mode = int(mode)
        if not pv:
            want = "null argument (pv)"
        elif not out:
            want = "null argument (out)"
        elif mode not in (0, 1, 2):
            want = "u_mode must be 0"
        elif mode != 2 and t:
            want = "t must be NULL unless u_mode is 2"
        elif mode == 2 and not t:
            want = "u_mode 2 takes t"
        elif not a and not b:
            want = "a and b are both NULL"
        elif mode == 1 and not (a and b):
            want = "u_mode 1 sums <a, b>: it takes both a and b"
        else:
            want = None
        if want is None:
            assert text is None, key
        else:
            assert text is not None and want in text, (key, text)
    # the accepted calls, spelled out: NIProver's statement, FastNIProver2's, explicit t, and each NULL half under modes 0 and 2
    for key in ("11110 0", "11110 1", "11111 2", "11100 0", "11010 0", "11101 2", "11011 2"):
        assert errs[key] is None, key


def test_the_proving_plan_is_unchanged(lines):
    """ipp_plan's base lists by their own rule (tests/test_ipa_prove_plan_cpu.py pins the rest): 1 + 2k(n + 1) entries, the head's u, then
    every round's L and R."""
    seen = []
    for ln in lines:
        n = ln["n"]
        if n & (n - 1):
            assert "plan" not in ln
            continue
        seen.append(n)
        p = ln["plan"]
        k = n.bit_length() - 1
        assert p["err"] == 0 and p["k"] == k and p["nbases"] == 2 * n + 1 and p["NT"] == (256 if n <= 256 else n) and p["per_block"] == p["NT"] // n
        assert p["max_proofs"] == min(1 << 20, (1 << 27) // n) and p["off_head"] == 0 and p["off_round"] == 1
        want = [0]
        for r in range(k):
            ln_r = n >> r
            half = ln_r // 2
            for side in (0, 1):
                want += [1 + j for j in range(n) if (j % ln_r >= half) == (side == 0)]
                want += [1 + n + j for j in range(n) if (j % ln_r < half) == (side == 0)]
                want.append(0)
        assert p["bases"] == want and len(p["bases"]) == 1 + 2 * k * (n + 1)
    assert seen == [1 << e for e in range(11)]
