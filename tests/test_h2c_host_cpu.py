"""The bulk hash to the curve checked on the CPU: python-bulletproofs_amd/csrc/h2c.hpp -- the bodies the kernels run -- is plain C++,
so tests/csrc_host/h2c_host_main.cpp, a stand-alone program, is compiled with the host compiler (once plainly, once under the address
and undefined-behaviour sanitizers) and driven through a command file: the block feeder of both hashes against hashlib at every
padding edge, the candidate body on digests no real message produces, and the whole function against the oracle's elliptic_hash."""
import hashlib
import os
import subprocess

import pytest

import h2c_ref
from h2c_ref import P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "csrc_host", "h2c_host_main.cpp")
INC = os.path.join(REPO, "python-bulletproofs_amd", "csrc")

# total lengths (prefix + message) at the padding edges of both hashes: one block up to 55 bytes, two up to 119, three from 120
TOTALS = [0, 1, 54, 55, 56, 57, 63, 64, 65, 118, 119, 120, 121, 1000]
# (counter or 0 for no prefix at all, range-form index or None)
PREFIXES = [(0, None), (7, None), (42, None), (255, None), (1, 0), (3, 9), (10, 10), (2, 99999), (113, 2**32 - 1)]


def prefix_bytes(c, idx):
    return (b"%d" % c if c else b"") + (b"%d" % idx if idx is not None else b"")


def hx(b):
    return b.hex() if b else "-"


def feeder_cases():
    cases = []
    for total in TOTALS:
        for c, idx in PREFIXES:
            pre = prefix_bytes(c, idx)
            if len(pre) > total:
                continue
            msg = bytes((37 * k + total) & 0xFF for k in range(total - len(pre)))
            cases.append(("F %d %d %d %s" % (c, idx is not None, idx or 0, hx(msg)), pre + msg))
    return cases


def candidate_expect(x, bit):
    """what Python integers decide for the digest x: (accepted, 64 wire bytes)"""
    if x >= P:
        return 0, h2c_ref.IDENTITY
    rhs = (x**3 + 7) % P
    r = pow(rhs, (P + 1) // 4, P)
    if r * r % P != rhs:
        return 0, h2c_ref.IDENTITY
    return 1, x.to_bytes(32, "little") + (r if bit else P - r).to_bytes(32, "little")


def candidate_cases():
    residue = next(x for x in range(2, 100) if candidate_expect(x, 1)[0])
    non_residue = next(x for x in range(2, 100) if not candidate_expect(x, 1)[0])
    xs = [P, P + 1, 2**256 - 1, P - 1, 0, residue, non_residue, 2**255 + 12345, P - 2**32]
    return [(x, bit) for x in xs for bit in (0, 1)], residue, non_residue


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("h2c_host")
    plain, san = str(d / "h2c_host_main"), str(d / "h2c_host_main_san")
    common = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-misleading-indentation", "-I", INC, SRC]
    subprocess.check_call(common + ["-O2", "-o", plain])
    subprocess.check_call(common + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", san])

    def run(exe, lines):
        path = str(d / "commands.txt")
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
        r = subprocess.run([plain if exe == "plain" else san, path], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        return r.stdout.splitlines()
    return run


def parse_points(lines):
    """lines '<tries or accepted> <128 hex>' -> ([numbers], [64 bytes])"""
    return [int(ln.split()[0]) for ln in lines], [bytes.fromhex(ln.split()[1]) for ln in lines]


def test_feeders_at_the_padding_edges(programs):
    cases = feeder_cases()
    assert {len(text) for _, text in cases} == set(TOTALS)
    out = programs("plain", [line for line, _ in cases])
    assert len(out) == len(cases)
    for (line, text), got in zip(cases, out):
        assert got == hashlib.sha256(text).hexdigest() + " " + hashlib.md5(text).hexdigest(), line[:40]


def test_candidate_body_called_directly(programs):
    cases, residue, non_residue = candidate_cases()
    out = programs("plain", ["C %064x %d" % c for c in cases])
    ok, pts = parse_points(out)
    for (x, bit), a, pt in zip(cases, ok, pts):
        assert (a, pt) == candidate_expect(x, bit), (hex(x), bit)
    verdict = {c: a for c, a in zip(cases, ok)}
    for x in (P, P + 1, 2**256 - 1):
        assert verdict[(x, 0)] == 0 and verdict[(x, 1)] == 0               # x >= p: rejected whatever x^3 + 7 is
    assert verdict[(residue, 0)] == 1 and verdict[(non_residue, 1)] == 0
    both = {bit: pts[cases.index((residue, bit))] for bit in (0, 1)}
    y0, y1 = (int.from_bytes(both[b][32:], "little") for b in (0, 1))
    assert y0 != y1 and y0 + y1 == P and y1 == pow(residue**3 + 7, (P + 1) // 4, P)     # bit 1 keeps the root the exponentiation returns


def test_whole_function_on_the_reference_outputs(programs, golden):
    """the ten messages of hash_codec.json: the reference's own outputs, and the oracle's"""
    rows = golden("hash_codec.json")["elliptic_hash"]
    assert len(rows) == 10
    out = programs("plain", ["H 255 0 0 %s" % (m or "-") for m, _ in rows])
    tries, pts = parse_points(out)
    for (m, (x, y)), t, pt in zip(rows, tries, pts):
        assert pt == int(x, 16).to_bytes(32, "little") + int(y, 16).to_bytes(32, "little")
        assert (pt, t) == h2c_ref.oracle_one(bytes.fromhex(m))


def test_whole_function_on_4096_messages(programs):
    want_pts, want_tries = h2c_ref.gs_set()
    tries, pts = parse_points(programs("plain", ["R 255 0 4096 " + b"gs".hex()]))
    assert tries == want_tries and pts == want_pts
    assert max(tries) == 13 and [i for i, t in enumerate(tries) if t >= 10] == [1397, 1616, 2521, 3041]


def test_max_tries_one(programs):
    """exactly the messages whose first candidate fails report tries = 0 and an identity"""
    want_pts, want_tries = h2c_ref.gs_set()
    tries, pts = parse_points(programs("plain", ["R 1 0 4096 " + b"gs".hex()]))
    assert tries == [1 if t == 1 else 0 for t in want_tries]
    assert pts == [p if t == 1 else h2c_ref.IDENTITY for p, t in zip(want_pts, want_tries)]
    assert tries.index(0) == 2                                              # "2gs" is the first message that needs a second candidate


def test_same_answers_under_the_sanitizers(programs):
    """the same program built with -fsanitize=address,undefined, run as a program: every kind of command, a clean exit, the same lines"""
    cand, _, _ = candidate_cases()
    lines = [line for line, _ in feeder_cases()] + ["C %064x %d" % c for c in cand]
    lines += ["H 255 0 0 " + hx(m) for m in (b"", b"test", b"x" * 200)] + ["H 3 1 1616 " + b"gs".hex()]
    lines += ["R 255 1390 1400 " + b"gs".hex(), "R 1 0 64 " + b"gs".hex(), "R 255 999990 1000010 " + hx(b"s" * 60), "R 255 4294967290 4294967296 -"]
    assert programs("san", lines) == programs("plain", lines)


def test_abi_names():
    """the four entry points are in the header and in the binding table; nothing of the host twin is part of the product"""
    import bulletproofs_amd  # noqa: F401
    from bulletproofs_amd import _native
    names = ["bpmi_ec_hash_batch", "bpmi_ec_hash_batch_dev", "bpmi_ec_hash_range", "bpmi_ec_hash_range_dev"]
    header = open(os.path.join(REPO, "include", "bpmi.h")).read()
    for name in names:
        assert name in _native.SIGNATURES and name + "(" in header
    assert "src/utils/elliptic_curve_hash.py:7-23" in header and "NOT by the parity of y" in header
    assert sorted(n for n in _native.SIGNATURES if "hash" in n and "mod_hash" not in n) == sorted(names)
