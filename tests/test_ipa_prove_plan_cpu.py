"""The plan of the batched inner-product prover (python-bulletproofs_amd/csrc/ipa_prove_plan_host.hpp) checked on the CPU: the header is
plain C++, so tests/csrc_host/ipa_prove_plan_main.cpp -- a stand-alone program -- is compiled with the host compiler (and the address
and undefined-behaviour sanitizers) and prints the plan of every vector length as JSON: block sizes, table windows, per-call caps,
error texts, the transcript bound and the base lists the kernels index."""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "csrc_host", "ipa_prove_plan_main.cpp")
INC = os.path.join(REPO, "python-bulletproofs_amd", "csrc")

SIZES = [1 << e for e in range(0, 11)]


def table_bytes(nbases, w):
    """bases x ceil(256 / w) x 2^(w-1) x 64 B"""
    return nbases * -(-256 // w) * (1 << (w - 1)) * 64


BOUND = table_bytes(3 + 2 * 128, 16)         # the range prover's largest default table (128 elements at 16 bits): what bounds the default width


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ipa_prove_plan") / "ipa_prove_plan_main")
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
def defaults(plans):
    return {p["n"]: p for p in plans([(n, 0) for n in SIZES])}


def test_block_size_and_proofs_per_block(defaults):
    assert sorted(defaults) == SIZES
    for n, p in defaults.items():
        assert p["err"] == 0 and 1 << p["k"] == n and p["nbases"] == 2 * n + 1
        assert p["NT"] == (256 if n <= 256 else n) and p["NT"] in (256, 512, 1024)
        assert p["per_block"] == p["NT"] // n and p["per_block"] * n == p["NT"]


def test_table_windows_and_bytes(defaults, plans):
    """The default width is the range prover's for n elements (16 bits up to 128; above, the widest whose 3 + 2n-base table stays within
    8.7 GB); the bytes are those of 2n + 1 bases, by the one size formula."""
    for n, p in defaults.items():
        want = 16 if n <= 128 else max(w for w in range(4, 17) if table_bytes(3 + 2 * n, w) <= BOUND)
        assert p["tw"] == want, n
        assert p["wt"] == -(-256 // want) and p["bt"] == 1 << (want - 1) and p["table_bytes"] == table_bytes(2 * n + 1, want)
    shapes = [(1024, w) for w in range(4, 17)] + [(8, 13), (4, 16), (1, 6)]
    for (n, w), p in zip(shapes, plans(shapes)):
        assert p["err"] == 0 and p["tw"] == w and p["table_bytes"] == table_bytes(2 * n + 1, w)
    # the figures the GPU tests rely on: n = 1 024 at 6 bits, n = 4 at the default 16 bits, 13 bits: 20 windows, the top one short
    assert round(table_bytes(2049, 6) / 1e6) == 180 and round(defaults[4]["table_bytes"] / 1e6) == 302
    p13 = plans([(8, 13)])[0]
    assert p13["wt"] == 20 and 256 % 13 != 0


def test_per_call_caps(defaults):
    for n, p in defaults.items():
        assert p["max_proofs"] == min(1 << 20, (1 << 27) // n)
        e = p["batch_errors"]
        assert e["1"] is None and e[str(p["max_proofs"])] is None
        assert "2^20 proofs" in e[str((1 << 20) + 1)]
        over = e[str(p["max_proofs"] + 1)]
        assert over is not None and ("2^27" in over if n > 128 else "2^20" in over)
    assert defaults[1024]["max_proofs"] == 1 << 17


def test_argument_errors(plans):
    bad = [(0, 0), (3, 0), (6, 0), (1000, 0), (2048, 0), (1 << 20, 0), (1 << 31, 0), ((1 << 32) - 1, 0)]
    for shape, p in zip(bad, plans(bad)):
        assert p["err"] != 0 and "n" not in p, shape
        assert "power of two" in p["msg"] and "1024" in p["msg"] and "single-proof prover" in p["msg"]
    for p in plans([(1, 0), (2, 0), (1024, 0)]):
        assert p["err"] == 0 and p["msg"] is None


def test_call_errors(defaults):
    for n, p in defaults.items():
        e = p["call_errors"]
        assert e["p1"] is None and e["p2"] is None
        assert e["p1_no_c"] is None                                      # c NULL: c_p = <a_p, b_p>
        assert "protocol must be 1 or 2" in e["protocol0"] and "protocol must be 1 or 2" in e["protocol3"]
        for name in ("p1_no_P", "p1_no_head", "no_a", "no_b", "no_seed_off", "no_ab", "no_transcripts", "no_tr_off"):
            assert "null argument" in e[name], name
        for name in ("p2_c", "p2_P", "p2_head"):
            assert "must be NULL under Protocol 2" in e[name], name
        for name in ("no_xs", "no_LR"):                                  # a proof of one element has no rounds: nothing to write
            assert (e[name] is None) if n == 1 else ("null argument" in e[name]), (n, name)
        s = p["seed_errors"]
        assert s["ok"] is None and s["ok_longest"] == 65535 and s["null_empty_seeds"] is None
        assert "must not decrease" in s["decreasing"] and "65535" in s["too_long"] and "null argument" in s["null_seeds"]
        c = p["cap_errors"]
        assert c["exact"] is None and "too small" in c["one_less"] and "bpmi_ipa_prove_batch_transcript_bytes" in c["one_less"]
        assert "too small" in c["zero"]


def test_job_lanes(defaults):
    """The range prover's rule: 16 lanes per job up to 128 elements; above, a wave per job up to the measured crossover."""
    for n, p in defaults.items():
        for njobs, opt, lanes in p["job_lanes"]:
            if opt:
                assert lanes == opt
            elif n <= 128:
                assert lanes == 16
            else:
                assert lanes == (64 if njobs <= p["wave_jobs_max"] else 16)


def test_base_lists(defaults):
    """The head's one term is u; every round's L and R partition the 2n generator bases (u = 0, g_j = 1 + j, h_j = 1 + n + j) and end in
    u, and the kernel's rank (j / len) * half + (i mod half) addresses every position of a list once."""
    for n, p in defaults.items():
        k, bl = p["k"], p["bases"]
        gs, hs = [1 + j for j in range(n)], [1 + n + j for j in range(n)]
        assert max(bl) <= 2 * n < 1 << 16
        assert p["off_head"] == 0 and bl[0] == 0 and p["off_round"] == 1 and len(bl) == 1 + k * 2 * (n + 1)
        for r in range(k):
            ln = n >> r
            half = ln // 2
            at = p["off_round"] + r * 2 * (n + 1)
            L, R = bl[at: at + n + 1], bl[at + n + 1: at + 2 * (n + 1)]
            assert L[n] == 0 and R[n] == 0
            assert sorted(L[:n] + R[:n]) == gs + hs
            assert L[:n // 2] == [1 + j for j in range(n) if j % ln >= half] and L[n // 2: n] == [1 + n + j for j in range(n) if j % ln < half]
            assert R[:n // 2] == [1 + j for j in range(n) if j % ln < half] and R[n // 2: n] == [1 + n + j for j in range(n) if j % ln >= half]
            hit = {"L": set(), "R": set()}
            for j in range(n):
                i = j % ln
                up = i >= half
                rank = (j // ln) * half + (i % half)
                g_list, h_list = ("L", "R") if up else ("R", "L")
                assert (L if up else R)[rank] == 1 + j and (R if up else L)[n // 2 + rank] == 1 + n + j
                hit[g_list].add(rank)
                hit[h_list].add(n // 2 + rank)
            assert hit["L"] == set(range(n)) and hit["R"] == set(range(n))


def test_transcript_bound_is_the_longest_text(defaults):
    """The bound against the longest text the Python transcript can build: every point non-identity (44 characters), every number
    78 digits (q - 1), for every base64 padding of the seed."""
    import bulletproofs_amd  # noqa: F401
    from bulletproofs_amd.ec import Point, secp256k1
    from bulletproofs_amd.utils.transcript import Transcript
    q = secp256k1.q
    assert len(str(q - 1)) == 78
    G = Point._raw(secp256k1.gx, secp256k1.gy)
    for n, p in defaults.items():
        for seed_len in (0, 1, 2, 3, 4, 200, 65535):
            outer = Transcript(b"\xff" * seed_len)
            outer.add_number(q - 1)
            for protocol, prefix in ((1, outer.digest), (2, b"x" * seed_len)):
                inner = Transcript()
                inner.digest += prefix
                for _ in range(p["k"]):
                    inner.add_list_points([G, G])
                    inner.add_number(q - 1)
                assert len(inner.digest) == p["transcript_bytes"][str(protocol)][str(seed_len)], (n, protocol, seed_len)
