"""The host twin of the packed inner-product batch preparation (python-bulletproofs_amd/csrc/ipa_packed_host.hpp; the entry point
bpmi_ipa_batch_prepare runs the same functions) on the CPU: tests/csrc_host/ipa_packed_host_main.cpp -- a stand-alone program built
with the host compiler and the address and undefined-behaviour sanitizers -- runs it over proofs made by the oracle's provers
(oracle.bp_ref.ipa2_prove / ipa1_prove) at n = 1, 2, 4, 8, and its records, extra pairs and status bytes are compared with Python
integers, with the single-proof oracle verifiers on the objects built from the same bytes, and -- the tamper table -- with the
status each mutation must give."""
import json
import os
import random
import subprocess

import pytest

import ipa_packed_ref as PR
from oracle import bp_ref as R
from oracle.ec import INF

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "csrc_host", "ipa_packed_host_main.cpp")
INC = os.path.join(REPO, "python-bulletproofs_amd", "csrc")
Q = PR.Q
SEED = bytes(range(7, 39))


def hx(b):
    if b is None:
        return "-"
    return bytes(b).hex() or "."


def case_text(pk, weights, seed, threads=2):
    off = [0]
    for t in pk.trs:
        off.append(off[-1] + len(t))
    tr_off = b"".join(o.to_bytes(8, "little") for o in off)
    start = None if pk.starts is None else b"".join(s.to_bytes(4, "little") for s in pk.starts)
    p1 = pk.protocol == 1
    arrays = [pk.ab, pk.xs if pk.k else None, pk.lr if pk.k else None, b"".join(pk.trs), tr_off, start, pk.u, pk.P, pk.c if p1 else None,
              pk.head if p1 else None, weights, seed]
    return "%d %d %d %d\n%s" % (pk.k, pk.protocol, pk.count, threads, "\n".join(hx(a) for a in arrays))


# ---- the batches: valid proofs at n = 1, 2, 4, 8, both protocols; prefixes / seeds that put the SHA-256 padding edges into a round ----
def padding_prefixes():
    """Protocol 2, n = 2, a = b = 0 (every L and R is "AA=="): the first round hashes "1" "&" prefix "AA==&AA==&" = 12 + len(prefix)
    bytes -- exactly 55, 56, 63 and 64."""
    return [b"p" * (want - 13) + b"&" for want in (55, 56, 63, 64)]


def build_cases():
    cases = {}
    for n in (1, 2, 4, 8):
        k = n.bit_length() - 1
        g, h, pk = PR.oracle_batch2(n, 3, 100 + n)
        cases[("p2", n)] = (g, h, pk)
        # prefixes whose round-0 prefix ("1&" prefix L "&" R "&" = 92 + len) ends 55, 56, 63, 64 bytes into a block, and one with '&' items inside
        pre = [b"x" * ((e - 92) % 64 + 63) + b"&" for e in (55, 56, 63, 64)] + [b"aa&bb&c&"]
        g, h, pk = PR.oracle_batch2(n, len(pre), 200 + n, prefixes=pre)
        cases[("p2-prefix", n)] = (g, h, pk)
        seeds = [b"", b"s", b"seed-%d" % n, bytes(range(40))]
        g, h, pk = PR.oracle_batch1(n, len(seeds), 300 + n, seeds)
        cases[("p1", n)] = (g, h, pk)
    g, h, pk = PR.oracle_batch2(2, 4, 400, prefixes=padding_prefixes(), zero=(0, 1, 2, 3))
    cases[("p2-padding-edges", 2)] = (g, h, pk)
    return cases


def tamper_cases(cases):
    """One mutated proof (index 1) among valid ones, per row of the table and protocol; n = 4."""
    rnd = random.Random(5)
    out = {}
    for name, mut, want, protocols in PR.TAMPERS:
        for protocol in protocols:
            g, h, base = cases[("p2-prefix", 4)] if protocol == 2 else cases[("p1", 4)]
            pk = base.clone()
            mut(pk, 1, rnd)
            out[(name, protocol)] = (g, h, pk, want)
    # the last proof of the buffer truncated: no read past its end
    g, h, base = cases[("p2-prefix", 4)]
    pk = base.clone()
    pk.trs[-1] = pk.trs[-1][:-30]
    out[("last_truncated", 2)] = (g, h, pk, 1)
    return out


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ipa_packed_host") / "ipa_packed_host_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", INC, SRC, "-o", exe])

    def go(texts):
        r = subprocess.run([exe], input="%d\n%s\n" % (len(texts), "\n".join(texts)), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        lines = [json.loads(line) for line in r.stdout.splitlines()]
        assert len(lines) == len(texts)
        return [{key: (bytes.fromhex(v) if key != "err" else v) for key, v in line.items()} for line in lines]
    return go


@pytest.fixture(scope="module")
def cases():
    return build_cases()


@pytest.fixture(scope="module")
def valid_results(run, cases):
    keys = sorted(cases)
    explicit, texts = {}, []
    for key in keys:
        pk = cases[key][2]
        rnd = random.Random(sum(map(ord, key[0])) + key[1])
        explicit[key] = [[rnd.randrange(1, Q) for _ in range(3 if pk.protocol == 1 else 1)] for _ in range(pk.count)]
        explicit[key][0][0] = Q - 1
        texts.append(case_text(pk, PR.pack_weights(explicit[key]), None))
        texts.append(case_text(pk, None, SEED, threads=1))
    got = run(texts)
    return {key: (explicit[key], got[2 * i], got[2 * i + 1]) for i, key in enumerate(keys)}


def check_outputs(pk, got, weights):
    k, pairs = pk.k, PR.pairs_of(pk.k, pk.protocol)
    rb = 64 * k + 96
    for i in range(pk.count):
        rec, pts, sc = PR.expected(pk, i, weights[i])
        assert got["rec"][rb * i: rb * (i + 1)] == rec, i
        assert got["pts"][64 * pairs * i: 64 * pairs * (i + 1)] == pts, i
        assert got["sc"][32 * pairs * i: 32 * pairs * (i + 1)] == sc, i


def test_the_padding_edges_are_among_the_inputs(cases):
    pk = cases[("p2-padding-edges", 2)][2]
    hashed = [1 + len(b"&".join(t.split(b"&")[: s + 2]) + b"&") for t, s in zip(pk.trs, pk.starts)]
    assert hashed == [55, 56, 63, 64] and all(t.count(b"AA==") == 2 for t in pk.trs)
    pk = cases[("p2-prefix", 4)][2]
    assert [(1 + len(b"&".join(t.split(b"&")[: s + 2]) + b"&")) % 64 for t, s in zip(pk.trs, pk.starts)][:4] == [55, 56, 63, 0]


KEYS = [(kind, n) for n in (1, 2, 4, 8) for kind in ("p2", "p2-prefix", "p1")] + [("p2-padding-edges", 2)]


@pytest.mark.parametrize("key", KEYS, ids=lambda k_: "%s-n%d" % k_)
def test_valid_proofs_give_the_formulas_of_the_header(cases, valid_results, key):
    g, h, pk = cases[key]
    weights, got_explicit, got_seed = valid_results[key]
    for got, ws in ((got_explicit, weights), (got_seed, PR.weights_from_seed(pk, SEED))):
        assert "err" not in got
        assert got["status"] == bytes(pk.count)
        check_outputs(pk, got, ws)
    # the oracle accepts the same proofs, and the weighted combination of what the twin wrote is the identity
    assert all(PR.oracle_accepts(pk, i, g, h) for i in range(pk.count))
    assert PR.combination(pk.k, g, h, got_explicit["rec"], got_explicit["pts"], got_explicit["sc"], pk.count, pk.protocol) == INF


ROWS = [(name, protocol) for name, _, _, protocols in PR.TAMPERS for protocol in protocols] + [("last_truncated", 2)]


@pytest.fixture(scope="module")
def tamper_results(run, cases):
    tc = tamper_cases(cases)
    keys = sorted(tc)
    got = run([case_text(tc[key][2], None, SEED) for key in keys])
    return {key: (tc[key], g_) for key, g_ in zip(keys, got)}


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "%s-p%d" % r)
def test_tamper_table(tamper_results, row):
    (g, h, pk, want), got = tamper_results[row]
    status = got["status"]
    assert [i for i in range(pk.count) if status[i]] == ([1] if want else []) if row[0] != "last_truncated" else status == bytes(pk.count - 1) + b"\x01"
    bad = pk.count - 1 if row[0] == "last_truncated" else 1
    assert status[bad] == (want or 0)
    # the single-proof oracle verifier on the objects built from the same bytes: it rejects the mutated proof and only that one
    assert [PR.oracle_accepts(pk, i, g, h) for i in range(pk.count)] == [i != bad for i in range(pk.count)]
    k, pairs, rb = pk.k, PR.pairs_of(pk.k, pk.protocol), 64 * pk.k + 96
    ws = PR.weights_from_seed(pk, SEED)
    for i in range(pk.count):
        if status[i]:                 # a flagged proof contributes nothing
            assert got["rec"][rb * i: rb * (i + 1)] == bytes(rb)
            assert got["pts"][64 * pairs * i: 64 * pairs * (i + 1)] == bytes(64 * pairs) and got["sc"][32 * pairs * i: 32 * pairs * (i + 1)] == bytes(32 * pairs)
        else:
            rec, pts, sc = PR.expected(pk, i, ws[i])
            assert (got["rec"][rb * i: rb * (i + 1)], got["pts"][64 * pairs * i: 64 * pairs * (i + 1)], got["sc"][32 * pairs * i: 32 * pairs * (i + 1)]) == (rec, pts, sc)
    # the verdict of the batch: status 0 everywhere AND the combination is the identity -- false for every row
    value = PR.combination(k, g, h, got["rec"], got["pts"], got["sc"], pk.count, pk.protocol)
    if want:
        assert value == INF           # the flagged proof is left out, the rest verify
    else:
        assert value != INF           # only the group equation rejects it


def test_argument_errors_come_from_the_plan(run, cases):
    pk = cases[("p2", 2)][2]
    bad = pk.clone()
    bad.protocol = 3
    got = run([case_text(bad, None, SEED), case_text(pk, None, None)])
    assert got[0] == {"err": "protocol must be 1 or 2"} and got[1] == {"err": "weights or a 32-byte seed"}


@pytest.mark.parametrize("key", [("p2-prefix", 4), ("p1", 8), ("p2", 1)], ids=lambda k_: "%s-n%d" % k_)
def test_the_library_entry_point_runs_the_same_code(cases, valid_results, key):
    """bpmi_ipa_batch_prepare of the built library (host code: no GPU needed) gives the bytes of the stand-alone program."""
    import bulletproofs_amd  # noqa: F401
    from bulletproofs_amd import build
    from bulletproofs_amd.engine import EngineError, ipa_batch_prepare_host
    build.build()
    pk = cases[key][2]
    weights, got_explicit, got_seed = valid_results[key]
    rec, pts, sc, status = ipa_batch_prepare_host(pk.k, pk.protocol, *pk.args(), PR.pack_weights(weights), None, 2)
    assert (rec, pts, sc, status) == (got_explicit["rec"], got_explicit["pts"], got_explicit["sc"], got_explicit["status"])
    rec, pts, sc, status = ipa_batch_prepare_host(pk.k, pk.protocol, *pk.args(), None, SEED, 1)
    assert (rec, pts, sc, status) == (got_seed["rec"], got_seed["pts"], got_seed["sc"], got_seed["status"])
    with pytest.raises(EngineError, match="bpmi_ipa_batch_prepare: weights or a 32-byte seed"):
        ipa_batch_prepare_host(pk.k, pk.protocol, *pk.args(), None, None, 1)


def test_the_c_example_builds_against_the_header_and_the_library(tmp_path):
    """examples/ipa_prove_verify_c_abi.c is C99 over include/bpmi.h and libbpmi.so alone: it compiles without a warning and links (it
    RUNS in the GPU suite, tests/test_gpu_ipa_packed.py)."""
    import bulletproofs_amd  # noqa: F401
    from bulletproofs_amd import build
    build.build()
    libdir = os.path.join(REPO, "python-bulletproofs_amd")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"),
                           os.path.join(REPO, "examples", "ipa_prove_verify_c_abi.c"), "-o", str(tmp_path / "ipa_prove_verify_c_abi"),
                           os.path.join(libdir, "libbpmi.so"), "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined"])
