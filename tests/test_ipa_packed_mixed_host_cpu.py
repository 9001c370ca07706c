"""The host twin of the preparation of packed inner-product proofs of DIFFERENT lengths (ipap::prepare_all_mixed,
python-bulletproofs_amd/csrc/ipa_packed_host.hpp; the entry point bpmi_ipa_batch_prepare_mixed runs the same functions) on the CPU:
tests/csrc_host/ipa_packed_mixed_host_main.cpp -- a stand-alone program built with the host compiler and the address and
undefined-behaviour sanitizers -- runs it over classes of proofs made by the oracle's provers at n = 1, 2, 8, 64 (make_generators is
prefix-consistent: they are statements over the prefixes of one list), and its blocks are compared with the single-class twin
(tests/csrc_host/ipa_packed_host_main.cpp), with Python integers under the seed weights of the GLOBAL index, with the value of the
weighted combination, and -- the tamper table -- with the status each mutation must give at its global index."""
import json
import os
import random
import subprocess

import pytest

import ipa_packed_ref as PR
from oracle.ec import INF

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "tests", "csrc_host")
INC = os.path.join(REPO, "python-bulletproofs_amd", "csrc")
Q = PR.Q
SEED = bytes(range(9, 41))
K = 6
NS = (2, 64, 1, 8)                      # the classes' lengths, out of order


def hx(b):
    if b is None:
        return "-"
    return bytes(b).hex() or "."


def class_arrays(pk):
    off = [0]
    for t in pk.trs:
        off.append(off[-1] + len(t))
    tr_off = b"".join(o.to_bytes(8, "little") for o in off)
    start = None if pk.starts is None else b"".join(s.to_bytes(4, "little") for s in pk.starts)
    p1 = pk.protocol == 1
    return [pk.ab, pk.xs if pk.k else None, pk.lr if pk.k else None, b"".join(pk.trs), tr_off, start, pk.u, pk.P, pk.c if p1 else None, pk.head if p1 else None]


def mixed_text(protocol, pks, weights, seed, threads=3, K_=K):
    lines = ["%d %d %d %d" % (K_, protocol, len(pks), threads), hx(weights), hx(seed)]
    for pk in pks:
        lines.append("%d %d" % (pk.k, pk.count))
        lines += [hx(a) for a in (class_arrays(pk) if pk.count else [None] * 10)]
    return "\n".join(lines)


def single_text(pk, weights, seed, threads=2):
    return "%d %d %d %d\n%s" % (pk.k, pk.protocol, pk.count, threads, "\n".join(hx(a) for a in class_arrays(pk) + [weights, seed]))


def build(tmp, name, extra=()):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", INC, os.path.join(CSRC, name + ".cpp"), "-o", exe] + list(extra))
    return exe


@pytest.fixture(scope="module")
def runners(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ipa_packed_mixed_host")
    exes = {"mixed": build(tmp, "ipa_packed_mixed_host_main"), "single": build(tmp, "ipa_packed_host_main")}

    def go(which, texts):
        r = subprocess.run([exes[which]], input="%d\n%s\n" % (len(texts), "\n".join(texts)), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        lines = [json.loads(line) for line in r.stdout.splitlines()]
        assert len(lines) == len(texts)
        return [{key: (bytes.fromhex(v) if key not in ("err", "rec_off") else v) for key, v in line.items()} for line in lines]
    return go


@pytest.fixture(scope="module")
def batches():
    """protocol -> (g, h, [Packed per class, the order of NS]); 3 proofs per class, 2 at n = 64."""
    out = {}
    for protocol in (2, 1):
        pks = []
        for n in NS:
            count = 2 if n == 64 else 3
            if protocol == 2:
                g, h, pk = PR.oracle_batch2(n, count, 500 + n, prefixes=[b"", b"one&", b"aa&bb&c&"][:count])
            else:
                g, h, pk = PR.oracle_batch1(n, count, 600 + n, [b"", b"s", b"seed-%d" % n][:count])
            pks.append(pk)
            if n == 64:
                gens = (g, h)
        out[protocol] = (gens[0], gens[1], pks)
    return out


def explicit_weights(protocol, total, seed):
    rnd = random.Random(seed)
    ws = [[rnd.randrange(1, Q) for _ in range(3 if protocol == 1 else 1)] for _ in range(total)]
    ws[0][0] = Q - 1
    return ws


def blocks(pks, got):
    """Per class: (records, points, scalars, status) cut from a mixed result through rec_off and the caller's class order."""
    out, pair, base = [], 0, 0
    for c, pk in enumerate(pks):
        pairs, rb = PR.pairs_of(pk.k, pk.protocol) * pk.count, (64 * pk.k + 96) * pk.count
        o = got["rec_off"][c]
        out.append((got["rec"][o: o + rb], got["pts"][64 * pair: 64 * (pair + pairs)], got["sc"][32 * pair: 32 * (pair + pairs)], got["status"][base: base + pk.count]))
        pair, base = pair + pairs, base + pk.count
    assert 64 * pair == len(got["pts"]) and 32 * pair == len(got["sc"]) and base == len(got["status"])
    return out


def sorted_rec_offsets(pks):
    order = sorted(range(len(pks)), key=lambda c: -pks[c].k)            # descending k, stable
    offs, at = [0] * len(pks), 0
    for c in order:
        offs[c] = at if pks[c].count else 0
        at += (64 * pks[c].k + 96) * pks[c].count
    return offs, at


def combination(g, h, pks, got):
    acc = INF
    for pk, (rec, pts, sc, _) in zip(pks, blocks(pks, got)):
        n = 1 << pk.k
        acc = acc + PR.combination(pk.k, g[:n], h[:n], rec, pts, sc, pk.count, pk.protocol)
    return acc


@pytest.mark.parametrize("protocol", [2, 1])
def test_explicit_weights_give_the_single_class_twins_bytes_per_class(runners, batches, protocol):
    g, h, pks = batches[protocol]
    total = sum(pk.count for pk in pks)
    ws = explicit_weights(protocol, total, 11 + protocol)
    (got,) = runners("mixed", [mixed_text(protocol, pks, PR.pack_weights(ws), None)])
    assert "err" not in got and got["status"] == bytes(total)
    offs, size = sorted_rec_offsets(pks)
    assert got["rec_off"] == offs and len(got["rec"]) == size
    base, texts = 0, []
    for pk in pks:
        texts.append(single_text(pk, PR.pack_weights(ws[base: base + pk.count]), None))
        base += pk.count
    singles = runners("single", texts)
    for c, (mine, want) in enumerate(zip(blocks(pks, got), singles)):
        assert mine == (want["rec"], want["pts"], want["sc"], want["status"]), c
    assert combination(g, h, pks, got) == INF


@pytest.mark.parametrize("protocol", [2, 1])
def test_seed_weights_are_derived_from_the_global_index(runners, batches, protocol):
    g, h, pks = batches[protocol]
    with_empty = pks[:2] + [PR.Packed(5, protocol)] + pks[2:]          # an empty class in the middle: skipped, it shifts no index
    got, got1 = runners("mixed", [mixed_text(protocol, with_empty, None, SEED), mixed_text(protocol, with_empty, None, SEED, threads=1)])
    assert got == got1 and got["rec_off"][2] == 0
    nw, base = 3 if protocol == 1 else 1, 0
    for pk, (rec, pts, sc, status) in zip(with_empty, blocks(with_empty, got)):
        pairs, rb = PR.pairs_of(pk.k, protocol), 64 * pk.k + 96
        assert status == bytes(pk.count)
        for i in range(pk.count):
            w = [PR.derive_weight(SEED, base + i, t) for t in range(nw)]
            want = PR.expected(pk, i, w)
            assert (rec[rb * i: rb * (i + 1)], pts[64 * pairs * i: 64 * pairs * (i + 1)], sc[32 * pairs * i: 32 * pairs * (i + 1)]) == want, (pk.k, i)
        base += pk.count


@pytest.mark.parametrize("protocol", [2, 1])
def test_one_wrong_a_is_left_to_the_group_equation(runners, batches, protocol):
    g, h, pks = batches[protocol]
    bad = [pk.clone() for pk in pks]
    PR.mut_a_changed(bad[3], 1, None)                                  # class 3 (n = 8), its proof 1
    (got,) = runners("mixed", [mixed_text(protocol, bad, None, SEED)])
    assert got["status"] == bytes(sum(pk.count for pk in pks))
    assert combination(g, h, bad, got) != INF


ROWS = [(name, protocol) for name, _, _, protocols in PR.TAMPERS for protocol in protocols]


@pytest.fixture(scope="module")
def tamper_results(runners, batches):
    """Row r of the table lands in class r mod 2 of the classes with rounds (n = 2, n = 8), proof 1; n = 1 rides along untouched."""
    rnd = random.Random(6)
    cases, texts = {}, []
    for r, (name, mut, want, protocols) in enumerate(PR.TAMPERS):
        for protocol in protocols:
            g, h, pks = batches[protocol]
            mine = [pks[0].clone(), pks[2].clone(), pks[3].clone()]          # n = 2, 1, 8
            c = (0, 2)[r % 2]
            mut(mine[c], 1, rnd)
            cases[(name, protocol)] = (g, h, mine, c, want)
            texts.append(mixed_text(protocol, mine, None, SEED))
    got = runners("mixed", texts)
    return {key: cases[key] + (g_,) for key, g_ in zip(cases, got)}


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "%s-p%d" % r)
def test_tamper_table_at_the_global_index(tamper_results, row):
    g, h, pks, c, want, got = tamper_results[row]
    bad = sum(pk.count for pk in pks[:c]) + 1
    total = sum(pk.count for pk in pks)
    assert list(got["status"]) == [(want or 0) if i == bad else 0 for i in range(total)]
    nw, base = 3 if row[1] == 1 else 1, 0
    for pk, (rec, pts, sc, status) in zip(pks, blocks(pks, got)):
        pairs, rb = PR.pairs_of(pk.k, pk.protocol), 64 * pk.k + 96
        for i in range(pk.count):
            mine = (rec[rb * i: rb * (i + 1)], pts[64 * pairs * i: 64 * pairs * (i + 1)], sc[32 * pairs * i: 32 * pairs * (i + 1)])
            if status[i]:                 # a flagged proof contributes nothing
                assert mine == (bytes(rb), bytes(64 * pairs), bytes(32 * pairs))
            else:
                assert mine == PR.expected(pk, i, [PR.derive_weight(SEED, base + i, t) for t in range(nw)])
        base += pk.count
    value = combination(g, h, pks, got)
    assert (value == INF) == bool(want)           # flagged: left out, the rest verify; silent: only the group equation rejects it


def test_argument_errors_come_from_the_plan(runners, batches):
    g, h, pks = batches[2]
    got = runners("mixed", [mixed_text(3, pks, None, SEED), mixed_text(2, pks, None, None), mixed_text(2, pks, None, SEED, K_=5),
                            mixed_text(2, [PR.Packed(3, 2)], None, SEED)])
    assert got[0] == {"err": "protocol must be 1 or 2"} and got[1] == {"err": "class 0: weights or a 32-byte seed"}
    assert got[2]["err"].startswith("class 1: k must be at most K")
    assert got[3] == {"rec": b"", "rec_off": [0], "pts": b"", "sc": b"", "status": b""}           # every class empty: nothing to do


def engine_classes(pks):
    return [(pk.k,) + pk.args() for pk in pks]


@pytest.mark.parametrize("protocol", [2, 1])
def test_the_library_entry_point_runs_the_same_code(runners, batches, protocol):
    """bpmi_ipa_batch_prepare_mixed of the built library (host code: no GPU needed) gives the bytes of the stand-alone program."""
    import bulletproofs_amd  # noqa: F401
    from bulletproofs_amd import build as B
    from bulletproofs_amd.engine import EngineError, ipa_batch_prepare_mixed_host
    B.build()
    g, h, pks = batches[protocol]
    total = sum(pk.count for pk in pks)
    wb = PR.pack_weights(explicit_weights(protocol, total, 21))
    want_w, want_s = runners("mixed", [mixed_text(protocol, pks, wb, None), mixed_text(protocol, pks, None, SEED)])
    for want, (weights, seed) in ((want_w, (wb, None)), (want_s, (None, SEED))):
        rec, offs, pts, sc, status = ipa_batch_prepare_mixed_host(K, protocol, engine_classes(pks), weights, seed, 2)
        assert (rec, offs, pts, sc, status) == (want["rec"], want["rec_off"], want["pts"], want["sc"], want["status"])
    with pytest.raises(EngineError, match="bpmi_ipa_batch_prepare_mixed: class 0: weights or a 32-byte seed"):
        ipa_batch_prepare_mixed_host(K, protocol, engine_classes(pks), None, None, 1)
    with pytest.raises(EngineError, match="bpmi_ipa_batch_prepare_mixed: class 1: k must be at most K"):
        ipa_batch_prepare_mixed_host(5, protocol, engine_classes(pks), None, SEED, 1)
    assert ipa_batch_prepare_mixed_host(K, protocol, [(3, 0, b"", b"", b"", [], None, b"", b"")], None, SEED, 1) == (b"", [0], b"", b"", b"")


def test_the_c_example_builds_against_the_header_and_the_library(tmp_path):
    """examples/ipa_prove_verify_mixed_c_abi.c is C99 over include/bpmi.h and libbpmi.so alone: it compiles without a warning and links
    (it RUNS in the GPU suite, tests/test_gpu_ipa_packed_mixed.py)."""
    import bulletproofs_amd  # noqa: F401
    from bulletproofs_amd import build as B
    B.build()
    libdir = os.path.join(REPO, "python-bulletproofs_amd")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"),
                           os.path.join(REPO, "examples", "ipa_prove_verify_mixed_c_abi.c"), "-o", str(tmp_path / "ipa_prove_verify_mixed_c_abi"),
                           os.path.join(libdir, "libbpmi.so"), "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined"])
