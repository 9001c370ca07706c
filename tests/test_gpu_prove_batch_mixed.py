"""GPU parity of the batched range-proof prover over CLASSES of different sizes in one call (MixedBatchRangeProver,
bpmi_rp_prove_batch_mixed; csrc/rp_prove_mixed_kernels.hpp): a prover created for (bits, M) is a capacity, a class of m values per proof
runs over the first bits x m of its generators.  Every proof must be byte for byte what a prover created over that prefix writes --
BatchRangeProver(bits, g, h, gs[:n_c], hs[:n_c], u, m=m_c) -- and what the single-proof provers write
(/root/reference/src/rangeproofs/rangeproof_aggreg_prover.py:36-146, rangeproof_prover.py:35-91 behind the product's call surface): the
reference's own goldens of two sizes from one table, a block over every block size with unsorted and repeated classes, short rounds,
degenerate generators, the way through MixedBatchRangeVerifier, the argument errors, and the C example.

Every table is built under prover_table_bits = 6 (1 024 elements: 180 MB)."""
import ctypes
import os
import subprocess

import pytest

from conftest import load_golden
from helpers import Q
from test_gpu_prove_batch_wide import _rows

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = [(4, 3), (1, 65), (128, 2), (32, 1), (64, 2), (1, 2)]          # capacity (8, 128): (m, proofs) -- unsorted, m = 1 twice, 65 proofs in one class


@pytest.fixture(scope="module")
def gp():
    import gpu_common
    return gpu_common


_GENS = {}


def _gens(gp, elems):
    """g, h, gs, hs, u of a capacity of `elems` elements (made once per size)."""
    if elems not in _GENS:
        pts = gp.to_gpu_list(gp.rand_points(2 * elems + 3, 7700 + elems)[0])
        _GENS[elems] = (pts[0], pts[1], pts[3:3 + elems], pts[3 + elems:], pts[2])
    return _GENS[elems]


def _with_table_bits(gp, make, bits=6):
    eng = gp.engine()
    try:
        eng.set_option("prover_table_bits", bits)
        return make()
    finally:
        eng.set_option("prover_table_bits", 0)


def _mixed(gp, nb, gens, **kw):
    from bulletproofs_amd.rangeproofs import MixedBatchRangeProver
    g, h, gs, hs, u = gens
    return _with_table_bits(gp, lambda: MixedBatchRangeProver(nb, g, h, gs, hs, u, **kw))


def _prefix_proofs(gp, nb, gens, classes, formats=(2,)):
    """What the existing path writes: per class BatchRangeProver over the class's prefix -> {format: [the class's wire proofs]}."""
    from bulletproofs_amd.rangeproofs import BatchRangeProver
    g, h, gs, hs, u = gens
    want = {f: [] for f in formats}
    for m, vss, gss, seeds in classes:
        n = nb * m
        bp = _with_table_bits(gp, lambda: BatchRangeProver(nb, g, h, gs[:n], hs[:n], u, m=m))
        try:
            for f in formats:
                bp.wire_format = f
                want[f].append(bp.prove_wire(vss, gss, seeds))
        finally:
            bp.close()
    return want


def _split(result):
    return [[bytes(packed[offs[i]: offs[i + 1]]) for i in range(len(offs) - 1)] for _, packed, offs in result]


def _first_difference(got, want):
    for c, (a, b) in enumerate(zip(got, want)):
        if a != b:
            i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            return "class %d: proof %d of %d / %d differs" % (c, i, len(a), len(b))
    return None if len(got) == len(want) else "%d classes for %d" % (len(got), len(want))


@pytest.fixture(scope="module")
def block(gp):
    """The block of capacity (8, 128) and what the existing path proves for it, computed once: the generators, the classes
    (m, values, blinding factors, seeds) with the rows of the wide test -- zeros, all ones, an out-of-range value, zero blinding, seeds of
    0 / 1 / 300 bytes --, per class the indices of its out-of-range proofs, and the prefix provers' proofs in wire formats 2 and 3."""
    gens = _gens(gp, 1024)
    classes, bad = [], []
    for c, (m, count) in enumerate(BLOCK):
        vss, gss, seeds, b = _rows(8, m, count, c)
        classes.append((m, vss, gss, seeds))
        bad.append({i for i in range(count) if int(vss[i][m - 1].x) >= 1 << 8})          # (_rows names only the last one)
        assert (b is None) == (not bad[-1]) and (b is None or b == max(bad[-1]))
    return gens, classes, bad, _prefix_proofs(gp, 8, gens, classes, formats=(2, 3))


def test_one_call_reproduces_two_reference_goldens_from_one_table(gp):
    """tests/golden/rangeproofs.json, made by the reference itself: the aggregated cases (4 x 16 bits) and (32 x 16 bits) share their
    seeds, so the 64 generators of the first are a prefix of the 512 of the second.  One prover (16, 32), one call with the classes
    m = 4 and m = 32, each golden twice in its class: both goldens' fields."""
    from bulletproofs_amd.rangeproofs import proofs_from_bytes
    from bulletproofs_amd.utils import ModP, mod_hash
    from test_gpu_rangeproofs import check_range_proof, inputs
    small, big = load_golden("rangeproofs.json")["aggregated"][0], load_golden("rangeproofs.json")["aggregated"][2]
    assert (small["n"], small["m"], big["n"], big["m"]) == (16, 4, 16, 32) and small["seeds"] == big["seeds"]
    s, n, gs, hs, g, h, u = inputs(gp, big, 32)
    s4, _, gs4, hs4, _, _, _ = inputs(gp, small, 4)
    assert all(gp.same_point(a, b) for a, b in zip(gs4 + hs4, gs[:64] + hs[:64]))
    classes = []
    for c in (small, big):
        vs = [ModP(int(v, 16), Q) for v in c["vs"]]
        gammas = [mod_hash(str(j).encode() + s[5], Q) for j in range(c["m"])]
        classes.append((c["m"], [vs, vs], [gammas, gammas], [s[6], s[6]]))
    mp = _mixed(gp, 16, (g, h, gs, hs, u))
    try:
        out = mp.prove_classes_packed(classes)
        Vs = mp.commit(classes[0][1][:1], classes[0][2][:1])
    finally:
        mp.close()
    assert [n_c for n_c, _, _ in out] == [64, 512]
    for blobs, c in zip(_split(out), (small, big)):
        assert len(blobs) == 2
        for pr in proofs_from_bytes(blobs, engine=gp.engine()):
            check_range_proof(gp, pr, c["proof"])
    from helpers import P
    assert len(Vs) == 1 and all(gp.same_point(V, P(w)) for V, w in zip(Vs[0], small["Vs"]))


def test_block_equals_the_prefix_provers_under_every_lane_width_and_format(gp, block):
    """Capacity (8, 128): n_c runs 8 .. 1 024 over all three block sizes, per_block from 32 down to 1; the 65 proofs make a 64-lane chain
    unit and a job block straddle.  Every proof equals the prefix prover's, byte for byte, under prover_job_lanes 0 / 16 / 64 and in wire
    format 3; a second call on the same prover with other classes (fewer, in another order, other counts) sees no stale state."""
    from bulletproofs_amd.rangeproofs.codec import wire_v3_to_v2
    gens, classes, _, want = block
    eng = gp.engine()
    mp = _mixed(gp, 8, gens)
    try:
        got = {}
        for lanes in (0, 16, 64):
            eng.set_option("prover_job_lanes", lanes)
            got[lanes] = mp.prove_classes_packed(classes)
        eng.set_option("prover_job_lanes", 0)
        ms = mp.last_ms()
        # other classes on the same prover: the 1 024-element class alone first, then 3 of the 65, then the 512-element class's last proof
        cut = lambda c, lo, hi: (classes[c][0], classes[c][1][lo:hi], classes[c][2][lo:hi], classes[c][3][lo:hi])
        again = mp.prove_classes_packed([cut(2, 1, 2), cut(1, 61, 64), cut(4, 1, 2)])
        mp.wire_format = 3
        v3 = mp.prove_classes_packed(classes)
        mp.wire_format = 2
        after = mp.prove_classes_packed([cut(0, 0, 3)])
    finally:
        eng.set_option("prover_job_lanes", 0)
        mp.close()
    assert [n_c for n_c, _, _ in got[0]] == [8 * m for m, _ in BLOCK]
    for lanes in (0, 16, 64):
        assert _first_difference(_split(got[lanes]), want[2]) is None, lanes
    assert _first_difference(_split(v3), want[3]) is None
    assert [[wire_v3_to_v2(b) for b in cls] for cls in _split(v3)] == want[2]
    assert _split(again) == [want[2][2][1:2], want[2][1][61:64], want[2][4][1:2]] and [n_c for n_c, _, _ in again] == [1024, 8, 512]
    assert _split(after) == [want[2][0]]
    assert set(ms) == {"A_S", "yz_T1_T2", "x_vectors_Pnew", "ipa_rounds", "wire_bytes", "copy_out", "total"} and ms["total"] > 0
    assert all(v >= 0 for v in ms.values()) and ms["total"] >= ms["ipa_rounds"] > 0


def test_block_equals_the_single_proof_provers(gp, block):
    """Two proofs per class against proof_to_bytes(AggregNIRangeProver(..).prove()) over the class's prefix -- NIRangeProver for m = 1 --
    compared with the bytes the prefix provers gave (which the test above pins the mixed call to)."""
    from bulletproofs_amd.ec import secp256k1
    from bulletproofs_amd.rangeproofs import AggregNIRangeProver, NIRangeProver, proof_to_bytes
    (g, h, gs, hs, u), classes, _, want = block
    mp = _mixed(gp, 8, (g, h, gs, hs, u))
    try:
        got = _split(mp.prove_classes_packed(classes))
    finally:
        mp.close()
    for c, (m, vss, gss, seeds) in enumerate(classes):
        n = 8 * m
        for i in sorted({0, len(vss) - 1}):
            if m == 1:
                pr = NIRangeProver(vss[i][0], 8, g, h, gs[:n], hs[:n], gss[i][0], u, secp256k1, seeds[i]).prove()
            else:
                pr = AggregNIRangeProver(vss[i], 8, g, h, gs[:n], hs[:n], gss[i], u, secp256k1, seeds[i]).prove()
            assert got[c][i] == proof_to_bytes(pr, version=2), (c, i)


@pytest.mark.parametrize("nb,M,ms", [(2, 4, (1, 2, 4)), (1, 2, (2,))])
def test_short_rounds(gp, nb, M, ms):
    """Capacity (2, 4) with the classes n_c = 2, 4, 8 (one, two and three rounds: a class leaves the rounds beyond its own out), and
    capacity (1, 2) with its single class n_c = 2."""
    gens = tuple(x[:nb * M] if isinstance(x, list) else x for x in _gens(gp, 8))
    classes = []
    for c, m in enumerate(ms):
        vss, gss, seeds, _ = _rows(nb, m, 5 + c, c)
        classes.append((m, vss, gss, seeds))
    want = _prefix_proofs(gp, nb, gens, classes, formats=(2, 3))
    mp = _mixed(gp, nb, gens)
    try:
        got = mp.prove_classes_packed(classes)
        mp.wire_format = 3
        v3 = mp.prove_classes_packed(classes)
    finally:
        mp.close()
    assert [n_c for n_c, _, _ in got] == [nb * m for m in ms]
    assert _first_difference(_split(got), want[2]) is None and _first_difference(_split(v3), want[3]) is None


def test_a_single_class_of_the_capacity_equals_the_single_class_call(gp):
    """One class with m = M: the mixed call and bpmi_rp_prove_batch on the SAME prover write the same bytes, in either order."""
    gens = tuple(x[:64] if isinstance(x, list) else x for x in _gens(gp, 1024))
    vss, gss, seeds, _ = _rows(16, 4, 9, 1)
    mp = _mixed(gp, 16, gens)
    try:
        first = mp._bp.prove_wire(vss, gss, seeds)
        got = mp.prove_classes_packed([(4, vss, gss, seeds)])
        second = mp._bp.prove_wire(vss, gss, seeds)
        nothing = mp.prove_classes_packed([])
    finally:
        mp.close()
    assert _split(got) == [first] and second == first and nothing == []


def test_calls_of_every_kind_share_one_prover(gp):
    """One prover of capacity (8 bits, M = 4), at most 70 proofs per call (per_block 32 .. 8, a chain block is crossed at 65), takes in
    turn: bpmi_rp_prove_batch of 3 proofs with seeds of 0, 1 and 100 bytes; a mixed call of m = 1 x 65 and m = 4 x 2;
    bpmi_rp_prover_commit_batch of 5 pairs; bpmi_rp_prove_batch of 70 proofs, for which both of its buffers grow; the first call again.
    Every result is what a fresh prover gives for that call alone, the first and the last are identical, a pageable `out` gives the
    bytes of the page-locked one, and after each proving call last_ms holds seven finite non-negative values whose last is at least each
    other.  Under option prover_split a single-class call of 4 proofs gives the same bytes: 1 (halves of at least 2 048: not split),
    and 2 (split into 2 + 2)."""
    import math
    from bulletproofs_amd.rangeproofs.batch_prover import pack_pairs, seed_offsets
    gens = tuple(x[:32] if isinstance(x, list) else x for x in _gens(gp, 1024))
    eng = gp.engine()
    v3, g3, _, _ = _rows(8, 4, 3, 0)
    s3 = [b"", b"\x07", bytes(range(100))]
    v65, g65, s65, _ = _rows(8, 1, 65, 1)
    v2, g2, s2, _ = _rows(8, 4, 2, 2)
    v70, g70, s70, _ = _rows(8, 4, 70, 3)
    cv, cg, _, _ = _rows(8, 1, 5, 4)
    calls = [lambda p: p._bp.prove_wire(v3, g3, s3),
             lambda p: _split(p.prove_classes_packed([(1, v65, g65, s65), (4, v2, g2, s2)])),
             lambda p: p.commit_packed(cv, cg),
             lambda p: p._bp.prove_wire(v70, g70, s70),
             lambda p: p._bp.prove_wire(v3, g3, s3)]

    def timed(p):
        ms = list(p.last_ms().values())
        assert len(ms) == 7 and all(math.isfinite(v) and v >= 0 for v in ms) and ms[6] == max(ms) and ms[6] > 0, ms

    want = []
    for call in calls[:4]:
        fresh = _mixed(gp, 8, gens)
        try:
            want.append(call(fresh))
        finally:
            fresh.close()
    want.append(want[0])
    mp = _mixed(gp, 8, gens)
    try:
        got = []
        for i, call in enumerate(calls):
            got.append(call(mp))
            if i != 2:
                timed(mp)
        # the first call once more, into ordinary memory
        vb, gb, count = pack_pairs(v3, g3, 4)
        sb, off = seed_offsets(s3, count)
        cap = sum(len(b) for b in want[0])
        out, out_off = ctypes.create_string_buffer(cap), (ctypes.c_uint64 * (count + 1))()
        eng._ck(eng.lib.bpmi_rp_prove_batch(mp._bp._handle, count, vb, gb, sb, off, ctypes.cast(out, ctypes.c_void_p), cap, out_off))
        timed(mp)
        pageable = [out.raw[out_off[i]: out_off[i + 1]] for i in range(count)]
        split = {}
        for opt in (1, 2):
            eng.set_option("prover_split", opt)
            split[opt] = mp._bp.prove_wire(v70[:4], g70[:4], s70[:4])
            timed(mp)
    finally:
        eng.set_option("prover_split", 0)
        mp.close()
    assert len(got[0]) == 3 and [len(c) for c in got[1]] == [65, 2] and len(got[2]) == 64 * 5 and len(got[3]) == 70
    for i in range(5):
        assert got[i] == want[i], i
    assert got[4] == got[0] and pageable == got[0]
    assert split[1] == want[3][:4] and split[2] == want[3][:4]


def test_degenerate_generators_inside_the_shortest_prefix(gp):
    """A capacity list with an identity (gs_1) and a coinciding pair (hs_0 = gs_0) inside the shortest prefix, and hs_5 = -gs_5 in the next:
    every class still equals the prover over its prefix, which tests/test_gpu_rp_degenerate.py pins to the integer model."""
    from bulletproofs_amd.ec import Point
    g, h, gs, hs, u = _gens(gp, 1024)
    gs, hs = list(gs[:64]), list(hs[:64])
    assert isinstance(gs[5], Point)
    gs[1] = Point.IDENTITY_ELEMENT
    hs[0] = gs[0]
    hs[5] = -gs[5]
    gens = (g, h, gs, hs, u)
    classes = []
    for c, m in enumerate((8, 1, 2)):
        vss, gss, seeds, _ = _rows(8, m, 4, c)
        classes.append((m, vss, gss, seeds))
    want = _prefix_proofs(gp, 8, gens, classes, formats=(2, 3))
    mp = _mixed(gp, 8, gens)
    try:
        got = mp.prove_classes_packed(classes)
        mp.wire_format = 3
        v3 = mp.prove_classes_packed(classes)
    finally:
        mp.close()
    assert _first_difference(_split(got), want[2]) is None and _first_difference(_split(v3), want[3]) is None


def test_through_the_mixed_verifier(gp, block):
    """prove_classes_packed + commit_packed are the class tuples of MixedBatchRangeVerifier.partial_packed: 64 zero bytes without the
    out-of-range rows; with them the value is not the identity and locate_wire(items, group=None) names exactly them; prove_wire(items)
    returns the proofs in the items' order."""
    from bulletproofs_amd.ec import Point
    from bulletproofs_amd.rangeproofs import MixedBatchRangeVerifier
    gens, classes, bad, want = block
    g, h, gs, hs, u = gens
    assert [len(b) for b in bad] == [0, 13, 1, 1, 0, 0]
    keep = lambda xs, b: [x for i, x in enumerate(xs) if i not in b]
    good = [(m, keep(vss, b), keep(gss, b), keep(seeds, b)) for (m, vss, gss, seeds), b in zip(classes, bad) if len(vss) > len(b)]
    mp = _mixed(gp, 8, gens)
    bv = MixedBatchRangeVerifier(g, h, gs, hs, u)
    try:
        tuples = lambda cls: [(n_c, mp.commit_packed(vss, gss), packed, offs) for (n_c, packed, offs), (_, vss, gss, _) in zip(mp.prove_classes_packed(cls), cls)]
        assert bv.partial_packed(tuples(good)) == bytes(64)
        assert bv.partial_packed(tuples(classes)) != bytes(64)
        # items in an order that interleaves the classes; the value lists say the size
        items, where = [], []
        for c, (m, vss, gss, seeds) in enumerate(classes):
            for i in range(len(vss)):
                items.append((vss[i], gss[i], seeds[i]))
                where.append((c, i))
        order = sorted(range(len(items)), key=lambda j: (j * 37) % len(items))
        items, where = [items[j] for j in order], [where[j] for j in order]
        blobs = mp.prove_wire(items)
        assert blobs == [want[2][c][i] for c, i in where]
        Vs = mp.commit([v for v, _, _ in items], [gm for _, gm, _ in items])
        assert all(isinstance(V, Point) for row in Vs for V in row) and [len(row) for row in Vs] == [len(v) for v, _, _ in items]
        named = bv.locate_wire([(row if len(row) > 1 else row[0], blob) for row, blob in zip(Vs, blobs)], group=None)
        assert named == sorted(j for j, (c, i) in enumerate(where) if i in bad[c]) and len(named) == 15
    finally:
        bv.release()
        mp.close()


def _raw(eng, handle, specs, cap=None, out=True, out_off=True, n_classes=None, arr=True):
    """bpmi_rp_prove_batch_mixed on raw buffers.  specs: (m, n_proofs, values, gammas, seeds, seed_off) with bytes / a list of offsets /
    None.  out and out_off are poisoned; returns (rc, message, out bytes, out_off list, poison byte)."""
    from bulletproofs_amd import _native
    keep = []
    a = (_native.RpProveClass * max(len(specs), 1))()

    def addr(b):
        if b is None:
            return None
        buf = ctypes.create_string_buffer(bytes(b), max(len(b), 1))
        keep.append(buf)
        return ctypes.addressof(buf)
    total = 0
    for c, (m, count, values, gammas, seeds, off) in enumerate(specs):
        a[c].m, a[c].n_proofs = m, count
        a[c].values, a[c].gammas, a[c].seeds = addr(values), addr(gammas), addr(seeds)
        if off is not None:
            o = (ctypes.c_uint64 * len(off))(*off)
            keep.append(o)
            a[c].seed_off = ctypes.addressof(o)
        total += count if count < 1 << 21 else 0
    size = cap if cap is not None else 1 << 16
    obuf = (ctypes.c_char * max(size, 64)).from_buffer_copy(b"\xa5" * max(size, 64))
    ooff = (ctypes.c_uint64 * (min(total, 1 << 12) + 2))(*([0xA5A5A5A5A5A5A5A5] * (min(total, 1 << 12) + 2)))
    rc = eng.lib.bpmi_rp_prove_batch_mixed(handle, len(specs) if n_classes is None else n_classes, ctypes.cast(a, ctypes.c_void_p) if arr else None,
                                           ctypes.cast(obuf, ctypes.c_void_p) if out else None, size, ctypes.cast(ooff, ctypes.c_void_p) if out_off else None)
    msg = eng.lib.bpmi_last_error(eng.ctx)
    return rc, (msg.decode() if isinstance(msg, bytes) else str(msg)), obuf.raw, list(ooff)


def test_argument_errors_leave_the_output_untouched(gp):
    """Every rule of the plan, NULL arrays, decreasing seed offsets, a 65 536-byte seed, a cap one byte short, a value and a blinding
    factor equal to q in the second class: BPMI_E_ARG with a message naming the cause, `out` and `out_off` as they were.  The caps are
    tested with counts alone and tiny buffers: nothing is read beyond them.  n_classes = 0 is BPMI_OK with out_off[0] = 0."""
    E_ARG = -3                                            # BPMI_E_ARG (include/bpmi.h)
    eng = gp.engine()
    eng.set_option("prover_wire_format", 2)
    gens = _gens(gp, 1024)
    mp = _mixed(gp, 8, gens)
    tiny = _mixed(gp, 1, tuple(x[:2] if isinstance(x, list) else x for x in gens))
    one, z = bytes(32), [0, 0]
    qle = Q.to_bytes(32, "little")
    ok = lambda m, count: (m, count, bytes(32 * m * count), bytes(32 * m * count), b"", [0] * (count + 1))
    try:
        h8, h1 = mp._bp._handle, tiny._bp._handle
        fixed = eng.lib.bpmi_rp_prove_batch_proof_bytes_class
        assert fixed(h8, 3, 0) == 0 and fixed(h8, 256, 0) == 0 and fixed(h1, 1, 0) == 0
        assert fixed(h8, 1, 7) == 6 + 32 * 8 + 33 * 12 + 132 + 7 and fixed(h8, 128, 0) == 6 + 32 * 15 + 33 * 26 + 132 and fixed(h1, 2, 0) == 6 + 32 * 6 + 33 * 8 + 132
        cases = [
            (h8, [(3, 1, one, one, b"", z)], {}, "class 0: the number of values must be a power of two"),
            (h8, [ok(1, 1), (256, 1, one, one, b"", z)], {}, "class 1: the number of values must be a power of two, at most the prover's"),
            (h8, [(0, 1, one, one, b"", z)], {}, "class 0: the number of values"),
            (h1, [(1, 1, one, one, b"", z)], {}, "bits x values >= 2"),
            (h8, [ok(4, 2), (4, 0, one, one, b"", z)], {}, "class 1: n_proofs must be at least 1"),
            (h8, [(1, 1, one, one, b"", z)] * 65, {}, "n_classes must be at most 64"),
            (h8, [(1, 1 << 19, one, one, b"", z), (2, 1 << 19, one, one, b"", z), (1, 1, one, one, b"", z)], {"cap": 16}, r"at most 2^20 proofs"),
            (h8, [(1, (1 << 20) + 1, one, one, b"", z)], {"cap": 16}, "at most 2^20 proofs"),
            (h8, [(128, 1 << 16, one, one, b"", z), (64, 1 << 17, one, one, b"", z), (1, 1, one, one, b"", z)], {"cap": 16}, "at most 2^27 elements"),
            (h8, [(128, (1 << 17) + 1, one, one, b"", z)], {"cap": 16}, "at most 2^27 elements"),
            (h8, [ok(1, 2), (2, 1, None, bytes(64), b"", z)], {}, "class 1: null argument"),
            (h8, [ok(1, 2), (2, 1, bytes(64), None, b"", z)], {}, "class 1: null argument"),
            (h8, [(2, 1, bytes(64), bytes(64), b"", None)], {}, "class 0: null argument"),
            (h8, [(2, 1, bytes(64), bytes(64), None, [0, 3])], {}, "class 0: null argument"),
            (h8, [ok(1, 2)], {"out": False}, "null argument"),
            (h8, [ok(1, 2)], {"out_off": False}, "null argument"),
            (h8, [ok(1, 2)], {"arr": False}, "null argument"),
            (h8, [ok(1, 1), (1, 2, bytes(64), bytes(64), bytes(8), [4, 6, 5])], {}, "class 1: seed offsets must not decrease"),
            (h8, [(1, 1, one, one, bytes(65536), [0, 65536])], {"cap": 1 << 17}, "class 0: a seed is longer than 65535 bytes"),
            (h8, [ok(1, 2), ok(4, 1)], {"cap": 2 * fixed(h8, 1, 0) + fixed(h8, 4, 0) - 1}, "the output buffer is too small"),
            (h8, [ok(1, 2), (2, 2, bytes(96) + qle, bytes(128), b"", [0, 0, 0])], {}, r"class 1: values[3] is not below the group order"),
            (h8, [ok(1, 2), (2, 2, bytes(128), bytes(32) + qle + bytes(64), b"", [0, 0, 0])], {}, r"class 1: gammas[1] is not below the group order"),
        ]
        for handle, specs, kw, text in cases:
            rc, msg, obuf, ooff = _raw(eng, handle, specs, **kw)
            assert rc == E_ARG and text in msg and "bpmi_rp_prove_batch_mixed" in msg, (text, rc, msg)
            assert obuf == b"\xa5" * len(obuf) and ooff == [0xA5A5A5A5A5A5A5A5] * len(ooff), text
        # the exact cap passes, and n_classes = 0 is an empty success
        rc, msg, obuf, ooff = _raw(eng, h8, [ok(1, 2), ok(4, 1)], cap=2 * fixed(h8, 1, 0) + fixed(h8, 4, 0))
        assert rc == 0 and ooff[:4] == [0, fixed(h8, 1, 0), 2 * fixed(h8, 1, 0), 2 * fixed(h8, 1, 0) + fixed(h8, 4, 0)] and obuf[:5] == b"BPRP2"
        rc, msg, obuf, ooff = _raw(eng, h8, [], n_classes=0)
        assert rc == 0 and ooff[0] == 0 and ooff[1] == 0xA5A5A5A5A5A5A5A5 and obuf == b"\xa5" * len(obuf)
        # the Python surface refuses what it can see, and the prover still proves
        with pytest.raises(ValueError):
            mp.prove_classes_packed([(3, [], [], [])])
        with pytest.raises(ValueError):
            mp.prove_wire([([1, 2, 3], [1, 2, 3], b"")])
        vss, gss, seeds, _ = _rows(8, 2, 2, 0)
        assert len(_split(mp.prove_classes_packed([(2, vss, gss, seeds)]))[0]) == 2
    finally:
        mp.close()
        tiny.close()


def test_c_program_proves_two_classes_in_one_call_and_verifies_them(gp, tmp_path):
    """examples/prove_verify_mixed_c_abi.c: a C99 program over include/bpmi.h and libbpmi.so alone proves two classes in one call, commits
    from the prover's tables and verifies both with bpmi_rp_batch_verify_mixed_dev; with one commitment changed the block is rejected."""
    libdir = os.path.join(REPO, "python-bulletproofs_amd")
    exe = str(tmp_path / "prove_verify_mixed_c_abi")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"),
                           os.path.join(REPO, "examples", "prove_verify_mixed_c_abi.c"), "-o", exe, os.path.join(libdir, "libbpmi.so"),
                           "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined"])
    for args, code, word in (([], 0, "mixed batch verification: VALID"), (["70", "3", "64", "8"], 0, "mixed batch verification: VALID"),
                             (["9", "4", "16", "4", "1"], 1, "mixed batch verification: INVALID")):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == code and word in r.stdout, r.stdout + r.stderr
