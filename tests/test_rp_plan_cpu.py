"""The plan of a batch preparation on the device (python-bulletproofs_amd/csrc/rp_batch_plan_host.hpp) checked on the CPU: the header
is plain C++, so everything bpmi_rp_batch_prepare_dev / _verify_dev / _group_values_dev decide between their HIP calls -- the argument
errors, the walk of the caller's offset table, the bound of a format-2/3 expansion, the layout of the two device buffers, rows per
launch, upload slices, launch shapes, the group mode's geometry -- is compiled into tests/csrc_host/libhost_shim.so and held against
the invariants the kernels rely on.  The offset table is the caller's and the proofs come from the network: an off-by-one here is a
device fault on untrusted input."""
import array
import ctypes
import itertools
import random

from conftest import load_golden
from test_csrc_host import option_kv, shim  # noqa: F401  (the fixture that builds and loads the shim; options go by their bpmi_set_option names)

SHAPE = ["P", "m", "k", "per", "ncols", "nslots", "fmt0", "v2", "rp_prio", "maxlen", "W", "o_off", "o_w", "o_st", "stage_bytes"]
REGIONS = ["contrib", "ctx", "shared", "T", "lens"]
GROUP_REGIONS = ["gsum", "gfin", "verdict", "ptflag", "E", "vals"]
REST = ["o_bad", "o_fin", "need", "cell_row", "out_row", "rows", "lanes", "el_log", "ranges", "lds_bytes", "pin_bytes", "nsl"]
TAIL = ["decode", "group", "ngroups", "msm_windows", "route"]
WORDS = 1 + len(SHAPE) + 2 * (len(REGIONS) + len(GROUP_REGIONS)) + len(REST) + 4 * 4 + len(TAIL)
E_ARG = -3
RP_ROLES, RP_MAX_PROOF_BYTES, RP_UPLOAD_SLICES, MID_NMAX, GROUP_LIGHT_NMAX, XYZZ_BYTES = 4, 32768, 4, 8448, 512, 144
DECODE_BESIDE, DECODE_FIRST, DECODE_LAST = 0, 1, 2
ROUTE_NONE, ROUTE_LIGHT, ROUTE_MID, ROUTE_MSM_RUN = 0, 1, 2, 3

N_PROOFS = [1, 2, 63, 64, 65, 4095, 4096, 4100, 1 << 22, (1 << 22) + 1]
# (n_gens, m): every power of two at the ends and in the middle, m over divisors; the non-divisors and bad n_gens are in the error test
GENS = [(2, 1), (2, 2), (4, 1), (8, 1), (8, 2), (8, 8), (64, 1), (64, 4), (64, 64), (1024, 16), (65536, 1), (65536, 1024)]
OPTION_SETS = ([{}] + [{"rp_rows": r} for r in (1, 5, 1000)] + [{"rp_lanes": v} for v in (1, 16, 64)] + [{"rp_slices": s} for s in (1, 2, 3, 4)]
               + [{"rp_overlap": 0}, {"rp_overlap": 0, "rp_slices": 3}] + [{"rp_priority": p} for p in (0, 2)])
ERR_N_GENS = "n_gens must be a power of two in [2, 65536]"
ERR_M = "values_per_proof must divide n_gens"
ERR_P = "n_proofs must be in [1, 2^22]"
ERR_4G = "at most 4 GiB of proofs per call"
ERR_TABLE = "offset table leaves the buffer"


def bind(L):
    L.t_rp_plan.restype = ctypes.c_int
    L.t_rp_plan.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                            ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint64]
    L.t_rp_group_chunk.restype = None
    L.t_rp_group_chunk.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    L.t_rp_expansion_bound.restype = ctypes.c_uint64
    L.t_rp_expansion_bound.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int]
    return L


_tables = {}


def offset_table(P, fmt):
    """A table of P + 1 non-decreasing offsets (a ctypes array, shared and never modified) and its end: proofs of about the length of a
    64-bit proof in wire format `fmt`, small batches with empty, short and over-long ones among them."""
    if (P, fmt) not in _tables:
        rnd = random.Random(1000 * P + fmt)
        base = {1: 900, 2: 500, 3: 700}[fmt]
        if P <= 4100:
            lens = [rnd.choice([0, 5, 4999, 30000 + rnd.randrange(9000)]) if rnd.randrange(11) == 0 else base + rnd.randrange(97) for _ in range(P)]
        else:
            lens = itertools.islice(itertools.cycle([base + rnd.randrange(97) for _ in range(1009)]), P)
        t = (ctypes.c_uint64 * (P + 1)).from_buffer(array.array("Q", itertools.accumulate(lens, initial=0)))
        _tables[(P, fmt)] = (t, t[P])
    return _tables[(P, fmt)]


def raw_plan(L, opts, n_gens, m, P, blobs, blobs_len, table, weights=False, group=0):
    """(error code, message, the RP_PLAN_WORDS words) exactly as the shim returns them; blobs: bytes, or None for a null pointer."""
    kv, nkv = option_kv(L, opts)
    out, msg = (ctypes.c_uint64 * WORDS)(), ctypes.create_string_buffer(128)
    rc = L.t_rp_plan(kv, nkv, n_gens, m, P, blobs, blobs_len, table, int(weights), group, out, msg, 128)
    return rc, msg.value.decode(), list(out)


def plan(L, opts, n_gens, m, P, fmt, weights=False, group=0):
    table, end = offset_table(P, fmt)
    rc, msg, w = raw_plan(L, opts, n_gens, m, P, b"BPRP%d" % fmt, end, table, weights, group)
    assert (rc, msg, w[0]) == (0, "", 0), (rc, msg)
    it = iter(w[1:])
    p = {name: next(it) for name in SHAPE}
    p["regions"] = [(name, next(it), next(it)) for name in REGIONS + GROUP_REGIONS]
    p.update((name, next(it)) for name in REST)
    p["slices"] = [tuple(next(it) for _ in range(4)) for _ in range(4)]
    p.update((name, next(it)) for name in TAIL)
    return p, table, end


def check_plan(p, table, end, opts, n_gens, m, P, fmt, weights, group):
    tag = (opts, n_gens, m, P, fmt, weights, group)
    k = n_gens.bit_length() - 1
    ncols, per = 5 + 2 * n_gens, 6 + 2 * k
    assert (p["P"], p["m"], p["k"], p["per"], p["ncols"], p["nslots"]) == (P, m, k, per, ncols, 2 + 3 * k + m), tag
    assert p["fmt0"] == ord("0") + fmt and p["v2"] == (fmt != 1), tag
    assert p["rp_prio"] == {0: 0, 1: int(fmt != 3), 2: 1}[opts.get("rp_priority", 1)], tag
    assert p["W"] == (min(p["maxlen"], RP_MAX_PROOF_BYTES) + 7) // 8 + 16, tag
    # stage-in: blobs (with 128 bytes of slack) | offsets | weights | one status byte per role and proof -- in order, disjoint, on 256-byte lines
    assert 0 < end + 128 <= p["o_off"] and p["o_off"] + 8 * (P + 1) <= p["o_w"] and p["o_w"] + (128 * P if weights else 0) <= p["o_st"], tag
    assert p["o_st"] + RP_ROLES * P <= p["stage_bytes"] and all(p[x] % 256 == 0 for x in ("o_off", "o_w", "o_st", "stage_bytes")), tag
    # rp_buf: regions 256-byte aligned, in order, disjoint, each large enough for what the kernels write; need = the end of the last one
    rows, size = p["rows"], dict((name, bytes_) for name, _, bytes_ in p["regions"])
    live = [r for r in p["regions"] if r[0] in REGIONS or group]
    pos = 0
    for name, off, bytes_ in live:
        assert off % 256 == 0 and off >= pos and off - pos < 256, (tag, name)
        pos = off + bytes_
    assert p["need"] == pos, tag
    if not group:
        assert all((off, bytes_) == (0, 0) for name, off, bytes_ in p["regions"] if name in GROUP_REGIONS), tag
    assert size["contrib"] >= 36 * ncols * rows and size["ctx"] >= 36 * p["nslots"] * rows and size["T"] == 8 * p["W"] * P and size["lens"] >= 4 * P, tag
    shared = next(r for r in p["regions"] if r[0] == "shared")
    assert p["out_row"] == 32 * ncols and p["o_bad"] == shared[1] + p["out_row"] and p["o_bad"] + 8 <= p["o_fin"], tag      # d_bad: behind the summed columns ...
    assert p["o_fin"] % 16 == 0 and p["o_fin"] + 32 * (3 + 2 * n_gens) <= shared[1] + shared[2], tag                       # ... the MSM scalars behind it, inside the region
    assert p["pin_bytes"] >= p["out_row"] + 8, tag
    # rows per launch
    assert 1 <= rows <= P and p["cell_row"] == 36 * (ncols + p["nslots"]), tag
    assert rows == 1 or rows * p["cell_row"] <= 256 << 20, tag
    if opts.get("rp_rows", 0) > 0:
        assert rows <= opts["rp_rows"], tag
        assert rows == min(P, opts["rp_rows"]) or (rows + 1) * p["cell_row"] > 256 << 20, tag
    else:
        assert rows == P or (rows + 1) * p["cell_row"] > 256 << 20, tag
    chunks = [(base, min(rows, P - base)) for base in range(0, P, rows)] if P // rows <= 4096 else None
    if chunks:
        assert chunks[0][0] == 0 and sum(c for _, c in chunks) == P and all(a + c == b for (a, c), (b, _) in zip(chunks, chunks[1:])), tag
    # launch shapes
    assert p["lanes"] == (opts.get("rp_lanes", 0) or 64) and p["lds_bytes"] == (k + 1) * 9 * 64 * 4 <= 160 * 1024, tag
    assert p["el_log"] == min(3, (n_gens // m).bit_length() - 1) and p["ranges"] << p["el_log"] == n_gens, tag
    # upload slices: whole proofs, a partition of the proofs and of the bytes
    nsl, overlap = p["nsl"], opts.get("rp_overlap", 1)
    assert 1 <= nsl <= RP_UPLOAD_SLICES, tag
    if P < 4096 or not overlap:
        assert nsl == 1, tag
    else:
        assert nsl == (opts.get("rp_slices", 0) or (1 if fmt == 3 else RP_UPLOAD_SLICES)), tag
    sl = p["slices"][:nsl]
    assert sl[0][0] == 0 and sl[0][2] == 0 and sl[-1][1] == P and sl[-1][3] == end and all(s == (0, 0, 0, 0) for s in p["slices"][nsl:]), tag
    for (g0, g1, b0, b1), nxt in zip(sl, sl[1:] + [None]):
        assert g0 <= g1 and b0 <= b1 and (g0 == 0 or b0 == table[g0]) and (nxt is None or (nxt[0] == g1 and nxt[2] == b1 == table[g1])), tag
    assert p["decode"] == (DECODE_BESIDE if overlap else (DECODE_FIRST if group else DECODE_LAST)), tag
    # group mode
    if not group:
        assert (p["group"], p["ngroups"], p["msm_windows"], p["route"]) == (0, 0, 0, ROUTE_NONE), tag
        return chunks
    grp = min(group, P)
    ng = (P + grp - 1) // grp
    assert (p["group"], p["ngroups"], p["msm_windows"]) == (grp, ng, 255 // 7 + 1), tag
    pairs = 3 + 2 * n_gens + grp * (m + per)
    assert p["route"] == (ROUTE_LIGHT if pairs <= GROUP_LIGHT_NMAX else ROUTE_MID if pairs <= MID_NMAX else ROUTE_MSM_RUN), tag
    assert size["gsum"] >= 32 * ncols * ng and size["gfin"] >= 32 * (3 + 2 * n_gens) * ng and size["verdict"] >= P and size["ptflag"] >= P, tag
    assert size["E"] >= XYZZ_BYTES * p["msm_windows"] * ng and size["vals"] >= 64 * ng, tag
    return chunks


def big(P, n_gens):
    return P > 4100 and n_gens > 64      # (2^22 proofs over 65 536 generators: a table of 2^22 offsets per case is enough of them)


def test_plans_hold_their_invariants_over_the_sweep(shim):
    L = bind(shim)
    cases = 0
    for (n_gens, m), P in itertools.product(GENS, N_PROOFS[:-1]):
        for fmt, weights in itertools.product((1, 2, 3), (False, True)):
            sets = OPTION_SETS if not big(P, n_gens) else OPTION_SETS[:1]
            for opts in sets if (fmt, weights) == (1, False) or (P <= 4100 and (fmt, weights) == (3, True)) or P in (4096, 4100) else sets[:1]:
                for group in (0, 1, 4, P, P + 9):
                    p, table, end = plan(L, opts, n_gens, m, P, fmt, weights, group)
                    check_plan(p, table, end, opts, n_gens, m, P, fmt, weights, group)
                    cases += 1
    assert cases > 8000


def test_group_chunks_cover_every_group_with_a_proof_in_the_chunk_once(shim):
    """k_rp_group_colsum's geometry (rp_group_chunk) over the row chunks of a plan: lpg lanes per group and gpb groups per wave fill a
    wave exactly; the nt groups from t0 are those with a proof in [base, base + cnt); nblk waves hold them."""
    L = bind(shim)
    out = (ctypes.c_uint32 * 5)()
    rnd = random.Random(5)
    cases = [(g, b, c) for g in (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 100, 4096, 1 << 22) for b in (0, 1, 63, 64, 4095, 4100) for c in (1, 2, 5, 64, 65, 4097)]
    cases += [(rnd.randrange(1, 1 << rnd.randrange(1, 23)), rnd.randrange(0, 1 << 22), rnd.randrange(1, 1 << rnd.randrange(1, 22))) for _ in range(2000)]
    for group, base, cnt in cases:
        L.t_rp_group_chunk(group, base, cnt, out)
        t0, nt, lpg, gpb, nblk = out
        tag = (group, base, cnt)
        assert lpg * gpb == 64 and lpg & (lpg - 1) == 0 and (lpg >= min(group, 64) and (lpg == 1 or lpg // 2 < group)), tag
        assert t0 == base // group and t0 + nt - 1 == (base + cnt - 1) // group and nt >= 1, tag      # first and last group touched: all between are
        assert (nblk - 1) * gpb < nt <= nblk * gpb, tag
    # a plan's row chunks: every group is covered by the chunks that hold one of its proofs, and by no other
    for P, rows, group in ((9, 5, 4), (65, 7, 4), (100, 64, 1), (4100, 1000, 33), (64, 64, 64), (9, 2, 100)):
        p, _, _ = plan(L, {"rp_rows": rows}, 8, 1, P, 1, False, group)
        seen = {}
        for base in range(0, P, p["rows"]):
            cnt = min(p["rows"], P - base)
            L.t_rp_group_chunk(p["group"], base, cnt, out)
            for t in range(out[0], out[0] + out[1]):
                seen.setdefault(t, []).append((base, cnt))
        assert sorted(seen) == list(range(p["ngroups"]))
        for t, cs in seen.items():
            lo, hi = t * p["group"], min(P, (t + 1) * p["group"])
            assert cs == [(b, c) for b in range(0, P, p["rows"]) for c in [min(p["rows"], P - b)] if b < hi and b + c > lo]


def test_argument_errors_keep_their_texts_and_their_order(shim):
    L = bind(shim)
    table, end = offset_table(64, 2)
    ok = dict(n_gens=64, m=1, P=64, blobs_len=end)
    # one error each, in the order of precedence; the later ones are then combined with every earlier one
    errors = [(ERR_N_GENS, dict(n_gens=0)), (ERR_N_GENS, dict(n_gens=1)), (ERR_N_GENS, dict(n_gens=96)), (ERR_N_GENS, dict(n_gens=131072)),
              (ERR_M, dict(m=0)), (ERR_M, dict(m=3)), (ERR_M, dict(m=128)),
              (ERR_P, dict(P=0)), (ERR_P, dict(P=(1 << 22) + 1)),
              (ERR_4G, dict(blobs_len=(1 << 32) + 1)),
              (ERR_TABLE, dict(blobs_len=end - 1))]
    rank = [ERR_N_GENS, ERR_M, ERR_P, ERR_4G, ERR_TABLE]

    def call(a, tab=table, blobs=None):
        rc, msg, w = raw_plan(L, {}, a["n_gens"], a["m"], a["P"], blobs, a["blobs_len"], tab)
        assert w[0] == (rc & (2 ** 64 - 1)) and not any(w[1:]) or rc == 0
        return rc, msg
    for text, change in errors:
        assert call({**ok, **change}) == (E_ARG, text), change
    for (t1, c1), (t2, c2) in itertools.combinations(errors, 2):
        if set(c1) & set(c2):
            continue
        want = min((t1, t2), key=rank.index)
        if "P" in {**c1, **c2} and want == ERR_TABLE:
            continue
        assert call({**ok, **c1, **c2}) == (E_ARG, want), (c1, c2)
    # an offset table that decreases, or leaves the buffer at its start, in its middle or at its end: refused WITHOUT reading `blobs` (a null pointer here)
    for i, v in ((0, end + 1), (1, end + 1), (31, table[30] - 1), (64, end + 1), (64, table[63] - 1), (1, (1 << 64) - 1)):
        bad = (ctypes.c_uint64 * 65)(*table)
        bad[i] = v
        assert call(ok, bad) == (E_ARG, ERR_TABLE), (i, v)
    assert call({**ok, "P": (1 << 22) + 1, "blobs_len": 0}) == (E_ARG, ERR_P)      # (the table is not walked then: it has 65 entries)
    assert call(ok, table, b"BPRP2") == (0, "")


def test_the_call_has_the_wire_format_of_its_first_proof(shim):
    L = bind(shim)
    for fmt in (1, 2, 3):
        table, end = offset_table(65, fmt)
        for magic, want in ((b"BPRP%d" % fmt, fmt), (b"BPRP9", 9), (b"XXXX2", 2)):
            rc, _, w = raw_plan(L, {}, 8, 1, 65, magic, end, table)
            assert rc == 0 and (w[1 + SHAPE.index("fmt0")], w[1 + SHAPE.index("v2")]) == (ord("0") + want, int(want in (2, 3)))
    # a first proof too short to hold a magic, or a table whose first proof would end outside the buffer's first 5 bytes: format 1, nothing read
    short = (ctypes.c_uint64 * 3)(0, 4, 900)
    rc, _, w = raw_plan(L, {}, 8, 1, 2, None, 900, short)
    assert rc == 0 and w[1 + SHAPE.index("fmt0")] == ord("1") and w[1 + SHAPE.index("maxlen")] == 896
    late = (ctypes.c_uint64 * 2)(3, 3)
    rc, _, w = raw_plan(L, {}, 8, 1, 1, None, 3, late)
    assert rc == 0 and w[1 + SHAPE.index("fmt0")] == ord("1")


def _with_seeds(blob, seed, seed1):
    """The format-2 or -3 proof `blob` with its two transcript seeds replaced (the expansion's length depends on their lengths alone)."""
    k = blob[5]
    at = 6 + 32 * (5 + k) + 33 * (6 + 2 * k) + 128
    sl = int.from_bytes(blob[at:at + 2], "big")
    at1 = at + 2 + sl
    sl1 = int.from_bytes(blob[at1:at1 + 2], "big")
    return blob[:at] + len(seed).to_bytes(2, "big") + seed + len(seed1).to_bytes(2, "big") + seed1 + blob[at1 + 2 + sl1:]


def test_expansion_bound_covers_what_the_expander_writes(shim):
    """rp_expansion_bound(len, k, fmt) sizes the rows of the device's word-major proof array from a proof's LENGTH alone.  It must be
    at least what rpw::expand_v2 (the host twin of the device expander; through bpmi_rp_wire_v2_to_v1) writes for the reference-made
    golden proofs in formats 2 and 3, with their own seeds and with seeds of every length class up to the wire format's 16-bit limit."""
    import sys
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_wire_golden
    from bulletproofs_amd.rangeproofs.codec import proof_to_bytes
    from test_wire_v2_cpu import native_expand
    L = bind(shim)
    gold = load_golden("rangeproofs.json")
    want = {(e["family"], e["index"]): e for e in load_golden("wire_formats.json")["proofs"]}
    rnd = random.Random(11)
    checked, slack = 0, []
    for family in ("single", "aggregated"):
        for i, c in enumerate(gold[family]):
            pr = make_wire_golden.proof_of(c["proof"])
            for fmt in (2, 3):
                blob = proof_to_bytes(pr, version=fmt)
                assert len(blob) == want[(family, i)]["format_%d" % fmt]["bytes"]
                variants = [blob] + [_with_seeds(blob, rnd.randbytes(a), rnd.randbytes(b))
                                     for a, b in ((0, 0), (1, 0), (0, 1), (2, 2), (3, 1), (40, 0), (0, 40), (300, 301), (8999, 2), (1, 9000), (65535, 0), (0, 65535))]
                rc, bad, out = native_expand(variants)
                assert (rc, bad) == (0, -1)
                for v, e in zip(variants, out):
                    bound = L.t_rp_expansion_bound(len(v), v[5], ord("0") + fmt)
                    assert bound >= len(e), (family, i, fmt, len(v), len(e), bound)
                    slack.append(bound - len(e))
                    checked += 1
    assert checked == 2 * 13 * len(want)
    # the bound never decreases with the length: the longest proof of a batch bounds them all (rp_plan_shape relies on it)
    for k in (0, 1, 6, 16):
        for fmt in (2, 3):
            vals = [L.t_rp_expansion_bound(n, k, ord("0") + fmt) for n in range(0, 12000)]
            assert all(a <= b for a, b in zip(vals, vals[1:]))
