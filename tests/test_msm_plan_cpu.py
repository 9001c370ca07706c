"""The plan of an MSM (python-bulletproofs_amd/csrc/msm_plan_host.hpp) checked on the CPU: the header is plain C++, so everything
that decides a buffer size or a launch shape -- window bits, mixed-width windows, chunk length, workspace layout, the bucket
reduction's jobs, the tail's bit offsets, slices -- is compiled into tests/csrc_host/libhost_shim.so and held against the
invariants the kernels rely on, over every threshold of the size tables, seeded random sizes, the options that reach the plan and
every mode a caller passes."""
import ctypes
import random

import pytest

from test_csrc_host import option_kv, shim  # noqa: F401  (the fixture that builds and loads the shim; options go by their bpmi_set_option names)

GEOM = ["n", "c", "W", "w0", "B", "G", "L", "nv", "prio", "fuse", "top2", "inblock", "mid", "small", "glv", "mid_parts"]
REGIONS = ["glv_sub", "glv_bx", "glv_neg", "hist", "off", "cursor", "bsum", "coarse_hist", "coarse_off", "coarse_cursor", "dig", "sidx", "dig16", "negs",
           "chunk_key", "buckets", "rec_key0", "rec_pt0", "rec_key1", "rec_pt1", "D", "E", "F", "out"]
JOB = ["in_off", "in_stride", "N", "s", "type", "glanes", "gpw", "nsums", "out_off", "out_stride", "blk0", "cnt"]
JOBS_WORDS = 2 + 4 * len(JOB)
REDUCE_WORDS = 3 * JOBS_WORDS + 12
XYZZ_BYTES, PART_MAX, COARSE_HIST_WORDS, MID_NMAX = 144, 2048, 2048 + 192, 8448
CHAINED, FREE_RUN, BESIDE = 1, 2, 4
# what the callers pass: bpmi_msm_dev_enqueue (chained with async_lanes, free_run with accum_chain = 0), the slices of a large MSM
# (chained), msm_run_pair (chained under pair_chain / pair_sched, beside for a large pair)
MODES = [0, CHAINED, FREE_RUN, CHAINED | FREE_RUN, BESIDE, CHAINED | BESIDE]

THRESHOLDS = [1, 2, 1023, 1024, 2559, 2560, 4608, 4609, 5631, 5632, 8448, 8449, 10239, 10240, 15359, 15360, 18999, 19000, 1 << 15,
              (1 << 17) - 1, 1 << 17, (1 << 17) + 1, 184999, 185000, 1 << 19, 1 << 20, 1 << 23]
_rnd = random.Random(20261018)
SIZES = THRESHOLDS + sorted(int(2 ** _rnd.uniform(0, 23)) for _ in range(200))
OPTION_SETS = ([{}] + [{"window_bits": c} for c in range(2, 17)] + [{"mixed_windows": 0}, {"top_window_unsigned": 0}, {"glv": 1}]
               + [{"mid_parts": k} for k in (1, 2, 3, 4)] + [{"small_n": -1}, {"mid_single_min": -1}]
               + [{"reduce_epl": k} for k in (1, 4, 16, 64)] + [{"reduce_fit": 0}] + [{"chunk": k} for k in (1, 86, 4096)]
               + [{"rounds": k} for k in (1, 3, 16)] + [{"fused_scan": 0}])
# the option sets under which msm_run_split's two window groups are planned as well
GROUP_SETS = [{}, {"window_bits": 8}, {"window_bits": 13}, {"window_bits": 16}, {"mixed_windows": 0}]


def bind(L):
    L.t_msm_plan.restype = ctypes.c_uint32
    L.t_msm_plan.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.t_msm_slices.restype = ctypes.c_uint64
    L.t_msm_slices.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    return L


def raw_plan(L, opts, n, mode=0, w0=0, wcount=0):
    """(window bits of n, geom words, layout words, reduce words) exactly as the shim returns them."""
    kv, nkv = option_kv(L, opts)
    geom, layout, reduce = (ctypes.c_uint32 * len(GEOM))(), (ctypes.c_uint64 * 30)(), (ctypes.c_uint32 * REDUCE_WORDS)()
    c = L.t_msm_plan(kv, nkv, n, w0, wcount, mode, geom, layout, reduce)
    return c, list(geom), list(layout), list(reduce)


def _jobs(words):
    return {"njobs": words[0], "prio": words[1], "j": [dict(zip(JOB, words[2 + len(JOB) * k:2 + len(JOB) * (k + 1)])) for k in range(4)]}


def plan(L, opts, n, mode=0, w0=0, wcount=0):
    _, geom, layout, reduce = raw_plan(L, opts, n, mode, w0, wcount)
    t = reduce[3 * JOBS_WORDS:]
    return {"g": dict(zip(GEOM, geom)), "off": dict(zip(REGIONS, layout[:24])), "total": layout[24], "total_sizing": layout[25], "P": layout[26],
            "nscan_blocks": layout[27], "rec0_max": layout[28], "nchunks": layout[29],
            "j1": _jobs(reduce[:JOBS_WORDS]), "j2": _jobs(reduce[JOBS_WORDS:2 * JOBS_WORDS]), "j2top": _jobs(reduce[2 * JOBS_WORDS:3 * JOBS_WORDS]),
            "grid1": t[0], "top_w": t[1], "to": {"nv": t[2], "off": t[3:7], "top": t[7], "top_off": t[8:12]}}


def slices(L, opts, nseg, cap=4096):
    """K and the K segs_slice results (total, n[3], pts[3], sc[3]) for segments of nseg pairs at made-up, never-read addresses."""
    kv, nkv = option_kv(L, opts)
    pts = [(i + 1) << 44 for i in range(3)]
    sc = [((i + 1) << 44) + (1 << 43) for i in range(3)]
    out = (ctypes.c_uint64 * (10 * cap))()
    K = L.t_msm_slices(kv, nkv, (ctypes.c_uint32 * 3)(*nseg), (ctypes.c_uint64 * 3)(*pts), (ctypes.c_uint64 * 3)(*sc), cap, out)
    rows = [list(out[10 * k:10 * k + 10]) for k in range(min(K, cap))]
    return K, [{"total": r[0], "n": r[1:4], "pts": r[4:7], "sc": r[7:10]} for r in rows], pts, sc


def split_groups(L, opts, n):
    """(w0, wcount) of the two window groups msm_run_split forms: the first W / 2 windows of 255 / c + 1, and the rest."""
    c = raw_plan(L, opts, n)[0]
    W = 255 // c + 1
    return [(0, W // 2), (W // 2, W - W // 2)]


def _ceil(a, b):
    return (a + b - 1) // b


def _job_blocks(j):
    return _ceil(_ceil(j["cnt"] * j["nsums"], j["gpw"]), 4)


def check_plan(p, opts, n, wcount):
    """Every invariant of one plan; `tag` in each message names the case."""
    g, tag = p["g"], (opts, n, wcount)
    c, W, B, G, top2 = g["c"], g["W"], g["B"], g["G"], g["top2"]
    # windows
    assert B == 1 << (c - 1) and G == (W + top2) * B, tag
    if top2:
        assert (W - top2) * c + top2 * (c + 1) == 256, tag
    elif not wcount:
        assert W * c >= (129 if g["glv"] else 256), tag
    assert not (g["mid"] and g["small"]), tag
    assert not g["mid"] or n <= MID_NMAX, tag
    assert g["n"] == (2 * n if g["glv"] else n), tag
    # sort
    assert p["P"] in (0, G >> 8) and p["P"] <= PART_MAX, tag
    assert not p["P"] or g["n"] <= 1 << 23, tag
    # chunks
    nW = g["n"] * W
    assert g["L"] >= 1 and p["nchunks"] * g["L"] >= nW, tag
    written = 2 * (_ceil(p["nchunks"], 64) if g["fuse"] else p["nchunks"])           # what k_accum_l0 writes
    assert p["rec0_max"] >= written, tag
    # layout: regions in the order they are taken, each 256-byte aligned, each as large as what the kernels index
    off = p["off"]
    need = {"glv_sub": 16 * g["n"] if g["glv"] else 0, "glv_bx": 16 * g["n"] if g["glv"] else 0, "glv_neg": g["n"] if g["glv"] else 0,
            "hist": 4 * G, "off": 4 * (G + 1), "cursor": 4 * G, "bsum": 4 * (p["nscan_blocks"] + 1), "coarse_hist": 4 * COARSE_HIST_WORDS,
            "coarse_off": 4 * (p["P"] + 1), "coarse_cursor": 4 * (p["P"] + 1), "dig": 4 * nW, "sidx": 4 * nW, "dig16": 2 * nW if p["P"] else 0,
            "negs": g["n"] if p["P"] else 0, "chunk_key": 4 * (p["nchunks"] + 1), "buckets": XYZZ_BYTES * G, "rec_key0": 4 * p["rec0_max"],
            "rec_pt0": XYZZ_BYTES * p["rec0_max"], "rec_key1": 0, "rec_pt1": 0, "D": 0, "E": XYZZ_BYTES * W * 4, "F": XYZZ_BYTES * W * 64, "out": 64}
    assert p["nscan_blocks"] * 4096 >= G, tag
    ends = [off[r] for r in REGIONS[1:]] + [p["total"]]
    room = {}
    for r, end in zip(REGIONS, ends):
        assert off[r] % 256 == 0 and 0 <= off[r] <= end <= p["total"], (tag, r)          # in take order and disjoint: each ends where the next begins
        room[r] = end - off[r]
        assert room[r] >= need[r], (tag, r, room[r], need[r])
    assert off[REGIONS[0]] == 0 and p["total"] == p["total_sizing"] and p["total"] % 256 == 0, tag
    # the segmented scan's loop: level 1 reads buffer 0 and writes buffer 1, the levels after it ping-pong; R -> 2 ceil(R / 256)
    R, level = p["rec0_max"], 1
    while _ceil(R, 256) > 1:
        R = 2 * _ceil(R, 256)
        dst = "1" if level % 2 else "0"
        assert room["rec_key" + dst] >= 4 * R and room["rec_pt" + dst] >= XYZZ_BYTES * R, (tag, level, R)
        level += 1
    # reduction
    to = p["to"]
    if B <= 256:
        assert p["j1"]["njobs"] == 0 and to["nv"] == 1 and g["nv"] == 1, tag
        return
    assert g["nv"] == 4 and to["nv"] == 4 and to["top"] == top2 and p["top_w"] == (W - top2 if top2 else 0xFFFFFFFF), tag
    assert p["j1"]["njobs"] == (4 if top2 else 2) and p["j2"]["njobs"] == 4 and p["j2top"]["njobs"] == (4 if top2 else 0), tag
    d_records = 0
    for name in ("j1", "j2", "j2top"):
        J = p[name]
        blk = 0
        for j in J["j"][:J["njobs"]]:
            assert 1 <= j["glanes"] and j["glanes"] * j["gpw"] <= 64 and j["gpw"] >= 1, (tag, name, j)
            assert j["blk0"] == blk, (tag, name, j)
            blk += _job_blocks(j)
            assert j["nsums"] == ((j["N"] >> j["s"]) if j["type"] else (1 << j["s"]) - 1), (tag, name, j)
            if name == "j1":
                d_records = max(d_records, (j["cnt"] - 1) * j["out_stride"] + j["out_off"] + j["nsums"])
            else:                                  # the finish: 16 sums per array at most, each record of F / the LDS of the finish
                assert j["nsums"] <= 16 and j["out_stride"] == 64, (tag, name, j)
        if name == "j1":
            assert p["grid1"] == blk, tag
    assert room["D"] >= XYZZ_BYTES * d_records, (tag, room["D"], d_records)
    assert 8 + 4 * W <= COARSE_HIST_WORDS - PART_MAX, tag              # the spread finish's tickets behind the partition counts
    # stage 1 reads every bucket record exactly once per job type: its arrays tile [0, G)
    for typ in (0, 1):
        spans = sorted((a * j["in_stride"] + j["in_off"], a * j["in_stride"] + j["in_off"] + j["N"])
                       for j in p["j1"]["j"][:p["j1"]["njobs"]] if j["type"] == typ for a in range(j["cnt"]))
        assert spans[0][0] == 0 and spans[-1][1] == G and all(spans[k][1] == spans[k + 1][0] for k in range(len(spans) - 1)), (tag, typ)
    # stage 2 reads the D records stage 1 wrote: D0 then D1 of every window
    s1 = {(j["type"], k // 2): j for k, j in enumerate(p["j1"]["j"][:p["j1"]["njobs"]])}
    for name, grp in (("j2", 0), ("j2top", 1)):
        J = p[name]
        for k, j in enumerate(J["j"][:J["njobs"]]):
            src = s1[(k // 2, grp)]                # jobs 0, 1 split D0 (stage 1's type 0), jobs 2, 3 split D1
            assert (j["in_off"], j["in_stride"], j["N"], j["cnt"]) == (src["out_off"], src["out_stride"], src["nsums"], src["cnt"]), (tag, name, k)
    if opts.get("reduce_fit", 1) and not opts.get("reduce_epl", 0):
        waves = sum(_ceil(j["cnt"] * j["nsums"], j["gpw"]) for j in p["j1"]["j"][:p["j1"]["njobs"]])
        epl = max(_ceil((1 << j["s"]) if j["type"] else ((j["N"] - 1) >> j["s"]) + 1, j["glanes"]) for j in p["j1"]["j"][:p["j1"]["njobs"]])
        assert waves <= 1024 or epl >= 64, (tag, waves, epl)


@pytest.fixture(scope="module")
def L(shim):  # noqa: F811
    return bind(shim)


def cases(opts, L):
    """(w0, wcount) for every size under one option set: the whole MSM, and msm_run_split's groups where they are swept."""
    for n in SIZES:
        yield n, 0, 0
        if opts in GROUP_SETS and n >= 2:
            for w0, wcount in split_groups(L, opts, n):
                yield n, w0, wcount


@pytest.mark.parametrize("opts", OPTION_SETS, ids=lambda o: "-".join("%s=%d" % kv for kv in o.items()) or "defaults")
def test_plan_invariants(L, opts):
    """Every size x every window group x every mode under one option set.  The mode may move the chunk length and what follows
    from it (chunks, records, their regions) and nothing else, so a plan that equals the mode-0 plan word for word is not checked twice."""
    for n, w0, wcount in cases(opts, L):
        base = raw_plan(L, opts, n, 0, w0, wcount)
        p0 = plan(L, opts, n, 0, w0, wcount)
        assert p0["g"]["w0"] == w0 and (not wcount or p0["g"]["W"] == wcount)
        check_plan(p0, opts, n, wcount)
        for mode in MODES[1:]:
            if raw_plan(L, opts, n, mode, w0, wcount) == base:
                continue
            p = plan(L, opts, n, mode, w0, wcount)
            check_plan(p, opts, n, wcount)
            # the mode changes L only, and only from 2^19 pairs, and only through `chained` / `beside`
            assert n >= 1 << 19 and mode & (CHAINED | BESIDE) and not opts.get("chunk"), (opts, n, mode)
            assert {k: v for k, v in p["g"].items() if k != "L"} == {k: v for k, v in p0["g"].items() if k != "L"}, (opts, n, mode)
            assert p["g"]["L"] != p0["g"]["L"] and (p["j1"], p["j2"], p["j2top"], p["to"], p["grid1"], p["P"]) == (p0["j1"], p0["j2"], p0["j2top"], p0["to"], p0["grid1"], p0["P"])


def test_mode_free_run_alone_changes_nothing_and_chained_gives_three_rounds(L):
    for n in SIZES:
        assert raw_plan(L, {}, n, FREE_RUN) == raw_plan(L, {}, n, 0)
        assert raw_plan(L, {}, n, CHAINED | FREE_RUN) == raw_plan(L, {}, n, CHAINED)
        assert raw_plan(L, {}, n, CHAINED | BESIDE) == raw_plan(L, {}, n, CHAINED) == raw_plan(L, {}, n, BESIDE)
    assert plan(L, {}, 1 << 20, CHAINED)["g"]["L"] == 29 == _ceil(1 << 24, 64 * 3072 * 3)
    assert plan(L, {"rounds": 1}, 1 << 20, CHAINED)["g"]["L"] == 86
    assert plan(L, {}, (1 << 19) - 1, CHAINED)["g"]["L"] == plan(L, {}, (1 << 19) - 1)["g"]["L"]


# what the comments of msm_plan_host.hpp state for the defaults, one MSM at a time
TABLE = [(185000, {"c": 16, "mid": 0, "small": 0}), (19000, {"c": 13, "W": 19, "top2": 9}), (8449, {"c": 12, "W": 21, "top2": 4}),
         (8448, {"mid": 1}), (2560, {"mid": 1}), (2559, {"small": 1}), (1 << 20, {"c": 16, "W": 16, "top2": 0})]


@pytest.mark.parametrize("n,want", TABLE)
def test_documented_table_points(L, n, want):
    g = plan(L, {}, n)["g"]
    assert {k: g[k] for k in want} == want


def _split4(b, s0, t_lo, t_hi):
    lo, hi = b & ((1 << s0) - 1), b >> s0
    return [lo & ((1 << t_lo) - 1), lo >> t_lo, hi & ((1 << t_hi) - 1), hi >> t_hi]


@pytest.mark.parametrize("mixed", [1, 0])
@pytest.mark.parametrize("c", range(10, 17))
def test_tail_offsets_recombine_every_bucket_index(L, c, mixed):
    """The reduction multiplies bucket b by b through four digit sums; tail_combine is right because the digits the jobs' (N, s)
    cut b into, weighted 2^off[k], give b back -- for the windows of B buckets and for the wide ones of 2B."""
    p = plan(L, {"window_bits": c, "mixed_windows": mixed}, 1 << 20)
    g, to = p["g"], p["to"]
    assert (g["top2"] > 0) == (c == 15 or (bool(mixed) and c < 16))
    rnd = random.Random(c)
    for first, J2, offs, top in ((0, p["j2"], to["off"], g["B"]), (2, p["j2top"], to["top_off"], 2 * g["B"])):
        if first and not g["top2"]:
            continue
        d0, d1 = p["j1"]["j"][first], p["j1"]["j"][first + 1]
        assert d0["N"] == top and d0["s"] == d1["s"]
        s0, t_lo, t_hi = d0["s"], J2["j"][0]["s"], J2["j"][2]["s"]
        assert J2["j"][1]["s"] == t_lo and J2["j"][3]["s"] == t_hi
        limits = [J2["j"][0]["nsums"], J2["j"][1]["nsums"], J2["j"][2]["nsums"], J2["j"][3]["nsums"]]
        for b in (range(1, top + 1) if c <= 12 else [1, top, top - 1] + [rnd.randrange(1, top + 1) for _ in range(4096)]):
            d = _split4(b, s0, t_lo, t_hi)
            assert b & ((1 << s0) - 1) <= d0["nsums"] and b >> s0 <= d1["nsums"], (c, b)
            assert all(x <= m for x, m in zip(d, limits)), (c, b, d, limits)
            assert sum(x << o for x, o in zip(d, offs)) == b, (c, b, d, offs)


def test_slices_cover_the_input_and_stay_inside_it(L):
    rnd = random.Random(6)
    for opts in ({}, {"slice_n": 1 << 16}, {"slice_n": 1 << 22}, {"slice_n": -1}, {"slice_n": 1 << 20, "slice_min": 1 << 20}):
        slice_n = (1 << 23) if opts.get("slice_n", 0) < 0 else (opts.get("slice_n") or (1 << 20))
        totals = {int(f * slice_n) + d for f in (1.0, 1.625, 1.65, 2.0) for d in (-1, 0, 1)} | {(1 << 21) + 1, 1 << 23, (1 << 23) + 1}
        for total in sorted(totals):
            for nsegs in (1, 2, 3):
                cuts = sorted(rnd.randrange(1, total) for _ in range(nsegs - 1))
                nseg = [b - a for a, b in zip([0] + cuts, cuts + [total])] + [0] * (3 - nsegs)
                K, rows, pts, sc = slices(L, opts, nseg)
                assert K >= 1 and len(rows) == K
                if K == 1:
                    assert rows[0]["total"] == total
                    continue
                covered = 0
                for r in rows:
                    assert 1 <= r["total"] <= min(slice_n + slice_n // 16, 1 << 23) and sum(r["n"]) == r["total"], (opts, total, nseg)
                    # its pieces, in order, are the next r["total"] logical pairs: each inside one source array, starting where the slice before ended
                    for k in range(3):
                        if not r["n"][k]:
                            assert all(m == 0 for m in r["n"][k:])
                            break
                        seg = next(i for i in range(3) if sum(nseg[:i + 1]) > covered)
                        first = covered - sum(nseg[:seg])
                        assert r["pts"][k] == pts[seg] + 64 * first and r["sc"][k] == sc[seg] + 32 * first, (opts, total, nseg)
                        assert first + r["n"][k] <= nseg[seg], (opts, total, nseg)
                        covered += r["n"][k]
                assert covered == total, (opts, total, nseg)
    assert slices(L, {}, [(1 << 21) + 1, 0, 0])[0] == 2                  # a slice may be a sixteenth over: two slices, not three
    assert slices(L, {"window_bits": 16}, [1 << 22, 0, 0])[0] == 1 and slices(L, {"split": 1}, [1 << 22, 0, 0])[0] == 1
