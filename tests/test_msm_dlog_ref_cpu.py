"""The integer model of tests/msm_dlog_ref.py pinned -- both recodings against their defining sums, the model's bytes against the C
oracle on explicit points -- and, from the model alone, the proof that every (geometry, scenario, size) named by the route table of
test_gpu_msm_reduce_degenerate.py shows the edge it is there for, so that no case there can be vacuous.  The geometries of the table are
held against the MSM planner itself (csrc/msm_plan_host.hpp through tests/csrc_host), the tail replay for the four-digit reduction
uses the planner's bit offsets, and host_tail.hpp runs on the model's window sums here, without a GPU."""
import ctypes
import functools
import random

import pytest

import msm_dlog_ref as M
import test_gpu_msm_reduce_degenerate as T
from msm_dlog_ref import HALF, Q
from oracle import cbind
from test_csrc_host import shim  # noqa: F401  (the fixture that builds and loads the host shim)
from test_msm_plan_cpu import bind, plan

GEOS = {name: T.geo_of(name) for name in T.GEOS}
PIPELINE_OPTIONS = {name: next(opts for call, opts, geo, _, _ in T.ROUTES.values() if geo == name and call == "msm")
                    for name in T.GEOS if name not in ("small", "mid")}


@pytest.fixture(scope="module")
def L(shim):  # noqa: F811
    return bind(shim)


def edge_scalars(geo):
    out = [0, 1, 2, Q - 1, Q - 2, HALF - 1, HALF, HALF + 1, HALF + 2, 1 << 255, (1 << 255) + 1, (1 << 256) - 1, Q, Q + 1]
    for w, (at, wd) in enumerate(geo.wins):                # digits of magnitude exactly B, and one above (negative, with a carry)
        for t in ((1 << (wd - 1)) - 1, 1 << (wd - 1), (1 << (wd - 1)) + 1, (1 << wd) - 1):
            s = t << at
            if s <= HALF:
                out += [s, Q - s, s | ((1 << at) - 1)]
    return out


@pytest.mark.parametrize("name", list(GEOS))
def test_recoding_represents_the_scalar(name):
    """sum_w digit_w 2^at_w is the folded scalar exactly, = +-s mod q, and every magnitude is a bucket of its window."""
    geo = GEOS[name]
    rnd = random.Random("recoding/" + name)
    seen_B = set()
    for s in edge_scalars(geo) + [rnd.randrange(Q) for _ in range(300)] + [rnd.randrange(1 << 255, 1 << 256) for _ in range(20)]:
        neg, ds = geo.raw_digits(s)
        folded = sum(d << geo.wins[w][0] for w, d in enumerate(ds))
        assert 0 <= folded <= HALF and folded == (Q - s % Q if neg else s % Q), (name, hex(s))
        assert sum(d << geo.wins[w][0] for w, d in enumerate(geo.digits(s))) % Q == s % Q, (name, hex(s))
        for w, d in enumerate(ds):
            assert abs(d) <= geo.buckets(w), (name, hex(s), w, d)
            if abs(d) == geo.buckets(w):
                seen_B.add(d > 0)
                assert (d < 0) == (geo.kind == "mid"), "magnitude B is never negative in the pipeline, only negative in the mid recoding"
        if geo.kind == "mid":
            assert all(-64 <= d <= 63 for d in ds[:36]) and 0 <= ds[36] <= 9
    assert seen_B, name


def test_pipeline_recoding_is_the_special_case_of_the_peel_file():
    """windows() / run_lengths() of test_gpu_msm_runs_peel.py are this model at c = 12 (17 + 4 windows) and c = 13 (10 + 9)"""
    import test_gpu_msm_runs_peel as P
    rnd = random.Random("peel-windows")
    for n, key in ((8449, ("pipeline", 12, 21, 4)), (19000, ("pipeline", 13, 19, 9))):
        geo = M.Geo(*key)
        assert P.windows(n) == geo.wins
        es = [rnd.randrange(Q) for _ in range(200)] + [0, 1, Q - 1, HALF, HALF + 1]
        runs = {}
        for e in es:
            for w, d in enumerate(geo.raw_digits(e)[1]):
                if d:
                    runs[(w, abs(d))] = runs.get((w, abs(d)), 0) + 1
        assert runs == P.run_lengths(es, n)


@pytest.mark.parametrize("name", ["c4", "c9", "c13", "c15", "c16", "c12_short_top", "small", "mid"])
def test_model_bytes_equal_the_oracle_on_explicit_points(name):
    """random small inputs, folded and unfolded scalars, the identity and repeated points among them: one multiplication of G by the
    model's total against cbind.msm_bytes over the explicit points"""
    geo = GEOS[name]
    rnd = random.Random("model-vs-oracle/" + name)
    for n in (1, 7, 60):
        pool = [rnd.randrange(1, Q) for _ in range(5)] + [0]
        dlogs = [rnd.choice(pool) * rnd.choice((1, 1, Q - 1, 2)) % Q for _ in range(n)]
        scalars = [rnd.choice((rnd.randrange(Q), rnd.randrange(Q), rnd.randrange(1 << 20), 0, Q - 1)) for _ in range(n)]
        res = M.run(geo, dlogs, scalars)
        assert res.total == sum(k * s for k, s in zip(dlogs, scalars)) % Q
        pb = b"".join(M.dlogs_to_le64(dlogs))
        assert res.bytes() == cbind.msm_bytes(pb, M.pack_scalars(scalars), n), (name, n)
        assert M.replay_tail(geo, res.E)[0] == res.total


# ---- the route table against the planner --------------------------------------------------------------------------------------
def route_sizes(route):
    call, options, geo_name, sizes, names = T.ROUTES[route]
    for size in sizes:
        size = T.SMALL_LARGEST if size == "largest" else size
        yield size if size is not None else T.natural_size(GEOS[geo_name])


@pytest.mark.parametrize("route", [r for r, v in T.ROUTES.items() if v[0] != "batch"])
def test_route_geometry_is_what_the_planner_picks(L, route):
    """what the GPU file asserts of msm_geometry, from msm_pick_geometry on the host: kernel family, window bits, windows, wide windows --
    at the natural size and at the smallest size a scenario of the route has (the tail shapes: three pairs)"""
    call, options, geo_name, sizes, names = T.ROUTES[route]
    kind, c, W, wide = T.GEOS[geo_name]
    for n in set(route_sizes(route)) | ({3} if call == "msm" and sizes == (None,) else set()):
        g = plan(L, options, n)["g"]
        assert (g["c"], g["W"], g["top2"]) == (c, W, wide), (route, n, g)
        assert (g["mid"], g["small"]) == (int(geo_name == "mid"), int(geo_name == "small")), (route, n, g)
        assert g["nv"] == (1 if 1 << (c - 1) <= 256 else 4)
    if geo_name == "small":
        assert plan(L, options, T.SMALL_LARGEST + 1)["g"]["small"] == 0


def test_stage_one_trees_of_both_kinds_are_named(L):
    """k_digit_sums adds a group's lanes with a butterfly when the group is a power of two and with the __shfl_down tree otherwise.
    From the planner's jobs: at c = 13 reduce_epl = 3, 5 and 64 all give powers of two; 6 and 7 give groups of 12, 10 and 21 lanes, and
    so does the default rule at c = 15 (12 lanes, five sums to a wave)."""
    shapes = {}
    for route, (call, options, geo_name, sizes, names) in T.ROUTES.items():
        if call == "msm" and sizes == (None,) and GEOS[geo_name].c >= 10:
            p = plan(L, options, T.natural_size(GEOS[geo_name]))
            shapes[route] = sorted({j["glanes"] for j in p["j1"]["j"][:p["j1"]["njobs"]]})
    pow2 = lambda v: v & (v - 1) == 0      # noqa: E731
    for route in ("c13_epl3", "c13_epl5", "c13_epl64", "c13_fit0", "c16_final"):
        assert all(pow2(v) for v in shapes[route]), (route, shapes[route])
    assert shapes["c13_epl6"] == [12, 32] and shapes["c13_epl7"] == [10, 21] and shapes["c15_spread256"] == [12, 32], shapes
    assert shapes["c13_epl64"] == [1, 2] and shapes["c13_epl3"] == [32, 64], shapes      # one lane per sum: no tree at all; a whole wave per sum


def finish_kernels(options, geo):
    """msm_queue_reduce (csrc/msm_host.hpp), restated: the kernels that reduce the buckets of one pipeline MSM under `options`"""
    o = dict(T.DEFAULTS, **options)
    if 1 << (geo.c - 1) <= 256:
        return {"k_window_weighted_small_quad" if o["quad_final"] else "k_window_weighted_small"}
    out = {"k_digit_sums"}
    if o["quad_final"] and o["final_spread"] == 1 and geo.c >= 10:
        out.add("k_digit_final_spread<0>")
    elif o["quad_final"] and o["final_spread"] >= 2:
        out |= {"k_digit_final_spread<1>/64" if o["final_spread"] == 2 else "k_digit_final_spread<1>/256", "k_digit_final_spread<2>"}
    else:
        out.add("k_digit_final_quad" if o["quad_final"] else "k_digit_final")
    return out


def test_every_kernel_of_the_stage_is_named_by_a_route():
    named = set()
    for route, (call, options, geo_name, sizes, names) in T.ROUTES.items():
        if call == "msm":
            named |= finish_kernels(options, GEOS[geo_name]) | {"k_tail", "host tail"}
            if dict(T.DEFAULTS, **options)["accum_runs"] == 0 or options.get("accum_runs_cap") == 1:
                named.add("k_segscan")
        elif call == "batch":
            named |= {"k_msm_batch/light" if options["msm_batch_route"] == T.LIGHT else "k_msm_batch/mid", "k_msm_batch_tail"}
        elif geo_name == "small":
            sizes = [T.SMALL_LARGEST if s == "largest" else s for s in sizes]
            named |= {"k_msm_small_pair", "host tail"} if call == "pair" else {"k_msm_small", "host tail"}
            if any(s > 256 for s in sizes):                       # more than one block per window: the partials are combined
                named.add("k_small_combine_pair" if call == "pair" else "k_small_combine")
        else:
            named |= {"k_msm_mid", "host tail"}
    assert named >= {"k_window_weighted_small", "k_window_weighted_small_quad", "k_digit_sums", "k_digit_final", "k_digit_final_quad",
                     "k_digit_final_spread<0>", "k_digit_final_spread<1>/64", "k_digit_final_spread<1>/256", "k_digit_final_spread<2>", "k_segscan",
                     "k_msm_small", "k_msm_small_pair", "k_small_combine", "k_small_combine_pair", "k_msm_mid", "k_msm_batch/light", "k_msm_batch/mid",
                     "k_tail", "k_msm_batch_tail", "host tail"}, named


# ---- every pinned case shows its edge -----------------------------------------------------------------------------------------------
def tail_offsets(L, geo_name):
    """(off, top_off) of the four-digit reduction of a pipeline geometry with more than 256 buckets, None for nv = 1"""
    geo = GEOS[geo_name]
    if geo.kind == "mid" or 1 << (geo.c - 1) <= 256:
        return None
    to = plan(L, PIPELINE_OPTIONS[geo_name], T.natural_size(geo))["to"]
    assert to["nv"] == 4 and to["top"] == geo.wide
    return to["off"], to["top_off"]


@functools.lru_cache(maxsize=None)
def result_of(geo_name, name, n):
    """(model result, dlogs, scalars) of a scenario, computed once"""
    geo = GEOS[geo_name]
    dlogs, scalars = M.scenario(geo, name, n)
    assert n is None or len(dlogs) == n
    return M.run(geo, dlogs, scalars), dlogs, scalars


def check_control(L, geo_name, geo, n):
    pb, sb, m = T.control_inputs(n if n is not None else T.natural_size(geo))
    assert m == (n if n is not None else T.natural_size(geo)) and len(pb) == 64 * m and len(sb) == 32 * m
    assert len({pb[64 * i: 64 * i + 64] for i in range(m)}) == min(m, 1000)


def check_stage(L, geo_name, geo, n, name):
    res, dlogs, scalars = result_of(geo_name, name, n)
    assert all(s <= HALF for k, s in zip(dlogs, scalars) if k), "no scalar of a point is folded: nothing is negated"
    if name == "full_equal":
        M.check_full_equal(geo, res, M.effective_limits(res, geo.limits()))
    elif name == "window_zero":
        M.check_window_zero(geo, res, M.effective_limits(res, M.zero_limits(geo)))
        assert set(M.replay_tail(geo, res.E)[1]) == {"identity"}      # one record per window: the tail runs on identities only
        offs = tail_offsets(L, geo_name)
        if offs:
            # four records per window: stage 1 already meets the cancellation -- the sum D1[hi] over the 2^s0 buckets hi 2^s0 + lo is
            # the identity over leaves that are not -- and the records that are left cancel in the tail's chain
            for w, x in enumerate(res.X):
                s0 = (offs[1] if geo.wide and w + geo.wide >= geo.W else offs[0])[2]
                if max(x, default=0) >= 2 << s0:
                    assert all(x[(1 << s0) + lo] for lo in range(1 << s0)) and sum(x[(1 << s0) + lo] for lo in range(1 << s0)) % Q == 0, (geo, w)
            total, kinds = M.replay_tail(geo, res.split(*offs), *offs)
            assert total == 0 and "cancellation" in kinds, (geo, M.count_kinds(kinds))
    elif name == "mixed_multiples":
        M.check_mixed_multiples(geo, res, M.effective_limits(res, geo.limits()))
    elif name == "sparse_edges":
        M.check_sparse_edges(geo, res)
    elif name == "one_bucket":
        M.check_one_bucket(geo, res)
        assert len(set(dlogs)) == 1 and len(set(scalars)) == 1
    else:
        M.check_tail(geo, res, name)                       # the chain of nv = 1: B <= 256, the small kernel, the batch and group tails
        offs = tail_offsets(L, geo_name)
        if offs:
            M.check_tail(geo, res, name, *offs)            # ... and of the four records per window of msm_reduce_plan


def check_batch_rows(L, geo_name, geo, n):
    dlogs, rows = M.batch_rows(geo, n)
    assert len(dlogs) == n and all(len(r) == n for r in rows) and len({tuple(r) for r in rows}) == 3
    res = [M.run(geo, dlogs, r) for r in rows]
    assert len({r.total for r in res}) == 3, "three different results: a row mix-up cannot pass"
    M.check_full_equal(geo, res[0])
    M.check_window_zero(geo, res[1])
    M.check_mixed_multiples(geo, res[2])
    assert any(s > HALF for s in rows[0]) and any(s > HALF for s in rows[2]), "rows 0 and 2 reach +P through q - s on -P"


CHECKS = dict({name: (lambda L, g, geo, n, name=name: check_stage(L, g, geo, n, name)) for name in M.SCENARIOS},
              control=check_control, batch_rows=check_batch_rows)


@pytest.mark.parametrize("geo_name,name,n", T.pinned_cases(), ids=lambda v: str(v))
def test_every_pinned_case_shows_its_edge(L, geo_name, name, n):
    """walks the GPU file's route table: a (geometry, scenario, size) without a precondition here fails"""
    assert name in CHECKS, "route table names %r, which has no precondition here" % name
    CHECKS[name](L, geo_name, GEOS[geo_name], n)


def test_pinned_cases_cover_the_route_table():
    pinned = set(T.pinned_cases())
    for route, (call, options, geo_name, sizes, names) in T.ROUTES.items():
        assert geo_name in T.GEOS and names, route
        for size in sizes:
            size = T.SMALL_LARGEST if size == "largest" else size
            for name in (("batch_rows",) if call == "batch" else names):
                assert (geo_name, name, size) in pinned and name in CHECKS, (route, name, size)


# ---- host_tail.hpp on the model's window sums -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tail_cancel", "tail_double", "full_equal", "window_zero", "mixed_multiples", "sparse_edges"])
@pytest.mark.parametrize("geo_name", ["c4", "c9", "c10", "c13", "c15", "c16", "c12_short_top", "small", "mid"])
def test_host_tail_on_the_window_sums_of_the_model(L, shim, geo_name, name):  # noqa: F811
    """The window sums of a scenario as projective records with random scalings through bpmi_host::tail_combine: the accumulator
    meets its addend (tail_double), its negative (tail_cancel) and whole windows of identities on the 4 x 64-bit group law, with the
    offsets the planner hands the tail."""
    geo = GEOS[geo_name]
    res = result_of(geo_name, name, None)[0]
    offs = tail_offsets(L, geo_name)
    rec = [v for r in res.split(*offs) for v in r] if offs else list(res.E)
    nv = 4 if offs else 1
    rnd = random.Random("host-tail/%s/%s" % (geo_name, name))
    zs = [rnd.randrange(1, 1 << 256) % cbind.secp256k1.p or 1 for _ in rec]
    out = ctypes.create_string_buffer(64)
    o4 = (ctypes.c_uint32 * 4)(*(offs[0] if offs else (0, 0, 0, 0)))
    t4 = (ctypes.c_uint32 * 4)(*(offs[1] if offs else (0, 0, 0, 0)))
    shim.t_host_tail(b"".join(M.dlogs_to_le64(rec)), b"".join(z.to_bytes(32, "little") for z in zs), geo.W, geo.c, nv, o4, geo.wide if offs else 0, t4, out)
    assert out.raw == res.bytes(), (geo_name, name)
