"""The LAST stage of every MSM -- bucket sums -> window sums -> the Horner chain of the tail -- on COLLIDING bucket sums, against integers.

Every point is a known multiple of G (tests/msm_dlog_ref.py), so the bucket table, the window sums and the result are Python
integers times G.  The reduction tests elsewhere feed this stage sums of distinct random points, which never coincide: of the three
exceptional outcomes of the general addition (an identity operand, A + A, A + (-A)) they reach the first only.  Here whole windows
of buckets hold ONE point, +-P in a pattern that makes every window sum the identity, five small multiples side by side (ordinary,
doubling, cancelling and identity quads in the same wave), one bucket per window, and window sums that make the tail's accumulator
meet its addend and its negative -- on every route the stage has:

  pipeline, B <= 256     k_window_weighted_small / _quad (c = 4: the 64-thread block; 5; 9: 256 buckets)
  pipeline, B > 256      k_digit_sums (power-of-two groups and the __shfl_down tree of the other sizes: reduce_epl 3 / 5 / 64 / 6 / 7,
                         reduce_fit 0) followed by k_digit_final, k_digit_final_quad, k_digit_final_spread<0>, <1> in both block sizes + <2>, at
                         c = 10, 13, 15, 16 and the short top window of c = 12 without mixed widths
  tails                  every pipeline route under tail = 1 (k_tail) and tail = 2 (host_tail.hpp): equal bytes, equal to the model
  k_segscan              one_bucket under the chunked accumulation with chunk 1, 2 and the default; the accumulation by runs besides
  one launch             k_msm_small + k_small_combine, k_msm_small_pair + k_small_combine_pair, k_msm_mid (one and three parts,
                         single and as a pair), msm_mid_block in both block shapes through bpmi_msm_batch_dev and k_msm_batch_tail

The window_bits option forces the pipeline at any n; every route asserts the geometry (kernel family, window bits, windows, wide
windows) its model was built for, which is what keeps a route from moving to another kernel and still passing.  The group kernels
(k_msm_group*, k_msm_ipa_group*) take their scalars from proofs and cannot be steered this way; they share msm_mid_block and
msm_tail_combine with the routes above and are left out.  test_msm_dlog_ref_cpu.py proves, from the model alone, that every
(geometry, scenario, size) named here shows its edge, and walks ROUTES so that none is added without."""
import functools
import random

import pytest

import msm_dlog_ref as M
from msm_dlog_ref import Q

pytestmark = pytest.mark.gpu

HUGE = 1 << 30
# every option a route touches, at the library's default
DEFAULTS = {"window_bits": 0, "tail": 0, "quad_final": 1, "final_spread": 3, "reduce_epl": 0, "reduce_fit": 1, "mixed_windows": 1,
            "top_window_unsigned": 1, "accum_runs": 1, "accum_runs_cap": 0, "chunk": 0, "mid_parts": 0, "mid_single_min": 0, "mid_min": 0,
            "small_n": 0, "small_pair": 1, "msm_batch_route": 0}
# geometry name -> (recoding, window bits, windows, of which one bit wider): what msm_geometry must report, and what the model is built on
GEOS = {
    "c4": ("pipeline", 4, 64, 0), "c5": ("pipeline", 5, 52, 0), "c9": ("pipeline", 9, 29, 0),
    "c10": ("pipeline", 10, 25, 6), "c13": ("pipeline", 13, 19, 9), "c15": ("pipeline", 15, 17, 1), "c16": ("pipeline", 16, 16, 0),
    "c12_short_top": ("pipeline", 12, 22, 0),
    "small": ("pipeline", 8, 32, 0), "mid": ("mid", 7, 37, 0),
}
GEO_OPTIONS = {"c10": {"window_bits": 10}, "c13": {"window_bits": 13}, "c15": {"window_bits": 15}, "c16": {"window_bits": 16},
               "c12_short_top": {"window_bits": 12, "mixed_windows": 0, "top_window_unsigned": 0}}
STAGE = ("control", "full_equal", "window_zero", "mixed_multiples", "sparse_edges", "tail_cancel", "tail_double")
ALL = STAGE + ("one_bucket",)
FINISHES = {
    "final": {"quad_final": 0},                                   # k_digit_final
    "quad": {"quad_final": 1, "final_spread": 0},                 # k_digit_final_quad
    "tickets": {"quad_final": 1, "final_spread": 1},              # k_digit_final_spread<0> (needs the LDS sort: c >= 10)
    "spread64": {"quad_final": 1, "final_spread": 2},             # k_digit_final_spread<1> in 64-thread blocks + <2>
    "spread256": {"quad_final": 1, "final_spread": 3},            # k_digit_final_spread<1> in 256-thread blocks + <2>
}
LIGHT, MID = 1, 2


def _routes():
    """name -> (call, options, geometry, sizes, scenarios).  call: "msm" one bpmi_msm under tail 1 and 2 (the pipeline), "one" one bpmi_msm,
    "pair" one bpmi_msm2 of two different scenarios, "batch" bpmi_msm_batch_dev with three rows; sizes: None = the scenario's natural size
    (the smallest that fills every bucket of the route's windows once)."""
    r = {}
    for c in (4, 5, 9):                                           # B <= 256: one launch per MSM, nv = 1
        for quad in (1, 0):
            r["weighted_c%d_quad%d" % (c, quad)] = ("msm", {"window_bits": c, "quad_final": quad}, "c%d" % c, (None,), STAGE)
    for geo, base in GEO_OPTIONS.items():                         # B > 256: k_digit_sums + a finish, nv = 4
        for fin, opts in FINISHES.items():
            r["%s_%s" % (geo, fin)] = ("msm", dict(base, **opts), geo, (None,), STAGE)
    # stage 1's group sizes at c = 13 (digit_group, msm_plan_host.hpp): 32 / 64 lanes at 3 elements per lane, 16 / 32 at 5, 1 / 2 at 64 --
    # powers of two, the butterfly -- and 12 lanes at 6, 10 and 21 at 7: the __shfl_down tree with identity partners (c = 15 by default: 12)
    for epl in (3, 5, 64, 6, 7):
        r["c13_epl%d" % epl] = ("msm", {"window_bits": 13, "reduce_epl": epl}, "c13", (None,), STAGE)
    r["c13_fit0"] = ("msm", {"window_bits": 13, "reduce_fit": 0}, "c13", (None,), STAGE)
    # k_segscan: one, several and the default number of levels; then the accumulation by runs with the run over and under the cap
    for chunk in (1, 2, 0):
        r["segscan_chunk%d" % chunk] = ("msm", {"window_bits": 13, "accum_runs": 0, "chunk": chunk}, "c13", (4096,), ("one_bucket", "control"))
    r["runs_cap1"] = ("msm", {"window_bits": 13, "accum_runs": 2, "accum_runs_cap": 1}, "c13", (4096,), ("one_bucket", "control"))
    r["runs_caphuge"] = ("msm", {"window_bits": 13, "accum_runs": 2, "accum_runs_cap": HUGE}, "c13", (4096,), ("one_bucket", "control"))
    # one-launch routes, default window_bits.  "largest": the largest n msm_geometry still reports as small
    r["small"] = ("one", {}, "small", (64, 300, "largest"), ALL)
    # (a pair moves to k_msm_mid from 1 536 pairs: mid_min = -1 keeps the pair kernel up to the single MSM's bound)
    r["small_pair"] = ("pair", {"mid_min": -1}, "small", (64, 300, "largest"), ALL)
    for parts in (1, 3):                                          # (mid_single_min set: with mid_parts = 1 the default rule ends the kernel's range at 5 631)
        r["mid_parts%d" % parts] = ("one", {"mid_parts": parts, "mid_single_min": 2560}, "mid", (4097, 8448), ALL)
    r["mid_pair"] = ("pair", {}, "mid", (4097,), ALL)
    r["batch_light"] = ("batch", {"msm_batch_route": LIGHT}, "mid", (129, 512), M.BATCH_ROWS)
    r["batch_mid"] = ("batch", {"msm_batch_route": MID}, "mid", (513, 8448), M.BATCH_ROWS)
    return r


ROUTES = _routes()
SMALL_LARGEST = 2559          # what "largest" must come to under the default options (msm_plan_host.hpp: k_msm_mid takes over at 2 560)


def geo_of(name):
    return M.Geo(*GEOS[name])


def pinned_cases():
    """every (geometry name, scenario, size) the routes name -- what test_msm_dlog_ref_cpu.py must hold a precondition for"""
    out = set()
    for call, _, geo, sizes, names in ROUTES.values():
        for n in sizes:
            n = SMALL_LARGEST if n == "largest" else n
            out |= {(geo, "batch_rows" if call == "batch" else name, n) for name in names}
    return sorted(out, key=repr)


@pytest.fixture(scope="module")
def gp():
    import gpu_common
    return gpu_common


def natural_size(geo):
    return max(geo.limits())


@functools.lru_cache(maxsize=None)
def control_inputs(n):
    """1 000 distinct random points tiled over n pairs under random scalars -> (point bytes, scalar bytes, n)"""
    rnd = random.Random("msm-reduce/control")
    enc = M.dlogs_to_le64([rnd.randrange(1, Q) for _ in range(1000)])
    return b"".join(enc[i % 1000] for i in range(n)), b"".join(rnd.randrange(Q).to_bytes(32, "little") for _ in range(n)), n


@functools.lru_cache(maxsize=None)
def control_case(n):
    """... against the ORACLE's MSM: it separates "the route is broken" from "the collision is mishandled" """
    from oracle import cbind
    pb, sb, n = control_inputs(n)
    return pb, sb, n, cbind.msm_bytes(pb, sb, n)


@functools.lru_cache(maxsize=None)
def case(geo_name, name, n):
    """(point bytes, scalar bytes, pairs, the model's 64 bytes), computed once and shared by the routes of one geometry"""
    geo = geo_of(geo_name)
    if name == "control":
        return control_case(n if n is not None else natural_size(geo))
    dlogs, scalars = M.scenario(geo, name, n)
    return b"".join(M.dlogs_to_le64(dlogs)), M.pack_scalars(scalars), len(dlogs), M.run(geo, dlogs, scalars).bytes()


@functools.lru_cache(maxsize=None)
def batch_case(n):
    geo = geo_of("mid")
    dlogs, rows = M.batch_rows(geo, n)
    return b"".join(M.dlogs_to_le64(dlogs)), [M.pack_scalars(r) for r in rows], [M.run(geo, dlogs, r).bytes() for r in rows]


def check_geometry(eng, route, geo_name, n, kernel):
    g = eng.msm_geometry(n)
    kind, c, W, wide = GEOS[geo_name]
    assert (g["kernel"], g["window_bits"], g["windows"], g["wide_windows"]) == (kernel, c, W, wide), (route, geo_name, n, g)
    assert M.Geo.from_engine(g).key() == geo_of(geo_name).key(), (route, geo_name, n, g)


def largest_small(eng):
    return max(n for n in range(1, 8449) if eng.msm_geometry(n)["kernel"] == "small")


def check_runs_state(eng, options, route, geo, name):
    """the accumulation the route meant: chunked when accum_runs = 0 or the one run of a window is over the cap, by runs otherwise"""
    st = eng.msm_runs_state(0)
    assert st["planned"] == (options.get("accum_runs") == 2), (route, name, st)
    if st["planned"] and name == "one_bucket":
        assert st["long_run"] == (options["accum_runs_cap"] == 1), (route, name, st)
        if not st["long_run"]:
            assert st["runs"] == sum(1 for lim in geo.limits() if lim), (route, name, st)


@pytest.mark.parametrize("route", list(ROUTES))
def test_reduction_and_tail_on_colliding_bucket_sums(gp, route):
    call, options, geo_name, sizes, names = ROUTES[route]
    eng = gp.engine()
    geo = geo_of(geo_name)
    kernel = {"small": "small", "mid": "mid"}.get(geo_name, "pipeline")
    failures, ran = [], 0
    try:
        for k, v in dict(DEFAULTS, **options).items():
            eng.set_option(k, v)
        if options.get("final_spread") == 1:
            assert geo.c >= 10, "the ticket finish runs only behind the LDS sort (msm_lds_sort: c >= 10, n <= 2^23)"
        for size in sizes:
            if size == "largest":
                size = largest_small(eng)
                assert size == SMALL_LARGEST, (route, size)
            where = "route %s, %%s, %r, n = %s" % (route, geo, size)
            if call == "batch":
                pb, rows, wants = batch_case(size)
                d_pts, d_sc = eng.upload(pb), eng.upload(b"".join(rows))
                try:
                    got = eng.msm_batch_dev([d_pts], [size], [d_sc], len(rows))
                finally:
                    d_pts.free()
                    d_sc.free()
                for i, name in enumerate(names):
                    ran += 1
                    if got[64 * i: 64 * i + 64] != wants[i]:
                        failures.append(where % ("row %d = %s" % (i, name)) + ": differs from the integer model")
                continue
            if call == "pair":
                check_geometry(eng, route, geo_name, size, kernel)
                cases = [case(geo_name, name, size) for name in names]
                for i, name in enumerate(names):                   # two DIFFERENT scenarios side by side, every one in both places
                    a, b = cases[i], cases[(i + 1) % len(cases)]
                    got = eng.msm2_bytes(a[0], a[1], a[2], b[0], b[1], b[2])
                    ran += 1
                    other = names[(i + 1) % len(names)]
                    for out, want, nm in ((got[0], a[3], name), (got[1], b[3], other)):
                        if out != want:
                            failures.append(where % ("pair (%s, %s): %s" % (name, other, nm)) + ": differs from the integer model")
                continue
            for name in names:
                pb, sb, n, want = case(geo_name, name, size)
                check_geometry(eng, route, geo_name, n, kernel)
                ran += 1
                if call == "one":
                    if eng.msm_bytes(pb, sb, n) != want:
                        failures.append(where % name + ": differs from the integer model")
                    continue
                got = {}
                for tail in (1, 2):                                # k_tail, host_tail.hpp
                    eng.set_option("tail", tail)
                    got[tail] = eng.msm_bytes(pb, sb, n)
                    check_runs_state(eng, options, route, geo, name)
                if got[1] != got[2]:
                    failures.append(where % name + ": the device tail and the host tail differ")
                for tail in (1, 2):
                    if got[tail] != want:
                        failures.append(where % name + ": tail = %d differs from the integer model" % tail)
    finally:
        for k, v in DEFAULTS.items():
            eng.set_option(k, v)
    assert ran and not failures, "%d of %d cases failed:\n  " % (len(failures), ran) + "\n  ".join(failures)
