"""The plan of the batched inner-product prover's mixed calls (python-bulletproofs_amd/csrc/ipa_prove_mixed_plan_host.hpp) checked on the
CPU: the header is plain C++, so tests/csrc_host/ipa_prove_mixed_plan_main.cpp -- a stand-alone program -- is compiled with the host
compiler (and the address and undefined-behaviour sanitizers) and prints, as JSON, the base lists of every class of a capacity, the
refusals, and for a list of classes the regions, the launches with their unit tables and the jobs."""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "csrc_host", "ipa_prove_mixed_plan_main.cpp")
INC = os.path.join(REPO, "python-bulletproofs_amd", "csrc")

SIZES = [1 << e for e in range(0, 11)]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ipa_prove_mixed_plan") / "ipa_prove_mixed_plan_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe])

    def call(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-4000:]
        return json.loads(r.stdout)
    return call


def up256(x):
    return (x + 255) & ~255


def log2(n):
    return n.bit_length() - 1


def transcript_bytes(k, protocol, seed):
    """ipp_transcript_bytes: numbers 79, points 45 characters with their '&'"""
    return (1 + (seed + 2) // 3 * 4 + 1 + 79 if protocol == 1 else 1 + seed) + k * (2 * 45 + 79)


def job_lanes_log2(n, njobs, opt):
    """rpp_job_lanes_log2: 16 lanes up to 128 elements; above, a wave while the launch has at most 4 096 jobs"""
    if opt:
        return {16: 4, 64: 6}[opt]
    return 6 if n > 128 and njobs <= 4096 else 4


# ---- base lists ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bases(run):
    return run("bases")


def test_class_bases_of_a_prover_of_its_own_are_the_plans(bases):
    assert sorted(int(n) for n in bases["own"]) == SIZES and all(bases["own"].values())


def test_class_bases_stay_inside_the_prefix_of_the_capacity(bases):
    """Every base lies below 1 + 2N and names g_j / h_j with j < n_c only; round r's L and R partition the 2 n_c generators of the
    prefix; the capacity array's offsets are disjoint and ordered."""
    for N in (1, 2, 8, 1024):
        cap = bases["capacities"][str(N)]
        at = cat = 0
        for n in [s for s in SIZES if s <= N]:
            c = cap["classes"][str(n)]
            k, bl = log2(n), c["bases"]
            assert c["off"] == at and c["len"] == len(bl) == 1 + k * 2 * (n + 1)
            at += len(bl)
            gs, hs = [1 + j for j in range(n)], [1 + N + j for j in range(n)]
            assert bl[0] == 0 and max(bl) < 1 + 2 * N and set(bl) <= set([0] + gs + hs)
            for r in range(k):
                ln = n >> r
                half = ln // 2
                o = 1 + r * 2 * (n + 1)
                L, R = bl[o: o + n + 1], bl[o + n + 1: o + 2 * (n + 1)]
                assert L[n] == 0 and R[n] == 0 and sorted(L[:n] + R[:n]) == gs + hs
                assert L[:n // 2] == [1 + j for j in range(n) if j % ln >= half] and L[n // 2: n] == [1 + N + j for j in range(n) if j % ln < half]
            # the statements' three lists: (a, b, u), (a, u), (b, u)
            cb, (o_ab, o_a, o_b) = c["commit_bases"], c["commit_offsets"]
            assert c["commit_off"] == cat and len(cb) == 4 * n + 3
            cat += len(cb)
            assert cb[o_ab: o_ab + 2 * n + 1] == gs + hs + [0] and cb[o_a: o_a + n + 1] == gs + [0] and cb[o_b: o_b + n + 1] == hs + [0]
        assert cap["total"] == cap["end"] == at and cap["commit_total"] == cap["commit_end"] == cat
    assert bases["capacities"]["1024"]["total"] == 36989 and bases["capacities"]["1024"]["commit_total"] == 8221      # the sizes the header states


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_from_the_shapes(run):
    for N in (0, 3, 2048):
        assert "power of two with 1 <= n <= 1024" in run("args", N, "1:1")["msg"]
    assert run("many", 1024, 64, 1, 1)["msg"] == ""
    assert run("many", 1024, 65, 1, 1)["msg"] == "n_classes must be at most 64"
    assert run("args", 8, "8:1")["null_classes"] == "null argument"
    for bad_n in (0, 3, 16, 1 << 20):
        assert run("args", 8, "4:1", "%d:1" % bad_n)["msg"] == "class 1: the vector length must be a power of two, at most the prover's"
    assert run("args", 8, "8:5", "2:3", "4:0")["msg"] == "class 2: n_proofs must be at least 1"
    # the caps at exactly 2^20 / 2^27 and one above
    assert run("args", 8, "1:%d" % (1 << 20))["msg"] == ""
    assert run("args", 8, "1:%d" % ((1 << 20) + 1))["msg"] == "at most 2^20 proofs per call"
    assert run("args", 8, "1:%d" % (1 << 19), "2:%d" % (1 << 19))["msg"] == ""
    assert run("args", 8, "1:%d" % (1 << 19), "2:%d" % ((1 << 19) + 1))["msg"] == "at most 2^20 proofs per call"
    assert run("args", 1024, "1024:%d" % (1 << 17))["msg"] == ""
    assert run("args", 1024, "1024:%d" % ((1 << 17) - 1), "512:2")["msg"] == ""
    assert run("args", 1024, "1024:%d" % ((1 << 17) - 1), "512:2", "1:1")["msg"] == "at most 2^27 elements (proofs x n) per call"
    assert run("args", 1024, "1024:%d" % ((1 << 17) + 1))["msg"] == "at most 2^27 elements (proofs x n) per call"
    # through the plan: the same texts, and the seed bound
    assert run("plan", 8, 2, 0, "16:1:0:0")["msg"] == "class 0: the vector length must be a power of two, at most the prover's"
    assert run("plan", 8, 2, 0, "8:1:0:0", "8:1:65535:0")["err"] == 0
    p = run("plan", 8, 2, 0, "8:1:0:0", "8:1:65536:0")
    assert p["err"] != 0 and p["msg"] == "class 1: a seed is longer than 65535 bytes"
    assert run("commit", 8, 0, 0, "8:1:1:1:0", "3:1:1:1:0")["msg"] == "class 1: the vector length must be a power of two, at most the prover's"


# ---- plans -----------------------------------------------------------------------------------------------------------------------
CLASS_LISTS = {
    "one": [(64, 7)],
    "all_eleven": [(n, 3) for n in SIZES],
    "eleven_descending": [(n, 2) for n in reversed(SIZES)],
    "two_of_one_n": [(4, 3), (64, 2), (4, 2)],
    "sixty_four": [(SIZES[i % 11], 1 + i % 3) for i in range(64)],
    "counts": [(2, 1), (2, 64), (2, 65), (4, 257), (512, 1), (1024, 2), (256, 65)],
    "no_rounds": [(1, 5), (1, 70)],
}


def _plan(run, name, protocol, lanes=0, seed=5):
    classes = CLASS_LISTS[name]
    args = ["%d:%d:%d:%d" % (n, count, seed + 3 * c, c % 2) for c, (n, count) in enumerate(classes)]
    return classes, run("plan", 1024, protocol, lanes, *args)


@pytest.mark.parametrize("protocol", [1, 2])
@pytest.mark.parametrize("name", sorted(CLASS_LISTS))
def test_regions_are_aligned_disjoint_and_inside_the_buffer(run, name, protocol):
    classes, p = _plan(run, name, protocol)
    assert p["err"] == 0 and p["N"] == 1024 and p["n_proofs"] == sum(c for _, c in classes)
    spans, first = [], 0
    for c, ((n, count), q) in enumerate(zip(classes, p["classes"])):
        k, seed = log2(n), 5 + 3 * c
        assert (q["n"], q["k"], q["count"], q["first"]) == (n, k, count, first)
        assert q["NT"] == (256 if n <= 256 else n) and q["per_block"] * n == q["NT"]
        first += count
        ds = ((((seed + 2) // 3) * 4 + 1 if protocol == 1 else 1 + seed) + 15) & ~15
        ts = (transcript_bytes(k, protocol, seed) + 15) & ~15
        assert (q["dig0_stride"], q["tr_stride"], q["tr_bytes"]) == (ds, ts, transcript_bytes(k, protocol, seed))
        sizes = dict(dig0=count * ds, dlen=4 * count, ain=32 * count * n, bin=32 * count * n, cin=32 * count if protocol == 1 and c % 2 else 0,
                     Pin=64 * count if protocol == 1 else 0, uc=32 * count, hsc=64 * count, xr=64 * count, a=32 * count * n, b=32 * count * n, cg=32 * count * n,
                     hf=32 * count * n, jsc=32 * 2 * count * (n + 1), jout=144 * 2 * count, ab=64 * count, xs=32 * count * k, lr=128 * count * k, head=128 * count,
                     trlen=4 * count, tr=count * ts)
        for part, lo, hi in (("inputs", 0, p["in_bytes"]), ("scratch", p["in_bytes"], p["o_out"]), ("outputs", p["o_out"], p["need"])):
            for name_, at in q[part].items():
                assert at % 256 == 0 and lo <= at and at + sizes[name_] <= hi, (c, name_)
                spans.append((at, at + sizes[name_]))
                if name_ == "Pin":
                    assert p["o_P"] <= at and at + up256(sizes[name_]) <= p["o_P_end"]
    # the call's device tables: inside the upload
    sb, sa, sj, su = p["slots"]
    assert (sa, sj, su) == (32, 48, 8) and sb >= 208
    nsteps = p["nsteps"]
    assert nsteps == 1 + p["k_max"] and p["k_max"] == max(log2(n) for n, _ in classes) and len(p["jobs"]) == nsteps * len(classes)
    for at, size in ((p["o_batch"], sb * len(classes)), (p["o_affine"], sa * len(classes)), (p["o_jobs"], sj * len(p["jobs"])), (p["o_units"], su * p["n_units"])):
        assert at % 256 == 0 and at + size <= p["in_bytes"]
        spans.append((at, at + size))
    spans = sorted(s for s in spans if s[1] > s[0])
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    assert p["in_bytes"] <= p["o_out"] <= p["need"] and p["need"] % 256 == 0
    # the outputs of all classes are contiguous: class c + 1's first output starts where class c's last one ends (rounded up to 256)
    at = p["o_out"]
    for (n, count), q in zip(classes, p["classes"]):
        k = log2(n)
        for name_, size in (("ab", 64 * count), ("xs", 32 * count * k), ("lr", 128 * count * k), ("head", 128 * count), ("trlen", 4 * count), ("tr", count * q["tr_stride"])):
            assert q["outputs"][name_] == at
            at += up256(size)
    assert at == p["need"]


@pytest.mark.parametrize("protocol", [1, 2])
@pytest.mark.parametrize("lanes", [0, 16, 64])
@pytest.mark.parametrize("name", sorted(CLASS_LISTS))
def test_launches_and_their_bounds(run, name, protocol, lanes):
    """Per step: one launch per one-lane-per-proof kernel and per 256-thread kernel, at most one per block size for the wide kernel, at
    most one k_pv_msm_mixed per lane width -- whatever the number of classes; round r holds exactly the classes with k_c > r; every
    class's unit covers its whole blocks."""
    classes, p = _plan(run, name, protocol, lanes)
    nc, k_max = len(classes), p["k_max"]
    steps = {}
    for L in p["launches"]:
        steps.setdefault(L["step"], []).append(L)
    assert [L["step"] for L in p["launches"]] == sorted(L["step"] for L in p["launches"]) and sorted(steps) == list(range(1 + k_max))
    for s, launches in steps.items():
        r = s - 1
        members = list(range(nc)) if s == 0 else [c for c, (n, _) in enumerate(classes) if log2(n) > r]
        assert members
        kinds = [L["kind"] for L in launches]
        want = ["k_ip_begin_mixed", "k_ip_round_wide_mixed"] + (["k_pv_msm_mixed", "k_ip_head_mixed"] if protocol == 1 else []) if s == 0 else \
            ["k_pv_msm_mixed", "k_ip_affine_mixed", "k_ip_round_chal_mixed", "k_ip_round_wide_mixed"]
        assert [k for i, k in enumerate(kinds) if i == 0 or kinds[i - 1] != k] == want, (s, kinds)
        for kind in ("k_ip_begin_mixed", "k_ip_head_mixed", "k_ip_affine_mixed", "k_ip_round_chal_mixed"):
            assert kinds.count(kind) == (1 if kind in want else 0)
        wide = [L for L in launches if L["kind"] == "k_ip_round_wide_mixed"]
        assert len(wide) <= 3 and len({L["threads"] for L in wide}) == len(wide) and {L["threads"] for L in wide} <= {256, 512, 1024}
        msm = [L for L in launches if L["kind"] == "k_pv_msm_mixed"]
        assert len(msm) <= 3 and len({L["gl"] for L in msm}) == len(msm) and {L["gl"] for L in msm} <= {1, 4, 6}
        total_jobs = sum(2 * classes[c][1] for c in members)
        seen = {}
        for L in launches:
            assert L["units"] and L["units"][0][1] == 0
            assert [u[0] for u in L["units"]] == sorted(u[0] for u in L["units"])              # the caller's order
            firsts = [u[1] for u in L["units"]] + [L["blocks"]]
            for (c, first), nxt in zip(L["units"], firsts[1:]):
                n, count = classes[c]
                blocks = nxt - first
                assert c in members and blocks >= 1
                seen.setdefault(L["kind"], []).append(c)
                if L["kind"] in ("k_ip_begin_mixed", "k_ip_round_chal_mixed"):
                    assert L["threads"] == 64 and blocks == -(-count // 64)
                elif L["kind"] in ("k_ip_head_mixed", "k_ip_affine_mixed"):
                    assert L["threads"] == 256 and blocks == -(-2 * count // 256)
                elif L["kind"] == "k_ip_round_wide_mixed":
                    NT = 256 if n <= 256 else n
                    assert L["threads"] == NT and blocks == -(-count // (NT // n)) and (L["round"], L["first"]) == ((0, 1) if s == 0 else (r, 0))
                else:
                    gl = 1 if s == 0 else job_lanes_log2(n, total_jobs, lanes)
                    assert L["threads"] == 256 and L["gl"] == gl and blocks == -(-(2 * count << gl) // 256)      # the class's job range covers whole blocks
            if L["kind"] in ("k_ip_affine_mixed", "k_ip_round_chal_mixed"):
                assert L["round"] == r
        for kind, cs in seen.items():
            assert sorted(cs) == members, (s, kind)                                             # every class of the step once per kernel, no other
        # the jobs of the step
        for c, (n, count) in enumerate(classes):
            j = p["jobs"][s * nc + c]
            if s == 0:
                assert j == ([2 * count, 1, 1, 1, 0, 1] if protocol == 1 else [0, 0, 0, 0, 0, 0])
            elif c in members:
                assert j == [2 * count, 2, n + 1, n + 1, 1 + r * 2 * (n + 1), 0]
            else:
                assert j == [0, 0, 0, 0, 0, 0]
    for (n, _), q in zip(classes, p["classes"]):
        assert q["bases_off"] == sum(1 + log2(m) * 2 * (m + 1) for m in SIZES if m < n)


@pytest.mark.parametrize("n,count,protocol,seed,have_c", [(1, 5, 1, 0, 0), (2, 70, 2, 3, 0), (64, 7, 1, 200, 1), (256, 3, 1, 17, 0), (512, 2, 2, 65535, 0), (1024, 2, 1, 1, 1)])
def test_a_one_class_plan_is_the_single_call_layout(run, n, count, protocol, seed, have_c):
    """The strides and region sizes bpmi_ipa_prove_batch computes for that n (ipa_prove_host.hpp), restated: the same arrays in the same
    order behind the same 256-byte cursor, with the call's device tables between the inputs and the scratch."""
    p = run("plan", n, protocol, 0, "%d:%d:%d:%d" % (n, count, seed, have_c))
    q, k, P = p["classes"][0], log2(n), count
    dig0_stride = ((((seed + 2) // 3) * 4 + 1 if protocol == 1 else 1 + seed) + 15) & ~15
    tr_stride = (transcript_bytes(k, protocol, seed) + 15) & ~15
    assert (q["dig0_stride"], q["tr_stride"]) == (dig0_stride, tr_stride)
    o = 0

    def take(size):
        nonlocal o
        at = o
        o += up256(size)
        return at
    want_in = dict(dig0=take(P * dig0_stride), dlen=take(4 * P), ain=take(32 * P * n), bin=take(32 * P * n), cin=take(32 * P if have_c and protocol == 1 else 0),
                   Pin=take(64 * P if protocol == 1 else 0))
    assert q["inputs"] == want_in
    tables = p["in_bytes"] - o
    assert tables == up256(p["slots"][0]) + up256(32) + up256(48 * (1 + k)) + up256(8 * p["n_units"])
    o = p["in_bytes"]
    want_scratch = dict(uc=take(32 * P), hsc=take(64 * P), xr=take(64 * P), a=take(32 * P * n), b=take(32 * P * n), cg=take(32 * P * n), hf=take(32 * P * n),
                        jsc=take(32 * 2 * P * (n + 1)), jout=take(144 * 2 * P))
    assert q["scratch"] == want_scratch and p["o_out"] == o
    want_out = dict(ab=take(64 * P), xs=take(32 * P * k), lr=take(128 * P * k), head=take(128 * P), trlen=take(4 * P), tr=take(P * tr_stride))
    assert q["outputs"] == want_out and p["need"] == o
    # its launches: the single call's sequence, one launch each
    kinds = [L["kind"] for L in p["launches"]]
    head = ["k_pv_msm_mixed", "k_ip_head_mixed"] if protocol == 1 else []
    assert kinds == ["k_ip_begin_mixed", "k_ip_round_wide_mixed"] + head + ["k_pv_msm_mixed", "k_ip_affine_mixed", "k_ip_round_chal_mixed", "k_ip_round_wide_mixed"] * k


# ---- the statements' plan --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u_mode", [0, 1, 2])
@pytest.mark.parametrize("lanes", [0, 16, 64])
def test_commit_plan(run, u_mode, lanes):
    classes = [(1, 5, 1, 1), (2, 65, 1, 1), (4, 3, 1, 0 if u_mode != 1 else 1), (64, 2, 0 if u_mode != 1 else 1, 1), (256, 2, 1, 1), (512, 1, 1, 1), (1024, 2, 1, 1), (4, 2, 1, 1)]
    args = ["%d:%d:%d:%d:%d" % (n, count, a, b, 1 if u_mode == 2 else 0) for n, count, a, b in classes]
    p = run("commit", 1024, u_mode, lanes, *args)
    assert p["err"] == 0 and p["count"] == sum(c[1] for c in classes)
    spans, at = [], p["o_out"]
    total = p["count"]
    for (n, count, a, b), q in zip(classes, p["classes"]):
        T = (n if a else 0) + (n if b else 0) + (1 if u_mode else 0)
        assert (q["n"], q["count"], q["T"]) == (n, count, T) and q["NT"] == (256 if n <= 256 else n) and q["per_block"] * n == q["NT"]
        off = sum(4 * m + 3 for m in SIZES if m < n) + (0 if a and b else 2 * n + 1 if a else 3 * n + 2)
        assert q["bases_off"] == off
        sizes = dict(ain=32 * count * n if a else 0, bin=32 * count * n if b else 0, tin=32 * count if u_mode == 2 else 0, jsc=32 * count * T, jout=144 * count, pts=64 * count)
        for name_ in ("ain", "bin", "tin"):
            assert q[name_] % 256 == 0 and q[name_] + sizes[name_] <= p["in_bytes"]
        for name_ in ("jsc", "jout"):
            assert q[name_] % 256 == 0 and p["in_bytes"] <= q[name_] and q[name_] + sizes[name_] <= p["o_out"]
        assert q["pts"] == at and at % 64 == 0                       # the points of all classes back to back
        at += 64 * count
        spans += [(q[name_], q[name_] + sizes[name_]) for name_ in sizes]
    assert at <= p["need"] and p["need"] % 256 == 0
    sc, sa, sj, su = p["slots"]
    for o_, size in ((p["o_commit"], sc * len(classes)), (p["o_affine"], sa * len(classes)), (p["o_jobs"], sj * len(classes)), (p["o_units"], su * p["n_units"])):
        assert o_ % 256 == 0 and o_ + size <= p["in_bytes"]
        spans.append((o_, o_ + size))
    spans = sorted(s for s in spans if s[1] > s[0])
    assert all(x[1] <= y[0] for x, y in zip(spans, spans[1:]))
    kinds = [L["kind"] for L in p["launches"]]
    assert [k for i, k in enumerate(kinds) if i == 0 or kinds[i - 1] != k] == ["k_ip_commit_scalars_mixed", "k_pv_msm_mixed", "k_ip_affine_mixed"]
    assert kinds.count("k_ip_commit_scalars_mixed") == 3 and kinds.count("k_pv_msm_mixed") <= 3 and kinds.count("k_ip_affine_mixed") == 1
    for L in p["launches"]:
        firsts = [u[1] for u in L["units"]] + [L["blocks"]]
        for (c, first), nxt in zip(L["units"], firsts[1:]):
            n, count = classes[c][:2]
            if L["kind"] == "k_ip_commit_scalars_mixed":
                assert L["threads"] == (256 if n <= 256 else n) and nxt - first == -(-count // (L["threads"] // n))
            elif L["kind"] == "k_pv_msm_mixed":
                gl = job_lanes_log2(n, total, lanes)
                assert L["gl"] == gl and nxt - first == -(-(count << gl) // 256)
            else:
                assert nxt - first == -(-count // 256)
    for kind in set(kinds):
        assert sorted(u[0] for L in p["launches"] if L["kind"] == kind for u in L["units"]) == list(range(len(classes)))


# ---- the C example ---------------------------------------------------------------------------------------------------------------
def test_the_c_example_builds_against_the_header_and_the_library(tmp_path):
    """examples/ipa_prove_mixed_c_abi.c is C99 over include/bpmi.h and libbpmi.so alone: it compiles without a warning and links (it
    RUNS in the GPU suite, tests/test_gpu_ipa_prove_batch_mixed.py)."""
    import bulletproofs_amd  # noqa: F401
    from bulletproofs_amd import build as B
    B.build()
    libdir = os.path.join(REPO, "python-bulletproofs_amd")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"),
                           os.path.join(REPO, "examples", "ipa_prove_mixed_c_abi.c"), "-o", str(tmp_path / "ipa_prove_mixed_c_abi"),
                           os.path.join(libdir, "libbpmi.so"), "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined"])
