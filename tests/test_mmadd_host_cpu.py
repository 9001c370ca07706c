"""xyzz_mmadd (python-bulletproofs_amd/csrc/curve.hpp), the affine + affine addition that the accumulation by runs uses for the second
entry of a run, and segs_one_dense (shared_defs.hpp), the host predicate that picks the dense instantiation of k_accum_runs -- checked
on the CPU: tests/csrc_host/mmadd_main.cpp, a stand-alone program, is compiled with the host compiler under ASan + UBSan and its lines
are compared with Python integers mod p (the affine group law after X / ZZ, Y / ZZZ).  The addition formulas are identities in x and y
(the curve's b never enters them, and a = 0), so operands at the edge of their limb contracts need not be curve points."""
import os
import random
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "csrc_host", "mmadd_main.cpp")
INC = os.path.join(REPO, "python-bulletproofs_amd", "csrc")

P = 2**256 - 2**32 - 977
M29 = (1 << 29) - 1
BIAS2 = [0x3FFFF85E, 0x3FFFFFEE] + [0x3FFFFFFE] * 6 + [0x01FFFFFE]             # field.hpp BPMI_FE_BIAS2: 2p, every limb above a tight one
TIGHT_MAX = [M29] * 8 + [(1 << 24) + (1 << 20)]                                 # field.hpp "Magnitudes"
LOOSE_MAX = [(1 << 29) + (1 << 22) - 1, (1 << 29) + (1 << 15) - 1] + [M29] * 6 + [(1 << 24) - 1]
assert sum(b << (29 * k) for k, b in enumerate(BIAS2)) == 2 * P


def limbs(v):
    """the limbs fe_from_words gives a 256-bit value"""
    assert 0 <= v < 1 << 256
    return [(v >> (29 * k)) & M29 for k in range(8)] + [v >> 232]


def val(l):
    return sum(x << (29 * k) for k, x in enumerate(l))


def lazy_neg(l):
    """fe_neg: 2p - a, limb by limb (magnitude 2)"""
    return [b - x for b, x in zip(BIAS2, l)]


def affine_add(x1, y1, x2, y2):
    """the affine group law on residues; None = the identity"""
    x1, y1, x2, y2 = x1 % P, y1 % P, x2 % P, y2 % P
    if x1 == x2:
        if (y1 + y2) % P == 0:
            return None
        assert y1 == y2, "equal x with unrelated y: not a case of the group law"
        lam = 3 * x1 * x1 * pow(2 * y1, -1, P) % P
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, P) % P
    x3 = (lam * lam - x1 - x2) % P
    return x3, (lam * (x1 - x3) - y1) % P


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mmadd") / "mmadd_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe])

    def go(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-500:] + r.stderr[-3000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
        out = r.stdout.split("\n")[:-1]
        assert len(out) == len(lines)
        return out
    return go


def hexes(*ls):
    return " ".join("%x" % x for l in ls for x in l)


def parse(line):
    w = [int(x, 16) for x in line.split()]
    assert len(w) == 36
    return w[0:9], w[9:18], w[18:27], w[27:36]


def check_record(line, want, what):
    X, Y, ZZ, ZZZ = parse(line)
    if want is None:
        assert X + Y + ZZ + ZZZ == [0] * 36, what          # THE identity record: 36 zero words
        return
    for f in (X, Y, ZZ, ZZZ):                              # loose, as the mixed addition leaves its accumulator
        assert all(a <= b for a, b in zip(f, LOOSE_MAX)), (what, f)
    zz, zzz = val(ZZ) % P, val(ZZZ) % P
    assert zz != 0 and pow(zz, 3, P) == zzz * zzz % P, what
    assert val(X) * pow(zz, -1, P) % P == want[0], what
    assert val(Y) * pow(zzz, -1, P) % P == want[1], what


def curve_point(rnd):
    while True:
        x = rnd.randrange(P)
        y = pow(x * x * x + 7, (P + 1) // 4, P)
        if y * y % P == (x * x * x + 7) % P:
            return x, (y if rnd.random() < 0.5 else P - y)


def test_mmadd_matches_the_affine_group_law(run):
    rnd = random.Random(20260)
    cases = []                                             # (x1 limbs, y1 limbs, x2 limbs, y2 limbs, what)
    for i in range(40):                                    # random pairs of curve points, y2 plain or the lazy 2p - y
        (x1, y1), (x2, y2) = curve_point(rnd), curve_point(rnd)
        cases.append((limbs(x1), limbs(y1), limbs(x2), limbs(y2) if i % 2 else lazy_neg(limbs(y2)), "random %d" % i))
    for i in range(20):                                    # random residues (the formulas are identities)
        v = [rnd.randrange(P) for _ in range(4)]
        cases.append((limbs(v[0]), limbs(v[1]), limbs(v[2]), limbs(v[3]), "residues %d" % i))
    # every operand at its contract's largest limbs: x1, y1, x2 tight or loose maxima; y2 those or the lazy form of the smallest / largest y
    mid = limbs(rnd.randrange(P))
    edge_y2 = [TIGHT_MAX, LOOSE_MAX, lazy_neg([0] * 9), lazy_neg(TIGHT_MAX), lazy_neg(LOOSE_MAX), lazy_neg(mid)]
    for a, x1 in enumerate((TIGHT_MAX, LOOSE_MAX, mid)):
        for b, y1 in enumerate((TIGHT_MAX, LOOSE_MAX, mid)):
            for c, x2 in enumerate((TIGHT_MAX, LOOSE_MAX, [0] * 9, mid)):
                if val(x1) % P == val(x2) % P:
                    continue                               # (equal x: the exceptional cases have their own test)
                for d, y2 in enumerate(edge_y2):
                    cases.append((x1, y1, x2, y2, "edge %d%d%d%d" % (a, b, c, d)))
    # x or y equal to 0, 1, p - 1 (and the alias p of 0)
    small = [0, 1, P - 1, P]
    for x1 in small:
        for x2 in small:
            if x1 % P == x2 % P:
                continue
            for y1 in small:
                for y2 in small:
                    cases.append((limbs(x1), limbs(y1), limbs(x2), limbs(y2) if (x1 + y1) % 2 else lazy_neg(limbs(y2)), "small %d %d %d %d" % (x1, y1, x2, y2)))
    out = run(["mmadd " + hexes(c[0], c[1], c[2], c[3]) for c in cases])
    for c, line in zip(cases, out):
        check_record(line, affine_add(val(c[0]), val(c[1]), val(c[2]), val(c[3])), c[4])


def test_mmadd_exceptional_cases_and_alias_encodings(run):
    rnd = random.Random(20261)
    pts = [curve_point(rnd) for _ in range(8)]
    pts += [(5, 9), (0, 1), (1, P - 1), (2**32 + 976, 2**32 + 976), (3, 0x1234567)]       # residues small enough for the alias v + p < 2^256
    dbl_cases, inf_cases = [], []
    for x, y in pts:
        xs = [limbs(x)] + ([limbs(x + P)] if x + P < 1 << 256 else [])
        ys = [limbs(y)] + ([limbs(y + P)] if y + P < 1 << 256 else [])
        nys = [limbs(P - y), lazy_neg(limbs(y))] + ([lazy_neg(limbs(y + P)), limbs(2 * P - y)] if y + P < 1 << 256 and 2 * P - y < 1 << 256 else [])
        for x1 in xs:
            for x2 in xs:
                for y1 in ys:
                    for y2 in ys + [lazy_neg(n) for n in nys[:1]]:          # y, its alias, and 2p - (p - y)
                        dbl_cases.append((x1, y1, x2, y2))
                    for y2 in nys:
                        inf_cases.append((x1, y1, x2, y2))
    assert any(c[0] != c[2] for c in dbl_cases) and any(c[0] != c[2] for c in inf_cases)      # equal x through DIFFERENT encodings
    out = run(["mmadd " + hexes(*c) for c in dbl_cases])
    for c, line in zip(dbl_cases, out):
        if val(c[1]) % P == 0:
            continue                                       # (y = 0 is its own negative: no such point on a prime-order curve)
        check_record(line, affine_add(val(c[0]), val(c[1]), val(c[2]), val(c[3])), "P = Q")
    for c, line in zip(inf_cases, run(["mmadd " + hexes(*c) for c in inf_cases])):
        check_record(line, None, "P = -Q")
    # P = Q is the affine doubling itself, limb for limb, of the addend with its y carried (canonical operands: the carry changes nothing)
    canon = [(limbs(x), limbs(y)) for x, y in pts[:8]]
    a = run(["mmadd " + hexes(x, y, x, y) for x, y in canon])
    b = run(["dbl " + hexes(x, y) for x, y in canon])
    assert a == b


def test_dense_predicate(run):
    D = 0xFF                                               # segs_init's "no half-block selection"
    #        n0    n1   n2   total hlog      phase    glv  dense
    cases = [((1000, 0, 0, 1000, D, D, D, 0, 0, 0, 0), 1),
             ((1 << 20, 0, 0, 1 << 20, 32, D, D, 0, 0, 0, 0), 1),            # hlog >= 32 is dense
             ((1, 0, 0, 1, D, D, D, 0, 0, 0, 0), 1),
             ((600, 400, 0, 1000, D, D, D, 0, 0, 0, 0), 0),                  # two segments
             ((500, 300, 200, 1000, D, D, D, 0, 0, 0, 0), 0),                # three
             ((0, 1000, 0, 1000, D, D, D, 0, 0, 0, 0), 0),
             ((1000, 0, 0, 1000, 3, D, D, 0, 0, 0, 0), 0),                   # half-block selection, phase 0
             ((1000, 0, 0, 1000, 3, D, D, 1, 0, 0, 0), 0),                   # ... phase 1
             ((1000, 0, 0, 1000, 0, D, D, 1, 0, 0, 0), 0),
             ((1000, 0, 0, 1000, 31, D, D, 0, 0, 0, 0), 0),
             ((1000, 0, 0, 1000, D, D, D, 0, 0, 0, 1), 0),                   # GLV
             ((1000, 0, 0, 999, D, D, D, 0, 0, 0, 0), 0),                    # n[0] != total
             ((1000, 0, 0, 2000, D, D, D, 0, 0, 0, 0), 0)]
    out = run(["dense " + " ".join(str(x) for x in c) for c, _ in cases])
    assert [int(x) for x in out] == [w for _, w in cases]
