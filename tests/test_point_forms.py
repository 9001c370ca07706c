"""The group law of csrc/curve.hpp at every limb form its contract admits, on the host build of the header (the device build is
compared with it limb for limb in tests/test_gpu_point_forms.py).

curve.hpp takes XYZZ and Jacobian records whose coordinates are tight or loose (field.hpp: tight = limbs 0..7 < 2^29, limb 8 <=
2^24 + 2^20; loose = limb 0 < 2^29 + 2^22, limb 1 < 2^29 + 2^15, limbs 2..7 < 2^29, limb 8 < 2^24) and affine addends whose y is
lazy (magnitude <= 2).  Random points almost never come in any form but the canonical one, so the cases here search the
projective scaling (or construct the point) until the form a case targets exists: value + p where that is still tight, the
borrow forms where limb 0 or limb 1 carries an extra 2^29, 2p - y and the other lazy forms of an affine y.  Around them: P + P
under different scalings and forms, P + (-P), the identity on either side and on both with ZZ (Z) as all zeros and as the limbs
of p.  Every result is decoded and checked against the oracle's affine group law."""
import ctypes
import random

from oracle import cbind
from oracle.ec import INF, Point, secp256k1
from test_csrc_host import M29, P, limbs_value, shim  # noqa: F401

TIGHT8 = (1 << 24) + (1 << 20)
BIAS2 = [0x3FFFF85E, 0x3FFFFFEE] + [0x3FFFFFFE] * 6 + [0x01FFFFFE]
PL = [(P >> (29 * k)) & M29 for k in range(9)]
# op -> (form of a, form of b): 'x' XYZZ record, 'j' Jacobian record, 'a' affine addend (y lazy), 't' affine (y tight / loose)
OPS = {0: ("x", "x"), 1: ("x", None), 2: ("x", "a"), 3: (None, "t"), 4: ("j", None), 5: ("j", "a"), 6: ("x", None), 7: ("j", None),
       8: ("x", "x"), 9: ("x", None)}
NAMES = {0: "xyzz_add", 1: "xyzz_dbl", 2: "xyzz_madd", 3: "xyzz_dbl_affine", 4: "jac_dbl", 5: "jac_madd", 6: "xyzz_to_affine",
         7: "jac_to_affine", 8: "xyzz_add(r, r, b)", 9: "xyzz_dbl(r, r)"}
PROJ_TARGETS = ("plus_p", "b0", "b1")


def limbs(v):
    return [(v >> (29 * k)) & M29 for k in range(9)]


def is_tight(l):
    return all(x < 1 << 29 for x in l[:8]) and l[8] <= TIGHT8


def is_loose(l):
    return l[0] < (1 << 29) + (1 << 22) and l[1] < (1 << 29) + (1 << 15) and all(x < 1 << 29 for x in l[2:8]) and l[8] < 1 << 24


def admits(v, form):
    """does 0 < v < p have a tight / loose representative of this form?"""
    if form == "plus_p":
        return v + P < (1 << 256) + (TIGHT8 - (1 << 24) + 1 << 232)
    if form == "b0":
        return v & M29 < 1 << 22 and (v >> 29) & M29 >= 1
    if form == "b1":
        return (v >> 29) & M29 < 1 << 15 and (v >> 58) & M29 >= 1
    return True


def proj_forms(v):
    """the tight or loose limb vectors of v (0 <= v < p): name -> limbs.  0 also has the limbs of p."""
    c = limbs(v)
    out = {"canon": c}
    if v == 0:
        out["p"] = list(PL)
    if v and admits(v, "plus_p"):
        out["plus_p"] = limbs(v + P)
    if v and admits(v, "b0"):
        out["b0"] = [c[0] + (1 << 29), c[1] - 1] + c[2:]
    if v and admits(v, "b1"):
        out["b1"] = [c[0], c[1] + (1 << 29), c[2] - 1] + c[3:]
    if "b0" in out and "b1" in out and c[1] >= 1:
        out["b01"] = [c[0] + (1 << 29), c[1] - 1 + (1 << 29), c[2] - 1] + c[3:]
    for name, l in out.items():
        assert limbs_value(l) % P == v and (is_tight(l) or is_loose(l)), (name, v)
    return out


def lazy_forms(v):
    """the forms of an affine y (magnitude <= 2: limbs 0..7 < 2^30, limb 8 < 2 (2^24 + 2^20)): the tight / loose ones, y + p limb
    by limb, 2p - (p - y) as fe_neg writes it (also of the loose forms of p - y), one borrow of 2^29 in any limb, all of them"""
    c = limbs(v)
    out = dict(proj_forms(v))
    out["plus_p_limbwise"] = [x + y for x, y in zip(c, PL)]
    for name, l in proj_forms((P - v) % P).items():
        out["neg_" + name] = [b - x for b, x in zip(BIAS2, l)]
    for k in range(8):
        if c[k + 1] >= 1:
            w = list(c)
            w[k] += 1 << 29
            w[k + 1] -= 1
            out["borrow%d" % k] = w
    if c[8] >= 1:
        w = list(c)
        for k in range(8):
            w[k] += 1 << 29
            w[k + 1] -= 1
        out["borrow_all"] = w
    out = {n: l for n, l in out.items() if all(x < 1 << 30 for x in l[:8]) and l[8] < 2 * TIGHT8}
    for name, l in out.items():
        assert limbs_value(l) % P == v, name
    return out


def coords(kind, pt, z):
    zz = z * z % P
    if kind == "j":
        return [pt.x * zz % P, pt.y * zz * z % P, z]
    return [pt.x * zz % P, pt.y * zz * z % P, zz, zz * z % P]


_MEMO = {}


def memo(key, make):
    """the searches below are the same for every op: each runs once, with a Random of its own (the result does not depend on the
    order in which the ops ask for it)"""
    if key not in _MEMO:
        _MEMO[key] = make(random.Random(repr(key)))
    return _MEMO[key]


def oracle_points():
    return memo("pool", lambda rnd: cbind.ec_mul_batch([secp256k1.G] * 64, [rnd.randrange(1, secp256k1.q) for _ in range(64)]))


def search_scaling(kind, target, rnd):
    """(point, z) such that the target form exists: target (coordinate, form) or 'all' (every coordinate non-canonical)"""
    pt = rnd.choice(oracle_points())
    while True:
        z = rnd.randrange(1, P)
        vals = coords(kind, pt, z)
        if target == "all":
            if all(any(admits(v, f) for f in PROJ_TARGETS) for v in vals):
                return pt, z
        elif admits(vals[target[0]], target[1]):
            return pt, z


class Gen:
    """records of points under projective scalings, each coordinate in a form its contract admits"""

    def __init__(self, rnd):
        self.rnd = rnd
        self.pool = oracle_points()

    def point(self):
        return self.rnd.choice(self.pool)

    def pick(self, forms, largest=False):
        if largest:                                            # the form with the largest limbs (by the sum of their sizes)
            return max(forms.values(), key=lambda l: sum(x.bit_length() for x in l))
        return forms[self.rnd.choice(sorted(forms))]

    def record(self, kind, pt, target=None, largest=False, z=None):
        """kind 'x' / 'j'; target None, (coordinate, form) or 'all' (every coordinate non-canonical; z from search_scaling); the
        other coordinates take a random admissible form (the largest one with largest=True)"""
        if pt == INF:
            return self.identity(kind)
        vals = coords(kind, pt, z or self.rnd.randrange(1, P))
        rec = []
        for i, v in enumerate(vals):
            forms = proj_forms(v)
            if target == "all":
                forms = {n: l for n, l in forms.items() if n != "canon"}
            rec += forms[target[1]] if (target not in (None, "all") and i == target[0]) else self.pick(forms, largest)
        return rec + [0] * (36 - len(rec))

    def identity(self, kind):
        """ZZ (Z) as all zeros or as the limbs of p; the other coordinates zero, as set_inf writes them, or those of a real point"""
        rnd = self.rnd
        zero = rnd.choice(([0] * 9, list(PL)))
        if rnd.randrange(2):
            xy = [0] * 18 if kind == "x" else [0] * 9 + [1] + [0] * 8
        else:
            xy = self.record(kind, self.point())[:18]
        rest = ([rnd.choice(([0] * 9, list(PL)))] if kind == "x" else [])
        rec = xy + zero + sum(rest, [])
        return rec + [0] * (36 - len(rec))

    def affine(self, pt, lazy, xform=None, yform=None, largest=False):
        """an affine addend: x tight / loose, y lazy (lazy=True) or tight / loose"""
        xf = proj_forms(pt.x)
        yf = lazy_forms(pt.y) if lazy else proj_forms(pt.y)
        x = xf[xform] if xform else self.pick(xf, largest)
        y = yf[yform] if yform else self.pick(yf, largest)
        return x + y + [0] * 18

    def affine_point_with(self, form, coord):
        return memo(("affine", form, coord), lambda rnd: affine_point_with(form, coord, rnd))


def affine_point_with(form, coord, rnd):
    """a curve point whose x (coord 0: drawn with the limb bits the form needs, then lifted) or y (coord 1: searched) admits
    `form`"""
    while True:
        x = rnd.randrange(1, P)
        if coord == 0 and form == "plus_p":
            x &= (1 << 251) - 1
        elif coord == 0 and form == "b0":
            x &= ~((M29 >> 7) << 22)
        elif coord == 0 and form == "b1":
            x &= ~((M29 >> 14) << 44)
        x |= 1 << 58
        rhs = (x * x * x + 7) % P
        y = pow(rhs, (P + 1) // 4, P)
        if x >= P or y * y % P != rhs:
            continue
        if coord == 0 and admits(x, form):
            return Point(x, y if rnd.randrange(2) else P - y, secp256k1)
        for yy in (y, P - y):
            if coord == 1 and admits(yy, form):
                return Point(x, yy, secp256k1)


def want_of(op, a, b):
    if op in (0, 2, 5, 8):
        return a + b
    if op in (1, 4, 9):
        return a + a
    if op == 3:
        return b + b
    return a


def point_cases(op, rnd, n_random=300):
    """(a record, b record, expected point) for op: every coordinate of every input in every non-canonical form, all coordinates
    at once in their largest forms, the special relations, random cases -- shuffled, so that special cases and general ones share
    waves on the device"""
    g = Gen(rnd)
    ka, kb = OPS[op]
    none = [0] * 36
    cases = []

    def add(pa, pb, ra, rb):
        cases.append((ra if ka else none, rb if kb else none, want_of(op, pa, pb)))

    def rec(kind, pt, **kw):
        if kind in ("x", "j"):
            return g.record(kind, pt, **kw)
        return g.affine(pt, kind == "a", **kw)

    targets = {"x": [(c, f) for c in range(4) for f in PROJ_TARGETS] + ["all"], "j": [(c, f) for c in range(3) for f in PROJ_TARGETS] + ["all"]}
    for side, kind in ((0, ka), (1, kb)):
        if kind is None:
            continue
        other = kb if side == 0 else ka
        if kind in ("x", "j"):
            for t in targets[kind]:
                for largest in (False, True):
                    pt, z = memo((kind, t, largest), lambda r: search_scaling(kind, t, r))
                    pa, pb = (pt, g.point()) if side == 0 else (g.point(), pt)
                    r = g.record(kind, pt, target=t, largest=largest, z=z)
                    o = rec(other, pb if side == 0 else pa, largest=largest) if other else none
                    add(pa, pb, *((r, o) if side == 0 else (o, r)))
        else:
            for coord in (0, 1):
                for form in PROJ_TARGETS:
                    for largest in (False, True):
                        pa, pb = g.point(), g.affine_point_with(form, coord)
                        kw = {"xform" if coord == 0 else "yform": form}
                        add(pa, pb, rec(ka, pa, largest=largest) if ka else none, g.affine(pb, kind == "a", largest=largest, **kw))
            pa, pb = g.point(), g.point()
            for yform in sorted(lazy_forms(pb.y) if kind == "a" else proj_forms(pb.y)):
                add(pa, pb, rec(ka, pa) if ka else none, g.affine(pb, kind == "a", yform=yform))
    # special relations: P + P (different scalings and forms), P + (-P), the identity on either side and on both
    for _ in range(40):
        pt = g.point()
        if kb in ("x", "a"):
            add(pt, pt, rec(ka, pt), rec(kb, pt))
            add(pt, -pt, rec(ka, pt), rec(kb, -pt))
            add(pt, pt, rec(ka, pt, largest=True), rec(kb, pt, largest=True))
            add(pt, -pt, rec(ka, pt, largest=True), rec(kb, -pt, largest=True))
            if kb == "a":                                       # the negated addend as xyzz_madd_signed hands it in: fe_neg(y)
                add(pt, -pt, rec(ka, pt), limbs(pt.x) + [b - x for b, x in zip(BIAS2, limbs(pt.y))] + [0] * 18)
            add(INF, pt, rec(ka, INF), rec(kb, pt))
            if kb == "x":
                add(pt, INF, rec(ka, pt), rec(kb, INF))
                add(INF, INF, rec(ka, INF), rec(kb, INF))
        elif ka:
            add(INF, None, rec(ka, INF), none)
    for _ in range(n_random):
        pa, pb = g.point(), g.point()
        add(pa, pb, rec(ka, pa) if ka else none, rec(kb, pb) if kb else none)
    rnd.shuffle(cases)
    return cases


def decode(op, rec):
    """the point a result record stands for, checking its limb form on the way"""
    if op in (6, 7):
        x, y = limbs_value(rec[0:9]), limbs_value(rec[9:18])
        assert all(v <= M29 for v in rec[:18]) and x < P and y < P and not any(rec[18:]), rec
        return INF if (x, y) == (0, 0) else (x, y)
    n = 3 if op in (4, 5) else 4
    cs = [rec[9 * k: 9 * k + 9] for k in range(n)]
    assert all(is_tight(c) or is_loose(c) for c in cs), rec
    assert not any(rec[9 * n:]), rec
    v = [limbs_value(c) % P for c in cs]
    if n == 3:
        if v[2] == 0:
            return INF
        zi = pow(v[2], -1, P)
        return (v[0] * zi * zi % P, v[1] * zi * zi * zi % P)
    if v[2] == 0:
        return INF
    assert v[3] and pow(v[2], 3, P) == v[3] * v[3] % P, rec                  # a consistent (Z^2, Z^3) pair
    return (v[0] * pow(v[2], -1, P) % P, v[1] * pow(v[3], -1, P) % P)


def flat(recs):
    return (ctypes.c_uint32 * (36 * len(recs)))(*[v for r in recs for v in r])


def host_point_op(L, op, cases):
    n = len(cases)
    L.t_point_op.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32,
                             ctypes.POINTER(ctypes.c_uint32)]
    out = (ctypes.c_uint32 * (36 * n))()
    L.t_point_op(op, flat([c[0] for c in cases]), flat([c[1] for c in cases]), n, out)
    got = list(out)
    return [got[36 * i: 36 * i + 36] for i in range(n)]


def check_against_oracle(op, cases, results):
    for i, ((ra, rb, want), rec) in enumerate(zip(cases, results)):
        got = decode(op, rec)
        assert got == (INF if want == INF else (want.x, want.y)), (NAMES[op], i, ra, rb)


def test_the_inputs_reach_every_form(shim):  # noqa: F811
    """the case lists hold what the tests below rely on: every input coordinate in a non-canonical form, and special relations"""
    for op in sorted(OPS):
        cases = point_cases(op, random.Random(100 + op), n_random=0)
        ka, kb = OPS[op]
        for side, kind in ((0, ka), (1, kb)):
            if kind is None:
                continue
            n = {"x": 4, "j": 3, "a": 2, "t": 2}[kind]
            for c in range(n):
                l = [case[side][9 * c: 9 * c + 9] for case in cases]
                assert any(x[0] >= 1 << 29 for x in l) and any(x[1] >= 1 << 29 for x in l), (op, side, c)
                if kind in ("x", "j") or c == 0:
                    assert any(x[8] > (1 << 24) for x in l), (op, side, c)           # value + p
        if ka in ("x", "j"):
            assert any(limbs_value(case[0][18:27]) == 0 for case in cases) and any(case[0][18:27] == PL for case in cases), op


def test_group_law_at_every_admissible_representative(shim):  # noqa: F811
    """xyzz_add, xyzz_dbl, xyzz_madd, xyzz_dbl_affine, jac_dbl, jac_madd, the two *_to_affine and the aliased xyzz_add(r, r, b) /
    xyzz_dbl(r, r) (host build) against the oracle's affine group law; every output coordinate tight or loose"""
    for op in sorted(OPS):
        cases = point_cases(op, random.Random(op))
        check_against_oracle(op, cases, host_point_op(shim, op, cases))
