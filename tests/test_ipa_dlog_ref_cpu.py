"""The integer model of tests/ipa_dlog_ref.py against the C oracle on explicit points, and -- from the model alone -- the proof that
every scenario shows the edge it is there for, so that no case of test_gpu_ipa_degenerate.py can be vacuous."""
import pytest

import ipa_dlog_ref as D
from ipa_dlog_ref import IOTA, LAMBDA, Q
from oracle import cbind
from oracle.ec import secp256k1

G = secp256k1.G


def test_constants():
    assert IOTA * IOTA % Q == Q - 1 and pow(IOTA, -1, Q) == Q - IOTA
    assert pow(LAMBDA, 3, Q) == 1 and LAMBDA != 1
    assert D.glv_split(1) == (1, 0) and D.glv_split(Q - 1) == (-1, 0)
    assert D.glv_split(LAMBDA) == (0, 1) and D.glv_split(Q - LAMBDA) == (0, -1)
    assert D.glv_split(LAMBDA * LAMBDA) == (-1, -1)
    # the endomorphism on the curve: lambda G = (beta x, y)
    lg = cbind.ec_mul_batch([G], [LAMBDA])[0]
    assert lg.y == G.y and lg.x != G.x and pow(lg.x * pow(G.x, -1, secp256k1.p), 3, secp256k1.p) == 1


def test_dlogs_to_le64():
    got = D.dlogs_to_le64([0, 1, Q - 1, 5, 1, Q + 5])
    assert got[0] == bytes(64) and got[1] == got[4] == cbind.pack_points([G]) and got[2] == cbind.pack_points([-G])
    assert got[3] == got[5] == cbind.pack_points([5 * G])


@pytest.mark.parametrize("n", [16, 64])
@pytest.mark.parametrize("name,scaled", [("control", False), ("control", True), ("identities", False), ("identities", True),
                                         ("halves_equal_iota", False)])
def test_model_vs_oracle_on_points(name, n, scaled):
    """Every round's L and R, the folded generators and vectors and the final scalars: the model's integers times G against
    cbind.msm / ec_lincomb2_batch / sc_fold over the explicit points (the loop of test_ipa_rounds_vs_oracle)."""
    sg, sh, su, a, b, xs, hscale = D.scenario(name, n, scaled)
    m = D.DlogIpa(sg, sh, su, a, b, hscale)
    pts = cbind.unpack_points(b"".join(D.dlogs_to_le64(sg + sh + [su])), 2 * n + 1)
    g, h, u = pts[:n], pts[n:2 * n], pts[2 * n]
    if hscale is not None:
        h = cbind.ec_mul_batch(h, hscale)
    for r, x in enumerate(xs):
        half = len(g) // 2
        cl, cr = cbind.sc_dot(a[:half], b[half:]), cbind.sc_dot(a[half:], b[:half])
        wantL = cbind.msm(g[half:] + h[:half] + [u], a[:half] + b[half:] + [cl])
        wantR = cbind.msm(g[:half] + h[half:] + [u], a[half:] + b[:half] + [cr])
        L, R = D.dlogs_to_le64(m.round_LR())
        assert (L, R) == (cbind.pack_points([wantL]), cbind.pack_points([wantR])), (name, n, r)
        xi = pow(x, -1, Q)
        m.fold(x, xi)
        g = cbind.ec_lincomb2_batch(g[:half], g[half:], xi, x)
        h = cbind.ec_lincomb2_batch(h[:half], h[half:], x, xi)
        a = cbind.sc_fold(a[:half], a[half:], x, xi)
        b = cbind.sc_fold(b[:half], b[half:], xi, x)
        eg, eh, ea, eb = m.export()
        assert b"".join(D.dlogs_to_le64(eg)) == cbind.pack_points(g) and b"".join(D.dlogs_to_le64(eh)) == cbind.pack_points(h), (name, n, r)
        assert (ea, eb) == (a, b), (name, n, r)
    assert m.finish() == (a[0], b[0])


def test_expected_trace_is_the_model_in_wire_bytes():
    events, case = D.expected_trace("identities", 64, scaled=True)
    sg, sh, su, a, b, xs, hscale = case
    m = D.DlogIpa(sg, sh, su, a, b, hscale)
    assert [e[:2] for e in events[:3]] == [("LR", 64), ("export", 64), ("LR", 32)] and events[-2][:2] == ("export", 1)
    assert events[0][2:] == tuple(D.dlogs_to_le64(m.round_LR()))
    assert events[1][2:] == (b"".join(D.dlogs_to_le64(m.sg)), b"".join(D.dlogs_to_le64(m.sh)), D.pack_scalars(a), D.pack_scalars(b))
    assert events[1][2][:64] == bytes(64) and events[1][3][64:128] == bytes(64)        # g[0] and h[1] are identities
    for x in xs:
        m.fold(x, pow(x, -1, Q))
    assert events[-1] == ("finish",) + m.finish()
    assert len([e for e in events if e[0] == "LR"]) == 6 and len([e for e in events if e[0] == "export"]) == 7


# ---- every scenario shows its edge ----------------------------------------------------------------------------------------------
SIZES = [64, 512, 1024, 4096]          # the lengths the GPU paths use (16 384 behaves as 4 096: the same constructions)


def run(name, n):
    """(case, per round: (L, R, sg', sh') after that round's fold)"""
    case = D.scenario(name, n)
    sg, sh, su, a, b, xs, _ = case
    m = D.DlogIpa(sg, sh, su, a, b)
    rounds = []
    for x in xs:
        L, R = m.round_LR()
        m.fold(x, pow(x, -1, Q))
        rounds.append((L, R, list(m.sg), list(m.sh)))
    return case, rounds


def stride_classes(v, m):
    return [[v[i + t * m] for t in range(len(v) // m)] for i in range(m)]


@pytest.mark.parametrize("n", SIZES)
def test_edge_control_has_none(n):
    """The control: no generator under one output of a 16-way (or pairwise) fold equals or negates another, nothing is the identity."""
    (sg, sh, su, a, b, xs, _), rounds = run("control", n)
    for v in (sg, sh):
        for m in (n // 2, n // 16):
            for cls in stride_classes(v, m):
                assert len({min(k, Q - k) for k in cls}) == len(cls) and 0 not in cls
    assert all(L and R and all(s2) and all(s3) for L, R, s2, s3 in rounds)
    cg, ch = D.coefficients(xs[:4])
    assert len(set(cg)) == 16 and all(abs(h) > 1 << 100 for c in cg + ch for h in D.glv_split(c))


@pytest.mark.parametrize("name,x", [("all_equal_ones", 1), ("all_equal_minus", Q - 1)])
@pytest.mark.parametrize("n", SIZES)
def test_edge_all_equal(name, x, n):
    (sg, sh, su, a, b, xs, _), rounds = run(name, n)
    s = sg[0]
    assert set(sg) == set(sh) == {s} and s and set(xs) == {x}
    # every coefficient of every depth is +-1: one GLV half is zero, the other +-1, and the 16 points under one output are ONE point
    for d in range(1, 7):
        cg, ch = D.coefficients(xs[:d])
        assert set(cg) == set(ch) == {pow(x, d, Q)} and D.glv_split(cg[0]) in ((1, 0), (-1, 0))
    assert set(D.coefficients(xs[:4])[0]) == {1}          # the 16-way folds: P + P at the second addition
    # every folded generator is the known multiple (2 x)^r s
    for r, (_, _, s2, s3) in enumerate(rounds):
        assert set(s2) == set(s3) == {pow(2 * x, r + 1, Q) * s % Q}


@pytest.mark.parametrize("n", SIZES)
def test_edge_halves_equal_iota(n):
    (sg, sh, su, a, b, xs, _), rounds = run("halves_equal_iota", n)
    assert set(xs) == {IOTA}
    for v in (sg, sh):
        assert all(v) and all(len(set(cls)) == 1 for cls in stride_classes(v, n // 16))
    cg, ch = D.coefficients(xs[:4])
    assert set(cg) == set(ch) == {1, Q - 1} and cg[0] != cg[1]          # P + P and P - P inside one ladder
    assert sorted(D.glv_split(c) for c in set(cg)) == [(-1, 0), (1, 0)]
    assert sum(cg) % Q == 0 and sum(ch) % Q == 0
    for _, _, s2, s3 in rounds:                               # identities from the FIRST fold on
        assert not any(s2) and not any(s3)
    assert rounds[0][0] and rounds[0][1] and rounds[1][0] and rounds[1][1]        # L, R are not: c_L u, c_R u remain


@pytest.mark.parametrize("n", SIZES)
def test_edge_halves_opposite_ones(n):
    (sg, sh, su, a, b, xs, _), rounds = run("halves_opposite_ones", n)
    assert xs[0] == 1 and 1 not in xs[1:] and all(sg) and all(sh)
    assert all((sg[i] + sg[i + n // 2]) % Q == 0 and (sh[i] + sh[i + n // 2]) % Q == 0 for i in range(n // 2))
    assert all(len(set(cls)) == 16 for cls in stride_classes(sg, n // 16))       # not equal points: opposite ones only
    for _, _, s2, s3 in rounds:
        assert not any(s2) and not any(s3)


@pytest.mark.parametrize("n", SIZES)
def test_edge_lambda(n):
    (sg, sh, su, a, b, xs, _), rounds = run("lambda", n)
    assert xs[:3] == [LAMBDA, LAMBDA * LAMBDA % Q, Q - LAMBDA]
    halves = set()
    for d in range(1, 7):
        for c in set(D.coefficients(xs[:d])[0]) | set(D.coefficients(xs[:d])[1]):
            k1, k2 = D.glv_split(c)
            assert abs(k1) <= 1 and abs(k2) <= 1
            halves.add((k1, k2))
    assert {(0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (-1, -1)} <= halves
    cg, _ = D.coefficients(xs[:4])
    assert any(0 in D.glv_split(c) for c in cg) and len(set(cg)) < 16
    assert all(all(s2) and all(s3) for _, _, s2, s3 in rounds[:4])               # distinct generators: nothing cancels


@pytest.mark.parametrize("n", SIZES)
def test_edge_undo(n):
    (sg, sh, su, a, b, xs, _), rounds = run("undo", n)
    assert all(xs[r] * xs[r + 1] % Q == 1 for r in range(len(xs) - 1)) and xs[0] == xs[2]
    cg, ch = D.coefficients(xs[:4])
    x = xs[0]
    assert set(cg) == set(ch) == {pow(x, e, Q) for e in (-4, -2, 0, 2, 4)}       # 16 coefficients, 5 values
    assert cg.count(1) == 6 and ch.count(1) == 6
    assert D.coefficients(xs[:2])[0].count(1) == 2


@pytest.mark.parametrize("n", SIZES)
def test_edge_identities(n):
    (sg, sh, su, a, b, xs, _), rounds = run("identities", n)
    pos = D.identity_positions(n)
    assert {i for i in range(n) if sg[i] == 0} == pos and {i for i in range(n) if sh[i] == 0} == {(i + 1) % n for i in pos}
    assert {0, n - 1} <= pos
    run_len = min(64, n // 4)
    assert any(all(i in pos for i in range(s, s + run_len)) for s in range(0, n, run_len))     # a whole aligned run (a wave at n >= 256)
    zero_out = [i for i, cls in enumerate(stride_classes(sg, n // 16)) if not any(cls)]
    assert zero_out                                            # one output of the 16-way fold adds up 16 identities ...
    mixed = [cls for cls in stride_classes(sg, n // 16) if any(cls) and not all(cls)]
    assert mixed                                               # ... others some
    assert xs[:5] == [2, (Q + 1) // 2, 1 << 128, D.A1, Q - D.MB1] and xs[0] * xs[1] % Q == 1
    assert D.glv_split(1 << 128)[0] and D.glv_split(D.A1)[0] and D.glv_split(Q - D.MB1)[0]
    # the folded generators of that output stay the identity down to the 16-way fold, in g and (one further) in h
    s2, s3 = rounds[3][2], rounds[3][3]
    assert all(s2[i] == 0 for i in zero_out) and all(s3[(i + 1) % (n // 16)] == 0 for i in zero_out) and any(s2) and any(s3)


@pytest.mark.parametrize("n", SIZES)
def test_edge_small_multiples(n):
    (sg, sh, su, a, b, xs, _), rounds = run("small_multiples", n)
    assert xs[:4] == [3, 5, 7, 1]
    small = set(D.SMALL)
    for v in (sg, sh):
        for cls in stride_classes(v, n // 16):
            assert set(cls) == small                           # all of +-1 .. +-8 under every output
            # a table entry d P of one base is another base, for every odd digit of the width-4 ladders
            assert all(any(d * k % Q in small for k in cls if k != d * k % Q) for d in (3, 5, 7))
    cg, ch = D.coefficients(xs[:4])
    assert 105 in cg and pow(105, -1, Q) in cg and 105 in ch


@pytest.mark.parametrize("n", SIZES)
def test_edge_zero_vectors(n):
    (sg, sh, su, a, b, xs, _), rounds = run("zero_vectors", n)
    half = n // 2
    assert a[0] == Q - 1 and not any(a[1:half]) and all(a[half:])
    assert not any(b[half: half + n // 4]) and all(b[:half]) and all(b[half + n // 4:])
    assert rounds[0][0] == 0 and rounds[0][1] != 0            # the first L is the identity, R is not
    assert all(L and R for L, R, _, _ in rounds[1:])
