"""Integer model of the single and aggregated range provers over generators with KNOWN discrete logarithms (test helper: plain
Python, no GPU).

Every generator is a known multiple of the base point G: g = sg G, h = sh G, u = su G, gs[i] = sgs[i] G, hs[i] = shs[i] G; a dlog
of 0 is the identity.  Everything the provers emit (src/rangeproofs/rangeproof_prover.py:35-112,
src/rangeproofs/rangeproof_aggreg_prover.py:36-146 and the NIProver / FastNIProver2 nested in them,
src/innerproduct/inner_product_prover.py:11-110) is then an integer mod q times G: V, A, S, T1, T2, u_new, P_new and every L_j, R_j.

BUILD CHOSEN: the `Point` subclass.  `DlogPoint` is an oracle.ec.Point that carries its dlog and is fed to
oracle.bp_ref.range_prove_generic through its `multiexp` hook (`dlog_multiexp`: sum e_i k_i mod q).  Its +, -, unary - and int *
work on the dlog alone, so Zq.__mul__ -- which tests isinstance(o, Point) and then evaluates int * o -- lands in DlogPoint.__mul__.
The scalar algebra, the transcripts and mod_hash are therefore the oracle's own lines, not a second restatement.  No MSM and no
group-law code takes part: a DlogPoint becomes a real point only when somebody reads its x or y -- the transcript (A and S before
y, T1 and T2 before x, L_j and R_j before x_j), and the caller for the emitted points -- and that is a batched k G over the distinct
values not seen yet (ipa_dlog_ref.dlogs_to_le64).  Folded generators, hs' = y^-i hs_i and every partial sum stay integers.

`prove(...)` returns the oracle's proof object (points are DlogPoints) and the dlogs of every emitted point; `product_proof` turns
it into the object rangeproofs.codec.proof_to_bytes(..., version=1|2|3) takes.

The named scenarios choose generators so that the batched prover's kernels (csrc/rp_prove_kernels.hpp) and the verifier's
preparation meet the identity, their own accumulator and its negative; test_rp_dlog_ref_cpu.py shows from the model alone that each
scenario reaches the edge it is there for, test_gpu_rp_degenerate.py compares the engine with the model's bytes."""
import functools
import random
from types import SimpleNamespace

from ipa_dlog_ref import Q, dlogs_to_le64
from oracle import bp_ref as R
from oracle.ec import Point, point_from_le64, secp256k1

assert Q == secp256k1.q

# ---- points that are their dlog ----------------------------------------------------------------------------------------------------
_XY = {0: (0, 0)}


def materialise(ks):
    """Make k G known for every k of `ks`: ONE batched multiplication of G over the distinct values not computed before."""
    todo = sorted({k % Q for k in ks} - _XY.keys())
    if todo:
        for k, raw in zip(todo, dlogs_to_le64(todo)):
            _XY[k] = (int.from_bytes(raw[:32], "little"), int.from_bytes(raw[32:], "little"))


def _xy(k):
    if k not in _XY:
        materialise([k])
    return _XY[k]


class DlogPoint(Point):
    """k G known by k.  x and y are computed when read; the group law is integer arithmetic mod q."""
    __slots__ = ("k",)

    def __init__(self, k):
        self.k = int(k) % Q

    x = property(lambda self: _xy(self.k)[0])
    y = property(lambda self: _xy(self.k)[1])
    curve = property(lambda self: secp256k1 if self.k else None)

    def __eq__(self, other):
        if isinstance(other, DlogPoint):
            return self.k == other.k
        return isinstance(other, Point) and (other.curve is None) == (self.k == 0) and (self.x, self.y) == (other.x, other.y)

    def __hash__(self):
        return hash(self.k)

    def __neg__(self):
        return DlogPoint(-self.k)

    def __add__(self, other):
        assert isinstance(other, DlogPoint)
        return DlogPoint(self.k + other.k)

    def __sub__(self, other):
        assert isinstance(other, DlogPoint)
        return DlogPoint(self.k - other.k)

    def __mul__(self, e):
        return DlogPoint(int(e) * self.k)

    __rmul__ = __mul__

    def __repr__(self):
        return "DlogPoint(%x)" % self.k


def dlog_multiexp(gs, es):
    """The `multiexp` hook: sum e_i gs_i on dlogs (what src/pippenger/pippenger.py:22-61 computes, without a group operation)."""
    if len(gs) != len(es):
        raise Exception("Different number of group elements and exponents")
    return DlogPoint(sum(int(e % Q) * g.k for g, e in zip(gs, es)))


def le64(ks):
    """[k] -> [64-byte wire point of k G]"""
    materialise(ks)
    return [_XY[k % Q][0].to_bytes(32, "little") + _XY[k % Q][1].to_bytes(32, "little") for k in ks]


def real_points(ks):
    """[k] -> [plain oracle Point k G] (for the oracle's own provers and verifiers, which then use their own group law)"""
    return [point_from_le64(b) for b in le64(ks)]


# ---- scenarios ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(2, 1), (8, 1), (32, 1), (64, 1), (4, 2), (8, 4), (64, 4), (64, 8)]


def _base(name, nb, m):
    n = nb * m
    rnd = random.Random("rp-dlog/%s/%d/%d" % (name, nb, m))
    sg, sh, su = (rnd.randrange(1, Q) for _ in range(3))
    sgs = [rnd.randrange(1, Q) for _ in range(n)]
    shs = [rnd.randrange(1, Q) for _ in range(n)]
    c = rnd.randrange(1, Q)
    return rnd, n, sg, sh, su, sgs, shs, c


def _gens(sg, sh, su, sgs, shs):
    return SimpleNamespace(sg=sg % Q, sh=sh % Q, su=su % Q, sgs=[v % Q for v in sgs], shs=[v % Q for v in shs])


def sc_control(nb, m):
    _, n, sg, sh, su, sgs, shs, c = _base("control", nb, m)
    return _gens(sg, sh, su, sgs, shs)


def sc_opposite_all_equal(nb, m):
    """gs_i = c G, hs_i = -c G: bit_i gs_i - (1 - bit_i) hs_i = c G whatever the bit, A = n c G + alpha h.  h is the identity here, so
    that alpha's windows add nothing in k_pv_commit_A: every live lane then ends with the same sum (n / 16 c, or c below 16 lanes),
    and every level of the butterfly adds a point to itself; from n = 32 a lane adds c G to c G inside the mixed addition."""
    _, n, sg, sh, su, sgs, shs, c = _base("opposite_all_equal", nb, m)
    return _gens(sg, 0, su, [c] * n, [Q - c] * n)


def sc_equal_cancel(nb, m):
    """gs_i = hs_i = c G, h the identity: a set bit adds c G, a clear bit takes it away.  A is (2 popcount - n) c G: the identity for
    popcount = n / 2.  The rows `lanes+-` / `lanes-+` alternate the sign inside every lane (positions i and i + 16), so a lane's
    accumulator returns to the identity and goes on (n = 64: twice); `0101` / `1010` give opposite lanes, cancelled by the butterfly."""
    _, n, sg, sh, su, sgs, shs, c = _base("equal_cancel", nb, m)
    return _gens(sg, 0, su, [c] * n, [c] * n)


def sc_vector_identities(nb, m):
    """gs = hs = u = identity: A = alpha h, S = rho h; u_new, P_new and every L, R are the identity; T1, T2 and V are finite."""
    _, n, sg, sh, su, sgs, shs, c = _base("vector_identities", nb, m)
    return _gens(sg, sh, 0, [0] * n, [0] * n)


def sc_vector_identities_u(nb, m):
    """gs = hs = identity, u finite: L_j = c_L u_new, R_j = c_R u_new, P_new = x_ip t_hat u: every lane of a job but the u term's idles."""
    _, n, sg, sh, su, sgs, shs, c = _base("vector_identities_u", nb, m)
    return _gens(sg, sh, su, [0] * n, [0] * n)


def sc_blinding_identities(nb, m):
    """g = h = identity: T1 = T2 = V = identity, A and S carry their vector part alone."""
    _, n, sg, sh, su, sgs, shs, c = _base("blinding_identities", nb, m)
    return _gens(0, 0, su, sgs, shs)


def sc_all_identity(nb, m):
    """Every generator is the identity: so is every point of every proof, every transcript item of a point is "AA==", and the proof
    verifies (0 = 0)."""
    _, n, *_ = _base("all_identity", nb, m)
    return _gens(0, 0, 0, [0] * n, [0] * n)


def some_identities_plan(n):
    """-> (zero positions of gs, zero positions of hs, (i, j): gs_i = gs_j, i: hs_i = -gs_i) -- the IPA tests' "collide"."""
    zg = {0, n - 1} if n > 2 else {0}
    zh = {1 % n, n // 2} if n > 2 else {1}
    free = [i for i in range(n) if i not in zg]
    pair = (free[0], free[-1]) if len(free) >= 2 and free[0] != free[-1] else None
    opp = [i for i in range(n) if i not in zg and i not in zh]
    return zg, zh, pair, (opp[len(opp) // 2] if opp else None)


def sc_some_identities(nb, m):
    _, n, sg, sh, su, sgs, shs, c = _base("some_identities", nb, m)
    zg, zh, pair, opp = some_identities_plan(n)
    if pair:
        sgs[pair[1]] = sgs[pair[0]]
    if opp is not None:
        shs[opp] = Q - sgs[opp]
    for i in zg:
        sgs[i] = 0
    for i in zh:
        shs[i] = 0
    return _gens(sg, sh, su, sgs, shs)


def sc_g_is_h(nb, m):
    """g = h: V = (v + gamma) g, the identity for the row `v_cancel` (v = 5, gamma = q - 5) by cancellation in the two lanes' butterfly."""
    _, n, sg, sh, su, sgs, shs, c = _base("g_is_h", nb, m)
    return _gens(sg, sg, su, sgs, shs)


def sc_u_is_g(nb, m):
    _, n, sg, sh, su, sgs, shs, c = _base("u_is_g", nb, m)
    return _gens(sg, sh, sg, sgs, shs)


def sc_u_is_minus_h(nb, m):
    _, n, sg, sh, su, sgs, shs, c = _base("u_is_minus_h", nb, m)
    return _gens(sg, sh, Q - sh, sgs, shs)


def rho_twin_index(nb, m):
    """The base that S's scalar s_(2 nb) multiplies: rho = mod_hash(str(2 nb) ...) (rangeproof_aggreg_prover.py:61) equals s_(2 nb),
    which is sL[2 nb] over gs[2 nb] when 2 nb < n, else sR[2 nb - n] over hs[2 nb - n]."""
    n = nb * m
    return ("gs", 2 * nb) if 2 * nb < n else ("hs", 2 * nb - n)


def sc_rho_twin(nb, m):
    """Aggregated only: h is the very base s_(2 nb) multiplies, so the terms rho h and s_(2 nb) base of S are the same point with the
    same scalar."""
    assert m > 1
    _, n, sg, sh, su, sgs, shs, c = _base("rho_twin", nb, m)
    side, i = rho_twin_index(nb, m)
    return _gens(sg, sgs[i] if side == "gs" else shs[i], su, sgs, shs)


SCENARIOS = {
    "control": sc_control,
    "opposite_all_equal": sc_opposite_all_equal,
    "equal_cancel": sc_equal_cancel,
    "vector_identities": sc_vector_identities,
    "vector_identities_u": sc_vector_identities_u,
    "blinding_identities": sc_blinding_identities,
    "all_identity": sc_all_identity,
    "some_identities": sc_some_identities,
    "g_is_h": sc_g_is_h,
    "u_is_g": sc_u_is_g,
    "u_is_minus_h": sc_u_is_minus_h,
    "rho_twin": sc_rho_twin,
}

# ---- values, blinding factors, seeds -------------------------------------------------------------------------------------------------
KINDS = ("zeros", "ones", "0101", "1010", "random", "over")
GAMMAS = ("zero", "one", "minus_one", "random")
SEED_LENGTHS = (0, 1, 2, 3, 17, 200)


def row_kinds(name, nb, m):
    """The rows of a case, in order: the six of KINDS; from n = 32 the two lane-alternating bit patterns; for g_is_h the cancelling pair."""
    kinds = list(KINDS)
    if nb * m >= 32:
        kinds += ["lanes+-", "lanes-+"]
    if name == "g_is_h":
        kinds.append("v_cancel")
    return kinds


def _from_bits(bits, nb, m):
    """element i of a proof's bit vector is bit i % nb of value i / nb (rangeproof_aggreg_prover.py:44-49)"""
    return [sum(bits[j * nb + t] << t for t in range(nb)) for j in range(m)]


def make_rows(name, nb, m, count=None):
    """-> [SimpleNamespace(kind, vs, gammas, seed, valid)]: `count` rows (default: all of row_kinds), values and blinding factors as
    ints.  Row r, slot j takes the blinding factor GAMMAS[(r + j) % 4]; row r's seed has SEED_LENGTHS[r % 6] bytes."""
    rnd = random.Random("rp-dlog-rows/%s/%d/%d" % (name, nb, m))
    n, top = nb * m, (1 << nb) - 1
    alt = sum(1 << t for t in range(0, nb, 2))            # ...0101
    rows = []
    for r, kind in enumerate(row_kinds(name, nb, m)):
        rand = [rnd.randrange(1 << nb) for _ in range(m)]
        if kind == "zeros":
            vs = [0] * m
        elif kind == "ones":
            vs = [top] * m
        elif kind == "0101":
            vs = [alt if j % 2 == 0 else top ^ alt for j in range(m)]
        elif kind == "1010":
            vs = [top ^ alt if j % 2 == 0 else alt for j in range(m)]
        elif kind == "random":
            vs = rand
        elif kind == "over":
            vs = rand[:-1] + [(1 << nb) + rnd.randrange(1 << nb)]          # only its low nb bits are proved (rangeproof_prover.py:40)
        elif kind in ("lanes+-", "lanes-+"):
            first = 1 if kind == "lanes+-" else 0
            vs = _from_bits([first ^ (i // 16 & 1) for i in range(n)], nb, m)
        else:
            assert kind == "v_cancel"
            vs = [5 if nb >= 3 else 1] * m
        gammas = []
        for j in range(m):
            gk = GAMMAS[(r + j) % 4]
            gammas.append({"zero": 0, "one": 1, "minus_one": Q - 1}.get(gk, rnd.randrange(2, Q - 1)))
        if kind == "v_cancel":
            gammas = [Q - v for v in vs]
        seed = rnd.randbytes(SEED_LENGTHS[r % 6])
        rows.append(SimpleNamespace(kind=kind, vs=vs, gammas=gammas, seed=seed, valid=kind != "over"))
    return rows if count is None else rows[:count]


# ---- the prover ---------------------------------------------------------------------------------------------------------------------
def dlog_generators(gens):
    return (DlogPoint(gens.sg), DlogPoint(gens.sh), [DlogPoint(k) for k in gens.sgs], [DlogPoint(k) for k in gens.shs], DlogPoint(gens.su))


def prove(gens, nb, vs, gammas, seed):
    """One proof of the values `vs` (m = len(vs) values of nb bits) with blinding factors `gammas` -> (proof, dlogs).  m = 1 takes the
    single-value prover's form (a scalar gamma), m > 1 the aggregated one.  proof: the oracle's RangeProof, points as DlogPoints;
    dlogs: {"V": [..], "A", "S", "T1", "T2", "u_new", "P_new", "Ls": [..], "Rs": [..]}."""
    g, h, gs, hs, u = dlog_generators(gens)
    m = len(vs)
    zv, zg = [R.Zq(v, Q) for v in vs], [R.Zq(x, Q) for x in gammas]
    Vs = [R.commitment(g, h, v, x) for v, x in zip(zv, zg)]           # src/utils/commitments.py:5-6
    pr = R.range_prove_generic(zv, nb, g, h, gs, hs, zg[0] if m == 1 else zg, u, Q, seed, dlog_multiexp)
    ip, p2 = pr.innerProof, pr.innerProof.proof2
    dlogs = dict(V=[V.k for V in Vs], A=pr.A.k, S=pr.S.k, T1=pr.T1.k, T2=pr.T2.k, u_new=ip.u_new.k, P_new=ip.P_new.k,
                 Ls=[P.k for P in p2.Ls], Rs=[P.k for P in p2.Rs])
    return pr, dlogs


def emitted(dlogs):
    """every emitted dlog of a proof, flat: V.. A S T1 T2 u_new P_new L.. R.."""
    return dlogs["V"] + [dlogs[k] for k in ("A", "S", "T1", "T2", "u_new", "P_new")] + dlogs["Ls"] + dlogs["Rs"]


def identity_names(dlogs):
    """the names of the emitted points that are the identity: "V0", "A", "L2", ..."""
    out = {"V%d" % j for j, k in enumerate(dlogs["V"]) if k == 0}
    out |= {k for k in ("A", "S", "T1", "T2", "u_new", "P_new") if dlogs[k] == 0}
    out |= {"L%d" % j for j, k in enumerate(dlogs["Ls"]) if k == 0} | {"R%d" % j for j, k in enumerate(dlogs["Rs"]) if k == 0}
    return out


def all_names(m, k):
    return {"V%d" % j for j in range(m)} | {"A", "S", "T1", "T2", "u_new", "P_new"} | {"%s%d" % (s, j) for s in "LR" for j in range(k)}


def expected_identities(name, row, nb, m):
    """What the scenario table promises, as a set of names: the emitted points that MUST be the identity in `row` (every other
    emitted point must be finite).  A commitment v g + gamma h is the identity when each of its two terms has a zero scalar or an
    identity base (the rows draw v = 0 and gamma = 0; opposite_all_equal and equal_cancel have h = identity), or, with g = h, when
    v + gamma = 0."""
    gens = SCENARIOS[name](nb, m)
    k = (nb * m).bit_length() - 1
    lr = {"%s%d" % (s, j) for s in "LR" for j in range(k)}
    out = {"V%d" % j for j in range(m) if (row.vs[j] % Q == 0 or gens.sg == 0) and (row.gammas[j] % Q == 0 or gens.sh == 0)}
    if name == "g_is_h":
        out |= {"V%d" % j for j in range(m) if (row.vs[j] + row.gammas[j]) % Q == 0}
    if name == "all_identity":
        out |= all_names(m, k)
    elif name == "vector_identities":
        out |= lr | {"u_new", "P_new"}
    elif name == "blinding_identities":
        out |= {"T1", "T2"}
    elif name == "equal_cancel" and 2 * sum(bin(v & ((1 << nb) - 1)).count("1") for v in row.vs) == nb * m:
        assert gens.sh == 0
        out |= {"A"}                                    # popcount = n / 2 and h the identity: always so in the rows 0101, 1010, lanes+-, lanes-+
    return out


def real_proof(pr):
    """the model's proof with plain oracle Points (what R.range_verify takes)"""
    ip, p2 = pr.innerProof, pr.innerProof.proof2
    ks = [pr.T1.k, pr.T2.k, pr.A.k, pr.S.k, ip.u_new.k, ip.P_new.k] + [P.k for P in p2.Ls] + [P.k for P in p2.Rs]
    pts = real_points(ks)
    k = len(p2.Ls)
    inner = R.Proof1(pts[4], pts[5], R.Proof2(p2.a, p2.b, p2.xs, pts[6: 6 + k], pts[6 + k:], p2.transcript, p2.start_transcript), ip.transcript)
    return R.RangeProof(pr.taux, pr.mu, pr.t_hat, pts[0], pts[1], pts[2], pts[3], inner, pr.transcript)


def product_proof(pr):
    """the model's proof as the product package's objects: what rangeproofs.codec.proof_to_bytes(..., version=1|2|3) accepts"""
    from test_batch_verify_cpu import convert_proof
    return convert_proof(real_proof(pr))


@functools.lru_cache(maxsize=None)
def case(name, nb, m, count=None):
    """A whole case, computed once per process: generators, rows, and per row the model's proof and dlogs.
    -> SimpleNamespace(name, nb, m, n, gens, rows): rows[r] has .proof (DlogPoints), .dlogs, .product (codec-ready) beside make_rows' fields."""
    gens = SCENARIOS[name](nb, m)
    materialise([gens.sg, gens.sh, gens.su] + gens.sgs + gens.shs)
    rows = make_rows(name, nb, m, count)
    for row in rows:
        row.proof, row.dlogs = prove(gens, nb, row.vs, row.gammas, row.seed)
    materialise([k for row in rows for k in emitted(row.dlogs)])
    for row in rows:
        row.product = product_proof(row.proof)
    return SimpleNamespace(name=name, nb=nb, m=m, n=nb * m, gens=gens, rows=rows)


# ---- k_pv_commit_A's lane split, on dlogs --------------------------------------------------------------------------------------------
def replay_commit_A(gens, nb, vs):
    """csrc/rp_prove_kernels.hpp k_pv_commit_A as documented there, on dlogs: 16 lanes per proof; lane l walks the positions
    i = l, l + 16, ... < n and adds gs_i for a set bit, -hs_i for a clear one (identity addends are skipped, as xyzz_madd_signed
    does); then the lanes' sums meet in a butterfly over the xor distances 1, 2, 4, 8 (each lane adds its partner's sum to its own).
    alpha h's windows, which the lanes add between the two, are left out: the scenarios that use this function have h = identity,
    whose table rows are all identities and add nothing -- asserted.
    -> SimpleNamespace(result, lane_doublings, lane_cancellations, lane_identity_then_continue, level_doublings, level_cancellations):
    counts of acc == addend != 0 / acc == -addend != 0 / "acc became the identity and a later position added a finite point" inside
    the lanes, and per butterfly level how many of the 16 lanes added a finite point to itself / to its negative."""
    assert gens.sh == 0
    m = len(vs)
    n = nb * m
    bits = [(vs[i // nb] >> (i % nb)) & 1 for i in range(n)]
    acc = [0] * 16
    doubl = canc = cont = 0
    for l in range(16):
        a, was_cancelled = 0, False
        for i in range(l, n, 16):
            t = gens.sgs[i] if bits[i] else (Q - gens.shs[i]) % Q
            if t == 0:
                continue
            if a == 0 and was_cancelled:
                cont += 1
                was_cancelled = False
            if a and a == t:
                doubl += 1
            if a and (a + t) % Q == 0:
                canc += 1
                was_cancelled = True
            a = (a + t) % Q
        acc[l] = a
    lvl_d, lvl_c = [], []
    for dist in (1, 2, 4, 8):
        other = [acc[l ^ dist] for l in range(16)]
        lvl_d.append(sum(1 for a, o in zip(acc, other) if a and a == o))
        lvl_c.append(sum(1 for a, o in zip(acc, other) if a and (a + o) % Q == 0))
        acc = [(a + o) % Q for a, o in zip(acc, other)]
    assert len(set(acc)) == 1
    return SimpleNamespace(result=acc[0], lane_doublings=doubl, lane_cancellations=canc, lane_identity_then_continue=cont,
                           level_doublings=lvl_d, level_cancellations=lvl_c)
