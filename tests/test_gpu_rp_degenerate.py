"""Range proofs over DEGENERATE generators against integers.

Every generator is a known multiple of G (tests/rp_dlog_ref.py), so every point of a proof -- V, A, S, T1, T2, u_new, P_new, every L
and R -- is a Python integer times G: identity, equal and opposite generators.  That drives the batched prover
(csrc/rp_prove_kernels.hpp) through what hash-derived generators never reach -- acc == addend and acc == -addend inside
k_pv_commit_A's lanes and at its butterfly, a lane that returns to the identity and goes on, identity rows in the fixed-base tables
(k_pv_table_level, k_pv_window_scalars, k_pv_msm), the identity as a transcript item ("AA==", put_point), as a wire point
(33 zero bytes, a zero y in format 3: k_pv_emit) and as u_new -- and the verifiers' preparation (k_rp_roles, k_rp_elements,
k_rp_expand_v2, csrc/rp_batch_host.hpp) through VALID proofs with identity points.  test_rp_dlog_ref_cpu.py pins the model to the
oracle and proves that each scenario shows its edge; here everything the engine returns must equal the model's bytes exactly.

GRID says which (scenario, bits per value, values per proof) run.  The shapes are the smallest at which each path exists: (2, 1) one
round; (8, 1) 9-term jobs, every term a remainder term of k_pv_msm<4>; (32, 1) two positions per lane of k_pv_commit_A; (64, 1)
cancel, then continue; (4, 2), (8, 4) aggregated with 8 and 32 elements; (64, 4) 256 elements, a wave per job; (64, 8) 512
elements, the NT = 512 kernels.  Provers are created under prover_table_bits = 6; one case runs at 13 bits and one at the default 16."""
import functools
import random

import pytest

import rp_dlog_ref as M
from rp_dlog_ref import Q

pytestmark = pytest.mark.gpu

GRID = {
    "control": [(2, 1), (8, 1), (32, 1), (64, 1), (4, 2), (8, 4), (64, 4), (64, 8)],
    "opposite_all_equal": [(8, 1), (32, 1), (64, 1), (8, 4), (64, 4)],
    "equal_cancel": [(2, 1), (8, 1), (64, 1), (4, 2), (8, 4), (64, 8)],
    "vector_identities": [(2, 1), (8, 1), (32, 1), (4, 2), (64, 4)],
    "vector_identities_u": [(8, 1), (64, 1), (8, 4), (64, 8)],
    "blinding_identities": [(2, 1), (32, 1), (4, 2), (64, 4)],
    "all_identity": [(2, 1), (8, 1), (64, 1), (4, 2), (8, 4), (64, 8)],
    "some_identities": [(2, 1), (8, 1), (32, 1), (64, 1), (8, 4), (64, 4)],
    "g_is_h": [(8, 1), (4, 2)],
    "u_is_g": [(8, 1), (8, 4)],
    "u_is_minus_h": [(32, 1), (4, 2)],
    "rho_twin": [(4, 2), (8, 4), (64, 4), (64, 8)],
}
# the cases that build their tables with other windows than 6 bits: 13 (straddling words) and 0 = the default, 16 for these sizes
TABLE_BITS = {("control", 8, 1): 13, ("some_identities", 2, 1): 0}
# rows of the wide cases (the proof count is cut, not the scenario): 256 elements 4 proofs, 512 elements 2 -- the rows that cancel
WIDE_KINDS = {256: ("zeros", "0101", "lanes-+", "over"), 512: ("1010", "lanes+-")}


def _grid():
    cases = [(name, nb, m) for name, shapes in GRID.items() for nb, m in shapes]
    assert {name for name, _, _ in cases} == set(M.SCENARIOS) and {(nb, m) for _, nb, m in cases} == set(M.SHAPES)
    assert len(set(cases)) == len(cases) and all(m > 1 for name, _, m in cases if name == "rho_twin")
    assert set(TABLE_BITS) <= set(cases) and sorted(TABLE_BITS.values()) == [0, 13]
    return cases


CASES = _grid()


@pytest.fixture(scope="module")
def gp():
    import gpu_common
    return gpu_common


@functools.lru_cache(maxsize=None)
def model(name, nb, m):
    """The model's case and everything the tests compare with, computed once and never changed: rows (the wide shapes' cut), the
    generators as the product's Points, per row the wire bytes in the three formats and the commitments as 64-byte points."""
    from bulletproofs_amd.ec import Point
    from bulletproofs_amd.rangeproofs.codec import proof_to_bytes
    c = M.case(name, nb, m)
    rows = [row for row in c.rows if c.n < 256 or row.kind in WIDE_KINDS[c.n]]
    pt = lambda k: Point.from_le64(M.le64([k])[0])
    gens = (pt(c.gens.sg), pt(c.gens.sh), [pt(k) for k in c.gens.sgs], [pt(k) for k in c.gens.shs], pt(c.gens.su))
    wire = {v: [proof_to_bytes(row.product, version=v) for row in rows] for v in (1, 2, 3)}
    Vs = [b"".join(M.le64(row.dlogs["V"])) for row in rows]
    return c, rows, gens, wire, Vs


def _prover(gp, name, nb, m, **kw):
    from bulletproofs_amd.rangeproofs import BatchRangeProver
    g, h, gs, hs, u = model(name, nb, m)[2]
    eng = gp.engine()
    try:
        eng.set_option("prover_table_bits", TABLE_BITS.get((name, nb, m), 6))
        return BatchRangeProver(nb, g, h, gs, hs, u, m=m, **kw)
    finally:
        eng.set_option("prover_table_bits", 0)


def _inputs(rows, m):
    from bulletproofs_amd.utils import ModP
    vs = [[ModP(v, Q) for v in row.vs] for row in rows]
    gammas = [[ModP(x, Q) for x in row.gammas] for row in rows]
    if m == 1:
        vs, gammas = [r[0] for r in vs], [r[0] for r in gammas]
    return vs, gammas, [row.seed for row in rows]


def _first_difference(got, want, rows):
    for i, (a, b) in enumerate(zip(got, want)):
        if a != b:
            at = next((j for j in range(min(len(a), len(b))) if a[j] != b[j]), min(len(a), len(b)))
            return "proof %d (row %s): %d / %d bytes, first difference at byte %d" % (i, rows[i].kind, len(a), len(b), at)
    return None if len(got) == len(want) else "%d proofs for %d" % (len(got), len(want))


@pytest.mark.parametrize("name,nb,m", CASES)
def test_batch_prover_writes_the_model_bytes(gp, name, nb, m):
    """BatchRangeProver.prove_wire == proof_to_bytes(model) in wire formats 2 and 3, a second, shorter batch on the same prover is
    the prefix, and commit_packed gives the model's V."""
    c, rows, gens, wire, Vs = model(name, nb, m)
    vs, gammas, seeds = _inputs(rows, m)
    bp = _prover(gp, name, nb, m)
    try:
        v2 = bp.prove_wire(vs, gammas, seeds)
        short = max(1, len(rows) // 2)
        again = bp.prove_wire(vs[:short], gammas[:short], seeds[:short])
        commits = bp.commit_packed(vs, gammas)
        bp.wire_format = 3
        v3 = bp.prove_wire(vs, gammas, seeds)
    finally:
        bp.close()
    assert _first_difference(v2, wire[2], rows) is None
    assert again == v2[:short]
    assert _first_difference(v3, wire[3], rows) is None
    assert [commits[64 * m * i: 64 * m * (i + 1)] for i in range(len(rows))] == Vs


def _golden_form(pr):
    """the model's proof in the layout of tests/golden/rangeproofs.json, which check_range_proof reads"""
    from helpers import hx
    xy = lambda P: [hx(P.x), hx(P.y)]
    ip, p2 = pr.innerProof, pr.innerProof.proof2
    proof2 = dict(a=hx(p2.a.x), b=hx(p2.b.x), xs=[hx(x.x) for x in p2.xs], Ls=[xy(P) for P in p2.Ls], Rs=[xy(P) for P in p2.Rs],
                  transcript=p2.transcript.decode(), start_transcript=p2.start_transcript)
    inner = dict(u_new=xy(ip.u_new), P_new=xy(ip.P_new), transcript=ip.transcript.decode(), proof2=proof2)
    return dict(taux=hx(pr.taux.x % Q), mu=hx(pr.mu.x % Q), t_hat=hx(pr.t_hat.x % Q), T1=xy(pr.T1), T2=xy(pr.T2), A=xy(pr.A), S=xy(pr.S),
                transcript=pr.transcript.decode(), inner=inner)


@pytest.mark.parametrize("name,nb,m", CASES)
def test_single_proof_provers_and_verifiers(gp, name, nb, m):
    """NIRangeProver / AggregNIRangeProver on the same inputs give the model's fields (check_range_proof's list); RangeVerifier /
    AggregRangeVerifier accept the proof of every in-range row, and raise "Proof invalid" with V + G."""
    from bulletproofs_amd.ec import Point, secp256k1
    from bulletproofs_amd.rangeproofs import AggregNIRangeProver, AggregRangeVerifier, NIRangeProver, RangeVerifier
    from test_gpu_rangeproofs import check_range_proof
    c, rows, (g, h, gs, hs, u), wire, Vs = model(name, nb, m)
    vs, gammas, seeds = _inputs(rows, m)
    for r, row in enumerate(rows):
        if m == 1:
            pr = NIRangeProver(vs[r], nb, g, h, gs, hs, gammas[r], u, secp256k1, seeds[r]).prove()
        else:
            pr = AggregNIRangeProver(vs[r], nb, g, h, gs, hs, gammas[r], u, secp256k1, seeds[r]).prove()
        check_range_proof(gp, pr, _golden_form(row.proof))
        if not row.valid:
            continue
        V = [Point.from_le64(Vs[r][64 * j: 64 * j + 64]) for j in range(m)]
        moved = [Point.from_le64(b) for b in M.le64([k + (1 if j == r % m else 0) for j, k in enumerate(row.dlogs["V"])])]
        if m == 1:
            assert RangeVerifier(V[0], g, h, gs, hs, u, pr).verify() is True, row.kind
            if r < 3:
                with pytest.raises(Exception, match="Proof invalid"):
                    RangeVerifier(moved[0], g, h, gs, hs, u, pr).verify()
        else:
            assert AggregRangeVerifier(V, g, h, gs, hs, u, pr).verify() is True, row.kind
            if r < 3:
                with pytest.raises(Exception, match="Proof invalid"):
                    AggregRangeVerifier(moved, g, h, gs, hs, u, pr).verify()


@pytest.mark.parametrize("name,nb,m", CASES)
def test_batch_verifier_accepts_the_model_proofs(gp, name, nb, m):
    """The in-range rows as one batch: verify_wire is True in wire formats 1, 2 and 3, partial_wire under explicit weights is the
    identity, and the device preparation equals the host twin byte for byte (scalars, shared coefficients, decoded points)."""
    from bulletproofs_amd.rangeproofs import BatchRangeVerifier
    from test_gpu_batch_dev import assert_same
    c, rows, (g, h, gs, hs, u), wire, Vs = model(name, nb, m)
    keep = [r for r, row in enumerate(rows) if row.valid]
    packed = b"".join(Vs[r] for r in keep)
    rnd = random.Random("rp-degenerate-weights/%s/%d/%d" % (name, nb, m))
    weights = [rnd.randrange(1, Q) for _ in range(4 * len(keep))]
    bv = BatchRangeVerifier(g, h, gs, hs, u)
    try:
        for v in (1, 2, 3):
            blobs = [wire[v][r] for r in keep]
            assert bv.verify_wire(packed, blobs) is True, v
            it = iter(weights)
            fixed = BatchRangeVerifier(g, h, gs, hs, u, rng=lambda: next(it))
            try:
                assert fixed.partial_wire(packed, blobs) == bytes(64), v
            finally:
                fixed.release()
            assert_same(gp.engine(), c.n, m, blobs, b"".join(w.to_bytes(32, "little") for w in weights), None)
    finally:
        bv.release()


@pytest.mark.parametrize("name,nb,m", CASES)
def test_batch_verifier_names_the_one_wrong_commitment(gp, name, nb, m):
    """One commitment of one proof moved by G: the batch fails and locate_wire names exactly that proof."""
    from bulletproofs_amd.rangeproofs import BatchRangeVerifier
    c, rows, (g, h, gs, hs, u), wire, Vs = model(name, nb, m)
    keep = [r for r, row in enumerate(rows) if row.valid]
    bad = len(keep) // 2
    row = rows[keep[bad]]
    slot = bad % m
    moved = b"".join(M.le64([k + (1 if j == slot else 0) for j, k in enumerate(row.dlogs["V"])]))
    packed = b"".join(moved if i == bad else Vs[r] for i, r in enumerate(keep))
    bv = BatchRangeVerifier(g, h, gs, hs, u)
    try:
        for v in (2, 3):
            blobs = [wire[v][r] for r in keep]
            with pytest.raises(Exception, match="^Proof invalid$"):
                bv.verify_wire(packed, blobs)
            assert bv.locate_wire(packed, blobs) == [bad], v
    finally:
        bv.release()
