"""The integer model of tests/rp_dlog_ref.py against the oracle's own provers and verifiers on explicit points, and -- from the model
alone -- the proof that every scenario shows the edge it is there for, so that no case of test_gpu_rp_degenerate.py can be vacuous;
then the model's wire bytes through the native host twin of the batch verifier's preparation (bpmi_rp_batch_prepare)."""
import pytest

import rp_dlog_ref as M
from rp_dlog_ref import Q
from oracle import bp_ref as R
from oracle import cbind

DEGENERATE = [name for name in M.SCENARIOS if name != "control"]
SMALL = [(2, 1), (8, 1), (4, 2)]
UP_TO_64 = [(2, 1), (8, 1), (32, 1), (64, 1), (4, 2), (8, 4)]
# (scenario, nb, m): control at every shape up to 64 elements, every degenerate scenario at the three smallest shapes
PINNED = [("control", nb, m) for nb, m in UP_TO_64] + [(name, nb, m) for name in DEGENERATE for nb, m in SMALL if not (name == "rho_twin" and m == 1)]
EVERYWHERE = [(name, nb, m) for name in M.SCENARIOS for nb, m in M.SHAPES if not (name == "rho_twin" and m == 1)]


def _generators(c):
    g, h, u = M.real_points([c.gens.sg, c.gens.sh, c.gens.su])
    return g, h, M.real_points(c.gens.sgs), M.real_points(c.gens.shs), u


def test_dlog_points_are_points_without_a_group_law():
    """DlogPoint: the group law on integers, x and y on demand, and Zq * DlogPoint lands on the dlog."""
    a, b = M.DlogPoint(5), M.DlogPoint(Q - 5)
    assert (a + b).k == 0 and (a + b).curve is None and (a + b) == R.INF and R.point_to_bytes(a + b) == b"\x00"
    assert (R.Zq(3, Q) * a).k == 15 and (7 * a).k == 35 and (a * 7).k == 35 and (-a) == b and (a - a).k == 0
    five = cbind.ec_mul_batch([M.secp256k1.G], [5])[0]
    assert (a.x, a.y) == (five.x, five.y) and a == five and not a == -five and R.point_to_bytes(a) == R.point_to_bytes(five)
    assert M.dlog_multiexp([a, b, M.DlogPoint(0)], [R.Zq(2, Q), 1, 9]).k == 5
    assert M.le64([0, 5]) == [bytes(64), cbind.pack_points([five])]


@pytest.mark.parametrize("name,nb,m", PINNED)
def test_model_equals_the_oracle_prover_field_for_field(name, nb, m):
    """R.range_prove / R.aggreg_range_prove with multiexp = cbind.msm over the REAL points k G (the oracle's own affine group law
    everywhere else; from 32 elements the C oracle's bulk form of the same element-wise expressions) give the model's proof."""
    c = M.case(name, nb, m)
    g, h, gs, hs, u = _generators(c)
    ecops = cbind.BulkEC() if c.n >= 32 else None
    for row in c.rows:
        vs, gammas = [R.Zq(v, Q) for v in row.vs], [R.Zq(x, Q) for x in row.gammas]
        if m == 1:
            want = R.range_prove(vs[0], nb, g, h, gs, hs, gammas[0], u, seed=row.seed, multiexp=cbind.msm, ecops=ecops)
        else:
            want = R.aggreg_range_prove(vs, nb, g, h, gs, hs, gammas, u, seed=row.seed, multiexp=cbind.msm, ecops=ecops)
        got = M.real_proof(row.proof)
        where = (name, nb, m, row.kind)
        assert (got.taux, got.mu, got.t_hat) == (want.taux, want.mu, want.t_hat), where
        assert (got.T1, got.T2, got.A, got.S) == (want.T1, want.T2, want.A, want.S), where
        assert got.transcript == want.transcript, where
        gi, wi = got.innerProof, want.innerProof
        assert (gi.u_new, gi.P_new, gi.transcript) == (wi.u_new, wi.P_new, wi.transcript), where
        g2, w2 = gi.proof2, wi.proof2
        assert (g2.a, g2.b, g2.xs, g2.Ls, g2.Rs) == (w2.a, w2.b, w2.xs, w2.Ls, w2.Rs), where
        assert (g2.transcript, g2.start_transcript) == (w2.transcript, w2.start_transcript), where
        assert M.real_points(row.dlogs["V"]) == [R.commitment(g, h, v, x) for v, x in zip(vs, gammas)], where


@pytest.mark.parametrize("name,nb,m", PINNED)
def test_the_oracle_verifiers_accept_the_model_proofs(name, nb, m):
    """range_verify / aggreg_range_verify (multiexp = cbind.msm) accept every in-range row and reject it with V moved by G; the
    control scenario's out-of-range row is rejected (with degenerate generators such a proof can be valid: 0 = 0)."""
    c = M.case(name, nb, m)
    g, h, gs, hs, u = _generators(c)

    def verify(Vks, pr):
        Vs = M.real_points(Vks)
        if m == 1:
            return R.range_verify(Vs[0], g, h, gs, hs, u, pr, multiexp=cbind.msm)
        return R.aggreg_range_verify(Vs, g, h, gs, hs, u, pr, multiexp=cbind.msm)

    for r, row in enumerate(c.rows):
        pr = M.real_proof(row.proof)
        if row.valid:
            assert verify(row.dlogs["V"], pr) is True, (name, nb, m, row.kind)
            if r % 3 == 1:
                moved = list(row.dlogs["V"])
                moved[r % m] += 1
                with pytest.raises(Exception, match="Proof invalid"):
                    verify(moved, pr)
        elif name == "control":
            with pytest.raises(Exception, match="Proof invalid"):
                verify(row.dlogs["V"], pr)


@pytest.mark.parametrize("name,nb,m", EVERYWHERE)
def test_every_scenario_emits_the_identities_its_table_row_states(name, nb, m):
    """Which emitted points are the identity, from the model alone, at every shape: exactly the set the scenario promises."""
    c = M.case(name, nb, m)
    k = c.n.bit_length() - 1
    for row in c.rows:
        got = M.identity_names(row.dlogs)
        assert got == M.expected_identities(name, row, nb, m), (name, nb, m, row.kind, sorted(got))
        assert len(row.dlogs["Ls"]) == len(row.dlogs["Rs"]) == k and len(row.dlogs["V"]) == m
    kinds = {row.kind: row for row in c.rows}
    if name == "all_identity":
        # the whole transcript of a point is "AA==": four items in the range-proof transcript, two per round in Protocol 2's
        for row in c.rows:
            assert row.proof.transcript.count(b"&AA==") == 4 and row.proof.innerProof.proof2.transcript.count(b"&AA==") == 2 * k
            assert M.identity_names(row.dlogs) == M.all_names(m, k)
    if name == "vector_identities":
        for row in c.rows:
            assert row.dlogs["A"] and row.dlogs["S"] and row.dlogs["T1"] and row.dlogs["T2"] and not any(row.dlogs["Ls"] + row.dlogs["Rs"])
    if name == "vector_identities_u":
        x_ip = int(c.rows[0].proof.innerProof.transcript.split(b"&")[1])
        for row in c.rows:
            assert row.dlogs["P_new"] == x_ip * row.proof.t_hat.x * c.gens.su % Q and row.dlogs["u_new"] == x_ip * c.gens.su % Q
    if name == "blinding_identities":
        assert all(row.dlogs["T1"] == row.dlogs["T2"] == 0 and not any(row.dlogs["V"]) for row in c.rows)
    if name == "equal_cancel":
        assert all(kinds[kd].dlogs["A"] == 0 for kd in ("0101", "1010"))
    if name == "g_is_h":
        assert kinds["v_cancel"].dlogs["V"] == [0] * m and all(v and x for v, x in zip(kinds["v_cancel"].vs, kinds["v_cancel"].gammas))
    if name == "u_is_g":
        assert c.gens.su == c.gens.sg
    if name == "u_is_minus_h":
        assert (c.gens.su + c.gens.sh) % Q == 0
    if name == "rho_twin":
        # rho IS s_(2 nb), and h IS the base that s_(2 nb) multiplies: S holds that point twice with the same scalar
        side, i = M.rho_twin_index(nb, m)
        assert c.gens.sh == (c.gens.sgs if side == "gs" else c.gens.shs)[i]
        for row in c.rows:
            digest = row.proof.transcript.split(b"&")[0] + b"&"
            assert R.mod_hash(str(2 * nb).encode() + digest, Q) == R.mod_hash(str(i if side == "gs" else c.n + i).encode() + digest, Q)
    if name == "some_identities":
        zg, zh, pair, opp = M.some_identities_plan(c.n)
        assert all(c.gens.sgs[i] == 0 for i in zg) and all(c.gens.shs[i] == 0 for i in zh)
        assert opp is None or (c.gens.shs[opp] + c.gens.sgs[opp]) % Q == 0
        assert pair is None or c.gens.sgs[pair[0]] == c.gens.sgs[pair[1]] != 0


def test_rows_draw_the_edge_values():
    """Every case has the six value kinds, blinding factors 0, 1 and q - 1 and seeds of 0, 1, 2, 3, 17 and 200 bytes."""
    for nb, m in M.SHAPES:
        rows = M.make_rows("control", nb, m)
        assert [row.kind for row in rows[:6]] == list(M.KINDS) and [len(row.seed) for row in rows[:6]] == [0, 1, 2, 3, 17, 200]
        flat = [x for row in rows for x in row.gammas]
        assert {0, 1, Q - 1} <= set(flat) and any(1 < x < Q - 1 for x in flat)
        top = (1 << nb) - 1
        assert rows[0].vs == [0] * m and rows[1].vs == [top] * m and rows[5].vs[-1] > top and not rows[5].valid
        assert all(a ^ b == top for a, b in zip(rows[2].vs, rows[3].vs)) and rows[2].vs[0] & 3 == 1 and rows[3].vs[0] & 3 == 2
        assert all(row.valid and max(row.vs) <= top for row in rows if row.kind != "over")


@pytest.mark.parametrize("nb,m", M.SHAPES)
def test_commit_A_lane_replay_opposite_all_equal(nb, m):
    """Every live lane holds the same sum, so every butterfly level with two live partners is a doubling in every lane; from 32
    elements every lane adds c G to c G at its second position; the result is n c G whatever the bits."""
    gens = M.SCENARIOS["opposite_all_equal"](nb, m)
    n = nb * m
    live = min(n, 16)
    for row in M.make_rows("opposite_all_equal", nb, m):
        t = M.replay_commit_A(gens, nb, row.vs)
        assert t.result == n * gens.sgs[0] % Q, row.kind
        assert t.level_doublings == [live if dist < live else 0 for dist in (1, 2, 4, 8)], row.kind
        assert t.level_cancellations == [0, 0, 0, 0] and t.lane_cancellations == 0 and t.lane_identity_then_continue == 0
        assert t.lane_doublings == (16 if n >= 32 else 0), row.kind
        # ... and the model's A is that point (h is the identity: alpha adds nothing)
    c = M.case("opposite_all_equal", nb, m)
    assert all(row.dlogs["A"] == n * gens.sgs[0] % Q for row in c.rows)


@pytest.mark.parametrize("nb,m", M.SHAPES)
def test_commit_A_lane_replay_equal_cancel(nb, m):
    """0101 / 1010: neighbouring lanes hold opposite sums and the first butterfly level cancels every live lane; lanes+- / lanes-+
    (from 32 elements): every lane cancels at every second position, and from 64 elements goes on from the identity; A is the
    identity in all four rows, and (2 popcount - n) c G in general."""
    gens = M.SCENARIOS["equal_cancel"](nb, m)
    n, c0 = nb * m, gens.sgs[0]
    live = min(n, 16)
    for row in M.make_rows("equal_cancel", nb, m):
        t = M.replay_commit_A(gens, nb, row.vs)
        pop = sum(bin(v & ((1 << nb) - 1)).count("1") for v in row.vs)
        assert t.result == (2 * pop - n) * c0 % Q, row.kind
        if row.kind in ("0101", "1010"):
            assert t.result == 0 and t.lane_cancellations + sum(t.level_cancellations) > 0, row.kind
            if m == 1 or n <= 32:             # (wider aggregated rows alternate the pattern per value: the lanes cancel inside)
                assert t.level_cancellations == [live, 0, 0, 0] and t.level_doublings == [0, 0, 0, 0], row.kind
                assert t.lane_cancellations == 0 and t.lane_doublings == (16 if n >= 32 else 0), row.kind
        if row.kind in ("lanes+-", "lanes-+"):
            per_lane = n // 16
            assert t.result == 0 and t.lane_cancellations == 16 * (per_lane // 2) and t.lane_doublings == 0, row.kind
            assert t.lane_identity_then_continue == 16 * (per_lane // 2 - 1), row.kind
            assert t.level_cancellations == [0, 0, 0, 0] and t.level_doublings == [0, 0, 0, 0], row.kind
    if n >= 64:
        assert any(row.kind == "lanes+-" for row in M.make_rows("equal_cancel", nb, m))


NATIVE = [(name, nb, m) for name in ("vector_identities", "blinding_identities", "all_identity", "equal_cancel") for nb, m in SMALL + [(64, 1)]]


@pytest.mark.parametrize("name,nb,m", NATIVE)
def test_native_host_preparation_accepts_the_model_wire_bytes(name, nb, m):
    """bpmi_rp_batch_prepare (csrc/rp_batch_host.hpp) on the model's proofs in wire formats 1, 2 and 3: rc = 0 and no bad proof, the
    same scalars and shared coefficients from the three formats, and identity points passed on as 33 zero bytes."""
    from bulletproofs_amd.rangeproofs.codec import proof_to_bytes
    from test_gpu_batch_dev import host_prepare
    c = M.case(name, nb, m)
    rows = [row for row in c.rows if row.valid]
    k = c.n.bit_length() - 1
    weights = b"".join((3 + 5 * i).to_bytes(32, "little") for i in range(4 * len(rows)))
    got = {}
    for version in (1, 2, 3):
        blobs = [proof_to_bytes(row.product, version=version) for row in rows]
        got[version] = host_prepare(c.n, m, blobs, weights, None)
        assert got[version][:2] == (0, -1), (name, nb, m, version)
    assert got[2] == got[1] and got[3] == got[1]
    comp = got[1][5]
    for j, row in enumerate(rows):
        names = ["T1", "T2", "A", "S", "u_new", "P_new"] + ["L%d" % i for i in range(k)] + ["R%d" % i for i in range(k)]
        zero = {nm for t, nm in enumerate(names) if comp[33 * (j * len(names) + t): 33 * (j * len(names) + t + 1)] == bytes(33)}
        assert zero == M.identity_names(row.dlogs) - {"V%d" % i for i in range(m)}, (name, nb, m, row.kind)
