"""The packed form of inner-product proofs (include/bpmi.h, "batch verifier of PACKED inner-product proofs") in Python, for the tests
of its preparation: packing oracle proofs, the expected records / extra pairs as Python integers, the seed-derived weights, the
single-proof oracle verdict on the objects built from the same bytes, the value of the weighted combination, and the tamper table."""
import copy
import hashlib
import random

from oracle import bp_ref as R
from oracle.ec import INF, point_from_le64, point_to_le64, secp256k1

Q, PF = secp256k1.q, secp256k1.p
le32 = lambda v: int(v).to_bytes(32, "little")
from_le = lambda b: int.from_bytes(b, "little")


def pairs_of(k, protocol):
    return 2 * k + (4 if protocol == 1 else 2)


class Packed:
    """One call's arrays; every field a bytearray (or a list of bytes: trs; None: starts)."""

    def __init__(self, k, protocol):
        self.k, self.protocol, self.count = k, protocol, 0
        self.ab, self.xs, self.lr, self.u, self.P, self.c, self.head = (bytearray() for _ in range(7))
        self.trs, self.starts = [], None

    def clone(self):
        return copy.deepcopy(self)

    def args(self):
        """(count, ab, xs, lr, transcripts, starts, u, P, c, head): the argument order of engine.packed_proof_args."""
        return (self.count, bytes(self.ab), bytes(self.xs), bytes(self.lr), list(self.trs), self.starts, bytes(self.u), bytes(self.P), bytes(self.c), bytes(self.head))

    def subset(self, idx):
        k, out = self.k, Packed(self.k, self.protocol)
        out.count = len(idx)
        for i in idx:
            out.ab += self.ab[64 * i: 64 * i + 64]
            out.xs += self.xs[32 * k * i: 32 * k * (i + 1)]
            out.lr += self.lr[128 * k * i: 128 * k * (i + 1)]
            out.P += self.P[64 * i: 64 * i + 64]
            out.c += self.c[32 * i: 32 * i + 32]
            out.head += self.head[128 * i: 128 * i + 128]
            if self.protocol == 2:
                out.u += self.u[64 * i: 64 * i + 64]
            out.trs.append(self.trs[i])
        if self.protocol == 1:
            out.u = bytearray(self.u)
        out.starts = None if self.starts is None else [self.starts[i] for i in idx]
        return out


def pack2(k, statements, with_starts=True):
    """statements: [(u, P, proof2)] of oracle objects -> Packed (Protocol 2)."""
    pk = Packed(k, 2)
    pk.starts = [] if with_starts else None
    for u, P, pr in statements:
        pk.count += 1
        pk.ab += le32(pr.a.x % Q) + le32(pr.b.x % Q)
        pk.xs += b"".join(le32(x.x) for x in pr.xs)
        pk.lr += b"".join(point_to_le64(p) for p in pr.Ls + pr.Rs)
        pk.u += point_to_le64(u)
        pk.P += point_to_le64(P)
        pk.trs.append(pr.transcript)
        if with_starts:
            pk.starts.append(pr.start_transcript)
        else:
            assert pr.start_transcript == 1
    return pk


def pack1(k, u, statements):
    """statements: [(P, c, proof1)] -> Packed (Protocol 1, one shared u)."""
    pk = Packed(k, 1)
    pk.u += point_to_le64(u)
    for P, c, p1 in statements:
        pr = p1.proof2
        assert pr.start_transcript == 3 and pr.transcript.startswith(b"&" + p1.transcript)
        pk.count += 1
        pk.ab += le32(pr.a.x % Q) + le32(pr.b.x % Q)
        pk.xs += b"".join(le32(x.x) for x in pr.xs)
        pk.lr += b"".join(point_to_le64(p) for p in pr.Ls + pr.Rs)
        pk.P += point_to_le64(P)
        pk.c += le32(c.x % Q)
        pk.head += point_to_le64(p1.u_new) + point_to_le64(p1.P_new)
        pk.trs.append(pr.transcript)
    return pk


def derive_weight(seed, index, t):
    """rp::derive_weight (csrc/rp_batch_host.hpp): SHA-256(seed || LE64(index) || t), byte 31 cleared, little-endian; 0 -> 1."""
    d = bytearray(hashlib.sha256(seed + index.to_bytes(8, "little") + bytes([t])).digest())
    d[31] = 0
    return from_le(d) or 1


def weights_from_seed(pk, seed):
    nw = 3 if pk.protocol == 1 else 1
    return [[derive_weight(seed, i, t) for t in range(nw)] for i in range(pk.count)]


def pack_weights(ws):
    return b"".join(le32(w) for row in ws for w in row)


def fields(pk, i):
    """Proof i's numbers and point bytes."""
    k = pk.k
    a, b = from_le(pk.ab[64 * i: 64 * i + 32]), from_le(pk.ab[64 * i + 32: 64 * i + 64])
    xs = [from_le(pk.xs[32 * (k * i + j): 32 * (k * i + j) + 32]) for j in range(k)]
    lr = [bytes(pk.lr[64 * (2 * k * i + j): 64 * (2 * k * i + j) + 64]) for j in range(2 * k)]
    return a, b, xs, lr


def expected(pk, i, w):
    """(record, points, scalars) of a proof with status 0 as Python integers / bytes, by the formulas of include/bpmi.h."""
    k = pk.k
    a, b, xs, lr = fields(pk, i)
    xi = [pow(x, -1, Q) for x in xs]
    rec = b"".join(le32(x) + le32(y) for x, y in zip(xs, xi)) + le32(a) + le32(b) + le32(w[0])
    P = bytes(pk.P[64 * i: 64 * i + 64])
    mid = [(-w[0] * x * x) % Q for x in xs] + [(-w[0] * y * y) % Q for y in xi]
    if pk.protocol == 2:
        pts = [bytes(pk.u[64 * i: 64 * i + 64])] + lr + [P]
        sc = [w[0] * a * b % Q] + mid + [(-w[0]) % Q]
    else:
        x = int(pk.trs[i].split(b"&")[2])
        c = from_le(pk.c[32 * i: 32 * i + 32])
        head = bytes(pk.head[128 * i: 128 * i + 128])
        pts = [head[:64]] + lr + [head[64:], P, bytes(pk.u)]
        sc = [(w[0] * a * b + w[2]) % Q] + mid + [(w[1] - w[0]) % Q, (-w[1]) % Q, (-(w[1] * c + w[2]) * x) % Q]
    return rec, b"".join(pts), b"".join(le32(s) for s in sc)


def oracle_accepts(pk, i, g, h):
    """Verifier2.verify / Verifier1.verify of the oracle on the object with proof i's bytes, plus the ABI's conventions (values below
    q, points on the curve or the identity, at most 2^17 bytes of transcript; a decimal item that is not canonical can never equal
    str(int))."""
    try:
        a, b, xs, lr = fields(pk, i)
        if a >= Q or b >= Q or any(x >= Q for x in xs) or len(pk.trs[i]) > 1 << 17:
            return False
        pts = [point_from_le64(p) for p in lr]
        P = point_from_le64(pk.P[64 * i: 64 * i + 64])
        k = pk.k
        z = lambda v: R.Zq(v, Q)
        if pk.protocol == 2:
            start = 1 if pk.starts is None else pk.starts[i]
            pr = R.Proof2(z(a), z(b), [z(x) for x in xs], pts[:k], pts[k:], pk.trs[i], start)
            return bool(R.ipa2_verify(g, h, point_from_le64(pk.u[64 * i: 64 * i + 64]), P, pr))
        c = from_le(pk.c[32 * i: 32 * i + 32])
        if c >= Q:
            return False
        items = pk.trs[i].split(b"&")
        outer = b"&".join(items[1:3]) + b"&"
        pr = R.Proof2(z(a), z(b), [z(x) for x in xs], pts[:k], pts[k:], pk.trs[i], 3)
        head = pk.head[128 * i: 128 * i + 128]
        p1 = R.Proof1(point_from_le64(head[:64]), point_from_le64(head[64:]), pr, outer)
        return bool(R.ipa1_verify(g, h, point_from_le64(pk.u), P, z(c), p1))
    except Exception:
        return False


def combination(k, g, h, rec, pts, sc, count, protocol, h_scale=None):
    """The value bpmi_ipa_verify_batch_packed_dev computes from the preparation's outputs, with the oracle's group law: the sum over
    the proofs of w a s_i g_i + w b s_i^-1 c_i h_i plus the extra pairs."""
    n, acc = 1 << k, INF
    rb = 64 * k + 96
    for p in range(count):
        r = rec[rb * p: rb * (p + 1)]
        xs = [R.Zq(from_le(r[64 * j: 64 * j + 32]), Q) for j in range(k)]
        xi = [from_le(r[64 * j + 32: 64 * j + 64]) for j in range(k)]
        a, b, w = (from_le(r[64 * k + 32 * t: 64 * k + 32 * t + 32]) for t in range(3))
        if w == 0:
            continue
        assert all(x.x * y % Q == 1 for x, y in zip(xs, xi))
        ss = [s.x for s in R.get_ss(xs, n)]
        for i in range(n):
            acc = acc + (w * a * ss[i] % Q) * g[i] + (w * b * pow(ss[i], -1, Q) * (h_scale[i] if h_scale else 1) % Q) * h[i]
    for t in range(pairs_of(k, protocol) * count):
        s = from_le(sc[32 * t: 32 * t + 32])
        if s:
            acc = acc + s * point_from_le64(pts[64 * t: 64 * t + 64])
    return acc


# ---- the tamper table: name -> (mutation of proof i of a Packed, expected status or None for "only the group equation rejects it") ----
def _set_item(tr, j, new):
    items = tr.split(b"&")
    items[j] = new
    return b"&".join(items)


def _start(pk, i):
    return 3 if pk.protocol == 1 else (1 if pk.starts is None else pk.starts[i])


def _rehash_from(tr, first_item, k):
    """Recompute every x item from item index first_item on, so that the chain is consistent again."""
    items = tr.split(b"&")
    for r in range(k):
        j = first_item + 3 * r + 2
        items[j] = str(R.mod_hash(b"&".join(items[:j]) + b"&", Q)).encode()
    return b"&".join(items)


def mut_l_item_byte(pk, i, rnd):
    j = _start(pk, i)
    item = bytearray(pk.trs[i].split(b"&")[j])
    item[5] = ord("B") if item[5] != ord("B") else ord("C")
    pk.trs[i] = _set_item(pk.trs[i], j, bytes(item))


def mut_xs_changed(pk, i, rnd):
    o = 32 * (pk.k * i + rnd.randrange(pk.k))
    pk.xs[o] ^= 1


def mut_x_item_other_decimal(pk, i, rnd):
    j = _start(pk, i) + 3 * rnd.randrange(pk.k) + 2
    pk.trs[i] = _set_item(pk.trs[i], j, str(rnd.randrange(1, Q)).encode())


def mut_x_item_leading_zeros(pk, i, rnd):
    j = _start(pk, i) + 2
    pk.trs[i] = _set_item(pk.trs[i], j, b"007" + pk.trs[i].split(b"&")[j])


def mut_x_item_sign(pk, i, rnd):
    j = _start(pk, i) + 2
    pk.trs[i] = _set_item(pk.trs[i], j, b"+" + pk.trs[i].split(b"&")[j])


def mut_a_plus_q(pk, i, rnd):
    a = from_le(pk.ab[64 * i: 64 * i + 32])
    if a + Q < 1 << 256:
        pk.ab[64 * i: 64 * i + 32] = le32(a + Q)
    else:                                             # (probability 2^-128: a is in the top sliver) -- the same convention on b's side
        pk.ab[64 * i: 64 * i + 32] = le32(Q)


def mut_r_other_parity(pk, i, rnd):
    o = 64 * (2 * pk.k * i + pk.k + rnd.randrange(pk.k))
    y = from_le(pk.lr[o + 32: o + 64])
    pk.lr[o + 32: o + 64] = le32(PF - y)


def mut_l_off_curve(pk, i, rnd):
    o = 64 * (2 * pk.k * i + rnd.randrange(pk.k))
    y = from_le(pk.lr[o + 32: o + 64])
    pk.lr[o + 32: o + 64] = le32((y + 2) % PF)        # same parity: the item still matches, the point is off the curve


def mut_cut_after_last_r(pk, i, rnd):
    items = pk.trs[i].split(b"&")
    j = _start(pk, i) + 3 * (pk.k - 1) + 1
    pk.trs[i] = b"&".join(items[: j + 1])


def mut_start_beyond(pk, i, rnd):
    pk.starts[i] = len(pk.trs[i].split(b"&")) + 5


def mut_empty_transcript(pk, i, rnd):
    pk.trs[i] = b""


def mut_item2_not_hash(pk, i, rnd):
    """Protocol 1: another canonical decimal as item 2, the rounds re-hashed consistently behind it."""
    tr = _set_item(pk.trs[i], 2, str(rnd.randrange(1, Q)).encode())
    pk.trs[i] = _rehash_from(tr, 3, pk.k)
    pk.xs[32 * pk.k * i: 32 * pk.k * (i + 1)] = b"".join(le32(int(pk.trs[i].split(b"&")[3 + 3 * r + 2])) for r in range(pk.k))


def mut_a_changed(pk, i, rnd):
    a = from_le(pk.ab[64 * i: 64 * i + 32])
    pk.ab[64 * i: 64 * i + 32] = le32((a + 1) % Q)


def mut_c_changed(pk, i, rnd):
    c = from_le(pk.c[32 * i: 32 * i + 32])
    pk.c[32 * i: 32 * i + 32] = le32((c + 1) % Q)


def mut_u_new_changed(pk, i, rnd):
    pk.head[128 * i: 128 * i + 64] = point_to_le64(7 * secp256k1.G)


def mut_p_changed(pk, i, rnd):
    pk.P[64 * i: 64 * i + 64] = point_to_le64(point_from_le64(pk.P[64 * i: 64 * i + 64]) + secp256k1.G)


def mut_l_replaced_rehashed(pk, i, rnd):
    """L_0 replaced by another curve point with the whole chain re-hashed consistently: every byte-level check passes."""
    k, s = pk.k, _start(pk, i)
    new = rnd.randrange(1, Q) * secp256k1.G
    pk.lr[128 * k * i: 128 * k * i + 64] = point_to_le64(new)
    tr = _set_item(pk.trs[i], s, R.point_to_b64(new))
    pk.trs[i] = _rehash_from(tr, s, k)
    pk.xs[32 * k * i: 32 * k * (i + 1)] = b"".join(le32(int(pk.trs[i].split(b"&")[s + 3 * r + 2])) for r in range(k))


# (name, mutation, expected status; None: status 0 and only the group equation rejects it, protocols it applies to, needs starts)
TAMPERS = [
    ("l_item_byte", mut_l_item_byte, 1, (1, 2)),
    ("xs_changed", mut_xs_changed, 1, (1, 2)),
    ("x_item_other_decimal", mut_x_item_other_decimal, 1, (1, 2)),
    ("x_item_leading_zeros", mut_x_item_leading_zeros, 1, (1, 2)),
    ("x_item_sign", mut_x_item_sign, 1, (1, 2)),
    ("a_plus_q", mut_a_plus_q, 1, (1, 2)),
    ("r_other_parity", mut_r_other_parity, 1, (1, 2)),
    ("l_off_curve", mut_l_off_curve, 2, (1, 2)),
    ("cut_after_last_r", mut_cut_after_last_r, 1, (1, 2)),
    ("start_beyond", mut_start_beyond, 1, (2,)),
    ("empty_transcript", mut_empty_transcript, 1, (1, 2)),
    ("item2_not_hash", mut_item2_not_hash, 1, (1,)),
    ("a_changed", mut_a_changed, None, (1, 2)),
    ("c_changed", mut_c_changed, None, (1,)),
    ("u_new_changed", mut_u_new_changed, None, (1,)),
    ("p_changed", mut_p_changed, None, (1, 2)),
    ("l_replaced_rehashed", mut_l_replaced_rehashed, None, (1, 2)),
]


def make_generators(n, tag=b"ipa-packed"):
    g = [R.elliptic_hash(tag + b"g%d" % i) for i in range(n)]
    h = [R.elliptic_hash(tag + b"h%d" % i) for i in range(n)]
    return g, h, R.elliptic_hash(tag + b"u")


def draw_vectors(n, rnd):
    return [R.Zq(rnd.randrange(Q), Q) for _ in range(n)], [R.Zq(rnd.randrange(Q), Q) for _ in range(n)]


def oracle_batch2(n, count, seed, prefixes=None, zero=()):
    """(g, h, Packed) of `count` Protocol-2 oracle proofs; prefixes[i]: the transcript prefix of proof i (None: none); proofs in `zero`
    have a = b = 0: every L and R is the identity ("AA==")."""
    rnd = random.Random(seed)
    g, h, u0 = make_generators(n)
    k, sts = n.bit_length() - 1, []
    for i in range(count):
        a, b = draw_vectors(n, rnd)
        if i in zero:
            a, b = [R.Zq(0, Q)] * n, [R.Zq(0, Q)] * n
        u = rnd.randrange(1, Q) * u0
        P = R.vector_commitment(g, h, a, b, R.multiexp_naive) + R.inner_product(a, b).x % Q * u
        sts.append((u, P, R.ipa2_prove(g, h, u, P, a, b, Q, prefixes[i] if prefixes else None, R.multiexp_naive)))
    return g, h, pack2(k, sts, with_starts=prefixes is not None)


def oracle_batch1(n, count, seed, seeds=None):
    rnd = random.Random(seed)
    g, h, u = make_generators(n)
    k, sts = n.bit_length() - 1, []
    for i in range(count):
        a, b = draw_vectors(n, rnd)
        c = R.inner_product(a, b)
        c = R.Zq(c.x % Q, Q)
        P = R.vector_commitment(g, h, a, b, R.multiexp_naive)          # Protocol 1's statement: P = g^a h^b, c = <a, b>
        sts.append((P, c, R.ipa1_prove(g, h, u, P, c, a, b, Q, seeds[i] if seeds else b"", R.multiexp_naive)))
    return g, h, pack1(k, u, sts)
