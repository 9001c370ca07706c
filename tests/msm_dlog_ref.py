"""Integer model of the LAST stage of every MSM -- bucket sums X[w][b] -> window sums E[w] = sum_b b X[w][b] -> the Horner chain of
the tail -- over points with KNOWN discrete logarithms (test helper: plain Python, no GPU).

Every point is a known multiple of the base point G: P = k G, -P, the identity (dlog 0, 64 zero bytes on the wire) and small
multiples of P.  A bucket sum, a window sum and the result are then integers mod q times G, and `ipa_dlog_ref.dlogs_to_le64` turns the
total into the 64 expected bytes with ONE multiplication of G, whatever n is.  Sums of different random subsets never coincide, so
random inputs reach none of the exceptional outcomes of the general addition behind the reduction (an identity operand apart): here
whole windows of buckets hold ONE point (every first addition of a lane or a tree is A + A), +-P in a pattern that makes every
window sum the identity (some addition is A + (-A)), or five small multiples side by side.

Two recodings, written from the comments of csrc/msm_kernels.hpp and not by calling the engine:
  pipeline / small kernel (for_each_digit): s mod q, folded to q - s on the NEGATED point when above (q - 1) / 2; windows of c bits,
    the last `wide` of them one bit wider; a window value t (with the carry in) above 2^(wd - 1) becomes the negative digit
    t - 2^wd with a carry out, so a digit of magnitude 2^(wd - 1) is never negative;
  mid (k_msm_mid, msm_mid_block): the same fold, then with K = 64 sum_{j < 36} 2^(7 j) the 7-bit field j of s + K is d_j + 64 for
    digits d_j in [-64, 63] -- magnitude 64 is only ever negative --, and the four-bit top field (bits 252 .. 255) is unsigned.

`Geo` is the window list of one geometry, `run` the bucket table / window sums / total of a list of (dlog, scalar) pairs,
`replay_tail` the integer replay of msm_tail_combine (which additions of the chain were identity operands, doublings, cancellations,
ordinary), and the scenario functions build the inputs.  test_msm_dlog_ref_cpu.py proves from this model alone that each scenario
shows the edge it is there for; test_gpu_msm_reduce_degenerate.py holds the engine's bytes against the model's."""
import random

from ipa_dlog_ref import Q, dlogs_to_le64, pack_scalars  # noqa: F401  (re-exported: the GPU file packs with them)

HALF = (Q - 1) // 2
MID_C, MID_W, MID_B = 7, 37, 64
MID_K = sum(64 << (7 * j) for j in range(36))


class Geo:
    """The windows of one geometry: kind "pipeline" (also the small kernel: c = 8, 32 windows, none wide) or "mid"."""

    def __init__(self, kind, c, W, wide=0):
        assert kind in ("pipeline", "mid") and 0 <= wide < W
        self.kind, self.c, self.W, self.wide = kind, c, W, wide
        self.wins, at = [], 0                                  # [(bit offset, width)]
        if kind == "mid":
            assert (c, W, wide) == (MID_C, MID_W, 0)
            self.wins = [(7 * j, 7) for j in range(36)] + [(252, 4)]
        else:
            for w in range(W):
                wd = c + (1 if w + wide >= W else 0)
                self.wins.append((at, wd))
                at += wd
            assert not wide or at == 256, "mixed widths cover the 256 bit positions exactly"
            assert at >= 255, "the windows cover every bit of a folded scalar"

    @classmethod
    def from_engine(cls, geom):
        """From what Engine.msm_geometry reports: kernel, window_bits, windows, wide_windows."""
        kind = "mid" if geom["kernel"] == "mid" else "pipeline"
        return cls(kind, geom["window_bits"], geom["windows"], geom["wide_windows"])

    def key(self):
        return (self.kind, self.c, self.W, self.wide)

    def __repr__(self):
        return "Geo(%s, c=%d, W=%d, wide=%d)" % self.key()

    def buckets(self, w):
        """bucket indices of window w are 1 .. buckets(w)"""
        return MID_B if self.kind == "mid" else 1 << (self.wins[w][1] - 1)

    def limit(self, w):
        """The largest digit b that a scenario may put into window w of a scalar that is NOT folded (s <= (q - 1) / 2 whatever the
        other windows hold) and that stays positive without a carry: 2^(wd - 1) in the pipeline, 63 in the mid recoding, and in the
        top windows what b 2^at < q / 2 leaves."""
        at, wd = self.wins[w]
        room = max((HALF >> at) - 1, 0)
        if self.kind == "mid":
            return min(63 if w < 36 else 15, room)
        return min(1 << (wd - 1), room)

    def limits(self):
        return [self.limit(w) for w in range(self.W)]

    # ---- the two recodings ------------------------------------------------------------------------------------------------------
    def raw_digits(self, s):
        """(negated, [signed digit per window]) of scalar s (any 256-bit value below 2 q: reduced once, as the device does):
        sum_w digit 2^at = the folded scalar, exactly."""
        assert 0 <= s < 2 * Q and s < 1 << 256
        if s >= Q:
            s -= Q
        neg = s > HALF
        if neg:
            s = Q - s
        out = []
        if self.kind == "mid":
            v = s + MID_K
            assert v < 1 << 256
            for j in range(36):
                out.append(((v >> (7 * j)) & 127) - 64)
            out.append(v >> 252)
        else:
            carry = 0
            for at, wd in self.wins:
                t = ((s >> at) & ((1 << wd) - 1)) + carry
                if t > 1 << (wd - 1):
                    out.append(t - (1 << wd))
                    carry = 1
                else:
                    out.append(t)
                    carry = 0
            assert carry == 0 and s >> (self.wins[-1][0] + self.wins[-1][1]) == 0
        return neg, out

    def digits(self, s):
        """[signed digit per window] with the fold's sign applied: sum_w digit 2^at = s (mod q)"""
        neg, ds = self.raw_digits(s)
        return [-d for d in ds] if neg else ds

    def scalar(self, ds):
        """the scalar whose digits are ds (all within limit(w): positive, no carry, not folded)"""
        assert len(ds) == self.W and all(0 <= d <= self.limit(w) for w, d in enumerate(ds)), ds
        s = sum(d << self.wins[w][0] for w, d in enumerate(ds))
        assert s <= HALF
        return s


class Result:
    """X[w] = {bucket: value mod q} over the buckets that received an entry of a non-identity point (the value may still be 0),
    E[w] = sum_b b X[w][b], total = sum_w 2^at E[w]."""

    def __init__(self, geo, X):
        self.geo, self.X = geo, X
        self.E = [sum(b * v for b, v in x.items()) % Q for x in X]
        self.total = sum(e << geo.wins[w][0] for w, e in enumerate(self.E)) % Q

    def bytes(self):
        return dlogs_to_le64([self.total])[0]

    def split(self, offs, wide_offs=None):
        """E[w][v] of the four-digit bucket reduction (msm_reduce_plan): b = hi 2^s0 + lo, each half cut again, the four digits'
        bit offsets being the tail's `offs` = [0, t_lo, s0, s0 + t_hi] (`wide_offs` for the wide windows)."""
        out = []
        for w, x in enumerate(self.X):
            o = wide_offs if (self.geo.wide and w + self.geo.wide >= self.geo.W) else offs
            s0, t_lo, t_hi = o[2], o[1], o[3] - o[2]
            e = [0, 0, 0, 0]
            for b, v in x.items():
                lo, hi = b & ((1 << s0) - 1), b >> s0
                four = (lo & ((1 << t_lo) - 1), lo >> t_lo, hi & ((1 << t_hi) - 1), hi >> t_hi)
                assert sum(d << o[i] for i, d in enumerate(four)) == b
                for i, d in enumerate(four):
                    e[i] += d * v
            out.append([v % Q for v in e])
        return out


def run(geo, dlogs, scalars):
    assert len(dlogs) == len(scalars)
    X = [dict() for _ in range(geo.W)]
    cache = {}
    for k, s in zip(dlogs, scalars):
        k %= Q
        if k == 0:
            continue                                       # the identity adds nothing to any bucket
        ds = cache.get(s)
        if ds is None:
            ds = cache[s] = geo.digits(s)
        for w, d in enumerate(ds):
            if d:
                b = -d if d < 0 else d
                assert b <= geo.buckets(w), (geo, w, d)
                x = X[w]
                x[b] = (x.get(b, 0) + (k if d > 0 else Q - k)) % Q
    return Result(geo, X)


KINDS = ("identity", "doubling", "cancellation", "ordinary")


def classify(acc, e):
    if acc == 0 or e == 0:
        return "identity"
    if acc == e:
        return "doubling"
    return "cancellation" if (acc + e) % Q == 0 else "ordinary"


def replay_tail(geo, E, offs=None, wide_offs=None):
    """msm_tail_combine on integers: ONE chain from the top bit position down, a doubling per position and an addition where a
    record's offset matches.  E[w] is an integer (nv = 1: the record of window w at offset 0) or a list of nv values with the
    tail's `offs` (`wide_offs` in the wide windows).  -> (total, [kind of every addition, in order])."""
    acc, kinds = 0, []
    for w in range(geo.W - 1, -1, -1):
        rec = E[w] if isinstance(E[w], (list, tuple)) else [E[w]]
        o = [0] if offs is None else ((wide_offs if (geo.wide and w + geo.wide >= geo.W) else offs)[:len(rec)])
        for r in range(geo.wins[w][1] - 1, -1, -1):
            acc = 2 * acc % Q
            if r in o:
                e = rec[o.index(r)]                        # (the device takes the first record whose offset matches)
                kinds.append(classify(acc, e))
                acc = (acc + e) % Q
    return acc, kinds


def count_kinds(kinds):
    return {k: kinds.count(k) for k in KINDS}


# ---- scenarios: (geo, n) -> (dlogs, scalars); n = None: the natural size ----------------------------------------------------------
def base_dlog(name):
    return random.Random("msm-dlog/" + name).randrange(1, Q)


def _by_bucket(geo, b, limits):
    """the scalar with digit b in every window whose limit admits it"""
    return geo.scalar([b if b <= lim else 0 for lim in limits])


def mid_bucket64_pair(geo, k):
    """Bucket 64 of the mid recoding holds only NEGATIVE digits: the fields 64, 63, 63, ... of s make every field of s + K zero with
    a carry -- digit -64 in all 36 signed windows -- and the last carry lands in the unsigned top field.  On the point -k G that
    is +k in bucket 64 of every window and -k in a bucket of the top window ABOVE its limit; the model accounts for it."""
    assert geo.kind == "mid"
    s = 64 + sum(63 << (7 * j) for j in range(1, 36)) + (geo.limit(36) << 252)
    assert s <= HALF and geo.digits(s) == [-64] * 36 + [geo.limit(36) + 1]
    return Q - k, s


def fit(pairs, n, k, name):
    """`pairs` repeated to the largest multiple that fits n (every bucket value times the number of copies) and filled up with pairs
    that add nothing: the identity under a random scalar, and a point under the scalar 0.  n = None: as they are."""
    if n is None:
        return [p[0] for p in pairs], [p[1] for p in pairs]
    assert pairs and n >= len(pairs), (name, n, len(pairs))
    rnd = random.Random("msm-dlog/pad/%s/%d" % (name, n))
    out = pairs * (n // len(pairs))
    while len(out) < n:
        out.append((0, rnd.randrange(Q)) if len(out) % 2 else (k, 0))
    return [p[0] for p in out], [p[1] for p in out]


def _prefix(pairs, n, unit=1):
    if n is not None and len(pairs) > n:
        pairs = pairs[:n - n % unit]
    return pairs


def sc_full_equal(geo, n=None):
    """Pair b carries digit b in every window where b is a legal positive digit: every bucket up to each window's limit holds
    exactly P, and the first addition of two elements in any lane or tree is P + P.  (mid: bucket 64 through mid_bucket64_pair.)"""
    k, lims = base_dlog("full_equal"), geo.limits()
    pairs = _prefix([(k, _by_bucket(geo, b, lims)) for b in range(1, max(lims) + 1)], n)
    if geo.kind == "mid":
        pairs.append(mid_bucket64_pair(geo, k))
    return fit(pairs, n, k, "full_equal")


def zero_limits(geo):
    return [lim - lim % 4 for lim in geo.limits()]


def sc_window_zero(geo, n=None):
    """The same pairs with +k for b = 0, 1 (mod 4) and -k for b = 2, 3, every window's range cut to a multiple of four:
    (4j + 1) - (4j + 2) - (4j + 3) + (4j + 4) = 0, so every bucket is +-P and every window sum is the identity."""
    k, lims = base_dlog("window_zero"), zero_limits(geo)
    pairs = _prefix([(k if b % 4 < 2 else Q - k, _by_bucket(geo, b, lims)) for b in range(1, max(lims) + 1)], n, 4)
    return fit(pairs, n, k, "window_zero")


MULTIPLES = (-2, -1, 0, 1, 2)


def multiple_of(b):
    return MULTIPLES[(b - 1) % 5]


def sc_mixed_multiples(geo, n=None):
    """Bucket b holds m_b P, m_b cycling through -2, -1, 0, 1, 2: |m| entries of the point sign(m) P (two entries of one point: the
    accumulation's doubling), none for 0."""
    k, lims = base_dlog("mixed_multiples"), geo.limits()
    pairs = []
    for b in range(1, max(lims) + 1):
        m = multiple_of(b)
        pairs += [(k if m > 0 else Q - k, _by_bucket(geo, b, lims))] * abs(m)
    return fit(_prefix(pairs, n), n, k, "mixed_multiples")


def sparse_buckets(geo):
    """the one bucket of window w: 1 and the window's last legal bucket in turn (B, 2B in a wide window; mid: 63; 0: a window no
    unfolded scalar reaches)"""
    return [min(lim, 1) if w % 2 == 0 else lim for w, lim in enumerate(geo.limits())]


def sc_sparse_edges(geo, n=None):
    """One non-empty bucket per window, at b = 1 and at the window's last bucket in turn; three points share the windows.  (mid: bucket
    64 of every window besides, through mid_bucket64_pair.)"""
    k, bs = base_dlog("sparse_edges"), sparse_buckets(geo)
    pairs = [((j + 1) * k % Q, geo.scalar([b if w % 3 == j else 0 for w, b in enumerate(bs)])) for j in range(3)]
    if geo.kind == "mid":
        pairs.append(mid_bucket64_pair(geo, k))
    return fit(pairs, n, k, "sparse_edges")


def sc_one_bucket(geo, n=4096):
    """One point, every scalar equal: one non-empty bucket per window, holding n P; every chunk partial of the chunked accumulation
    is the same multiple of P, so every level of k_segscan and every butterfly of the small kernel is a doubling."""
    rnd = random.Random("msm-dlog/one_bucket")
    k = base_dlog("one_bucket")
    s = geo.scalar([rnd.randrange(1, lim + 1) if lim else 0 for lim in geo.limits()])
    return [k] * n, [s] * n


# two-bucket shapes for the tail: E[1] = b1 P from one pair in window 1, E[0] = -+ copies b0 P in window 0 with copies b0 = 2^c
TAIL_PICKS = (0, 1, 2)      # b0 = B, B / 2, B / 4 (2, 4, 8 copies)


def tail_shape(geo, pick=0):
    """(b1, b0, copies) of candidate `pick`"""
    c = geo.wins[0][1]
    b0 = (1 << (c - 1)) >> pick
    assert b0 >= 1 and geo.wins[1][0] == c
    return 1, b0, (1 << c) // b0


def _tail(geo, n, name, sign, pick):
    k = base_dlog(name)
    b1, b0, copies = tail_shape(geo, pick)
    assert b0 <= geo.limit(0) and b1 <= geo.limit(1)
    pairs = [(k, b1 << geo.wins[1][0])] + [(k if sign > 0 else Q - k, b0 << geo.wins[0][0])] * copies
    return fit(pairs, n, k, name)


def tail_pick(geo):
    """the mid recoding has no positive digit 64 = B: its window 0 takes 4 x 32"""
    return 1 if geo.kind == "mid" else 0


def sc_tail_cancel(geo, n=None):
    """(P, 2^at_1) and copies x (-P, b0 2^at_0) with copies b0 = 2^c: E[1] = P, E[0] = -2^c P, the Horner accumulator meets its
    negative at window 0 and the total is the identity with non-identity window sums."""
    return _tail(geo, n, "tail_cancel", -1, tail_pick(geo))


def sc_tail_double(geo, n=None):
    """The same with +P: E[0] = 2^c E[1], the Horner accumulator equals its addend at window 0."""
    return _tail(geo, n, "tail_double", +1, tail_pick(geo))


SCENARIOS = {
    "full_equal": sc_full_equal,
    "window_zero": sc_window_zero,
    "mixed_multiples": sc_mixed_multiples,
    "sparse_edges": sc_sparse_edges,
    "one_bucket": sc_one_bucket,
    "tail_cancel": sc_tail_cancel,
    "tail_double": sc_tail_double,
}


def scenario(geo, name, n=None):
    dlogs, scalars = SCENARIOS[name](geo, n) if n is not None else SCENARIOS[name](geo)
    assert len({d for d in dlogs if d}) <= 4 and (n is None or len(dlogs) == n)
    return dlogs, scalars


# ---- three scenarios over ONE shared point set (the batched MSM: rows of scalars, the points are the same for every row) ----------
BATCH_ROWS = ("full_equal", "window_zero", "mixed_multiples")
BATCH_BLOCK = 2 * 63 + 1


def batch_rows(geo, n):
    """Two slots per bucket b = 1 .. 63, both the point s_b k G with the sign of window_zero's pattern, and the bucket-64 pair.  A row
    reaches +P through the scalar s on +P or q - s on -P (the fold negates the point), 2P through both slots, nothing through the
    scalar 0: row 0 is full_equal, row 1 window_zero, row 2 mixed_multiples -- three different results over the same points.
    -> (dlogs, [scalars of row 0, 1, 2])"""
    assert geo.kind == "mid" and n >= BATCH_BLOCK
    k, lims, zlims = base_dlog("batch_rows"), geo.limits(), zero_limits(geo)
    dlogs, rows = [], [[], [], []]
    for b in range(1, 64):
        plus = b % 4 < 2
        dlogs += [k if plus else Q - k] * 2
        s = _by_bucket(geo, b, lims)
        toward = lambda positive, s=s: s if positive == plus else Q - s      # noqa: E731  (the scalar that adds +-P to bucket b)
        rows[0] += [toward(True), 0]
        rows[1] += [_by_bucket(geo, b, zlims), 0]
        m = multiple_of(b)
        rows[2] += [toward(m > 0) if abs(m) >= 1 else 0, toward(m > 0) if abs(m) == 2 else 0]
    d64, s64 = mid_bucket64_pair(geo, k)
    dlogs.append(d64)
    rows[0].append(s64)
    rows[1].append(0)
    rows[2].append(0)
    assert len(dlogs) == BATCH_BLOCK
    copies = n // BATCH_BLOCK
    dlogs, rows = dlogs * copies, [r * copies for r in rows]
    rnd = random.Random("msm-dlog/batch-pad/%d" % n)
    while len(dlogs) < n:                                  # the identity under random scalars, a point under zeros
        ident = len(dlogs) % 2 == 1
        dlogs.append(0 if ident else k)
        for r in rows:
            r.append(rnd.randrange(Q) if ident else 0)
    return dlogs, rows


# ---- what each scenario must show, from the model alone (test_msm_dlog_ref_cpu.py; AssertionError with the window) ------------------
def effective_limits(res, limits):
    """the limits of a scenario cut short by its size n: window 0 admits every b, so its highest non-empty bucket is how far the pairs got"""
    top = max(res.X[0])
    return [min(lim, top) for lim in limits]


def check_full_equal(geo, res, limits=None):
    values = set()
    for w, lim in enumerate(limits or geo.limits()):
        for b in range(1, lim + 1):
            assert b in res.X[w], (geo, w, b)
            values.add(res.X[w][b])
        if geo.kind == "mid" and w < 36:
            values.add(res.X[w].get(64))
    assert len(values) == 1 and values.pop() not in (0, None), geo


def check_window_zero(geo, res, limits=None):
    values = set()
    for w, lim in enumerate(limits or zero_limits(geo)):
        assert res.E[w] == 0, (geo, w)
        here = set(res.X[w].values())
        assert 0 not in here, (geo, w)
        if lim >= 4:
            assert len(here) == 2 and sum(here) == Q, (geo, w, here)      # both signs present
        values |= here
    assert len(values) == 2 and sum(values) == Q, geo


SHARE_FROM = 24       # floor(L / 5) >= L / 6 for every L >= 24: below that, five values cannot each hold a sixth of L buckets


def check_mixed_multiples(geo, res, limits=None):
    """Each of the five values holds at least a sixth of the window's buckets 1 .. limit (the buckets a digit can reach) in every
    window with at least SHARE_FROM of them; a smaller window shows every value it has room for (limit >= 5: all five)."""
    vals = sorted({v for x in res.X for v in x.values()} - {0})
    assert len(vals) == 4, (geo, vals)
    unit = [v for v in vals if {v, 2 * v % Q, Q - v, (Q - 2 * v) % Q} == set(vals)][0]
    names = {0: 0, unit: 1, 2 * unit % Q: 2, Q - unit: -1, (Q - 2 * unit) % Q: -2}
    for w, lim in enumerate(limits or geo.limits()):
        count = dict.fromkeys(MULTIPLES, 0)
        for b in range(1, lim + 1):
            count[names[res.X[w].get(b, 0)]] += 1
        if lim >= SHARE_FROM:
            assert all(6 * v >= lim for v in count.values()), (geo, w, lim, count)
        else:
            assert sum(1 for v in count.values() if v) == min(lim, 5), (geo, w, lim, count)


def check_one_bucket(geo, res):
    for w, lim in enumerate(geo.limits()):
        assert len(res.X[w]) == (1 if lim else 0) and 0 not in res.X[w].values(), (geo, w)


def check_sparse_edges(geo, res):
    most = 2 if geo.kind == "mid" else 1                   # (mid: bucket 64 besides, and in the top window where its carry lands)
    seen = set()
    for w, lim in enumerate(geo.limits()):
        assert len(res.X[w]) <= most and (not lim or res.X[w]) and 0 not in res.X[w].values(), (geo, w)
        seen |= {(b, geo.buckets(w)) for b in res.X[w]}
    assert any(b == 1 for b, _ in seen) and any(b == B for b, B in seen), (geo, seen)        # the first and the last bucket of a window


def check_tail(geo, res, name, offs=None, wide_offs=None):
    """tail_cancel: at least one cancellation and no ordinary addition after it; tail_double: at least one doubling."""
    E = res.E if offs is None else res.split(offs, wide_offs)
    total, kinds = replay_tail(geo, E, offs, wide_offs)
    assert total == res.total, (geo, name)
    if name == "tail_cancel":
        assert "cancellation" in kinds and "ordinary" not in kinds[kinds.index("cancellation"):], (geo, kinds)
        assert total == 0 and any(res.E), geo
    else:
        assert "doubling" in kinds, (geo, kinds)
    return kinds
