"""Integer model of the inner-product prover over generators with KNOWN discrete logarithms (test helper: plain Python, no GPU).

Every generator is a known multiple of the base point G: g[i] = sg[i] G, h[i] = sh[i] G, u = su G.  Everything the prover must
produce is then an integer mod q times G (the conventions of test_ipa_rounds_vs_oracle):

    c_L = <a_lo, b_hi>,  c_R = <a_hi, b_lo>
    L = (sum_{i<half} a[i] sg[half+i] + b[half+i] sh[i] + c_L su) G
    R = (sum_{i<half} a[half+i] sg[i] + b[i] sh[half+i] + c_R su) G
    fold(x, xi):  sg'[i] = xi sg[i] + x sg[half+i]     sh'[i] = x sh[i] + xi sh[half+i]
                  a'[i]  = x a[i]  + xi a[half+i]      b'[i]  = xi b[i] + x b[half+i]
    scaled:       sh[i] <- c[i] sh[i] before the first round

A dlog of 0 is the identity (64 zero bytes on the wire); equal dlogs are equal points, negated dlogs negated points -- the engine
sees only points.  `DlogIpa` returns integers; `dlogs_to_le64` turns a list of them into 64-byte points with ONE batched
multiplication of G.  The named scenarios choose generators, challenges and vectors so that the generator-fold kernels meet their
own accumulator, the identity, and coefficients whose GLV halves are 0 or +-1; test_ipa_dlog_ref_cpu.py proves from the model alone
that each scenario shows the edge it is there for."""
import random

Q = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141


def _fourth_root_of_one():
    # q = 1 mod 4: g^((q-1)/4) has order 4 exactly when g is a quadratic non-residue (Euler: g^((q-1)/2) = -1)
    for base in range(2, 100):
        if pow(base, (Q - 1) // 2, Q) == Q - 1:
            return pow(base, (Q - 1) // 4, Q)
    raise AssertionError("no quadratic non-residue below 100")


IOTA = _fourth_root_of_one()
assert Q % 4 == 1 and IOTA * IOTA % Q == Q - 1
# the cube root of unity of the GLV endomorphism and the lattice constants, as in test_gpu_ops.py
LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
assert LAMBDA != 1 and pow(LAMBDA, 3, Q) == 1
A1, MB1 = 0x3086D221A7D46BCDE86C90E49284EB15, 0xE4437ED6010E88286F547FA90ABFE4C3
A2 = A1 + MB1
# (a1, b1 = -mb1) and (a2, b2 = a1) span the lattice of pairs (k1, k2) with k1 + k2 lambda = 0
assert (A1 - MB1 * LAMBDA) % Q == 0 and (A2 + A1 * LAMBDA) % Q == 0


def glv_split(k):
    """k = k1 + k2 lambda (mod q) with |k1|, |k2| < 2^128: the nearest lattice point by rounding (signed integers)."""
    k %= Q
    c1 = (A1 * k + Q // 2) // Q
    c2 = (MB1 * k + Q // 2) // Q
    k1 = k - c1 * A1 - c2 * A2
    k2 = c1 * MB1 - c2 * A1
    assert (k1 + k2 * LAMBDA - k) % Q == 0 and abs(k1) < 1 << 128 and abs(k2) < 1 << 128
    return k1, k2


class DlogIpa:
    """The prover's state as dlogs.  sh is taken scaled when `hscale` is given (bpmi_ipa_create_scaled)."""

    def __init__(self, sg, sh, su, a, b, hscale=None):
        n = len(sg)
        assert n and n & (n - 1) == 0 and len(sh) == len(a) == len(b) == n and (hscale is None or len(hscale) == n)
        self.sg = [v % Q for v in sg]
        self.sh = [v % Q for v in sh] if hscale is None else [c * v % Q for c, v in zip(hscale, sh)]
        self.su = su % Q
        self.a = [v % Q for v in a]
        self.b = [v % Q for v in b]

    def __len__(self):
        return len(self.a)

    def round_LR(self):
        """(dlog of L, dlog of R)"""
        half = len(self) // 2
        sg, sh, a, b = self.sg, self.sh, self.a, self.b
        cl = sum(a[i] * b[half + i] for i in range(half))
        cr = sum(a[half + i] * b[i] for i in range(half))
        L = sum(a[i] * sg[half + i] + b[half + i] * sh[i] for i in range(half)) + cl % Q * self.su
        R = sum(a[half + i] * sg[i] + b[i] * sh[half + i] for i in range(half)) + cr % Q * self.su
        return L % Q, R % Q

    def fold(self, x, xi):
        half = len(self) // 2
        sg, sh, a, b = self.sg, self.sh, self.a, self.b
        self.sg = [(xi * sg[i] + x * sg[half + i]) % Q for i in range(half)]
        self.sh = [(x * sh[i] + xi * sh[half + i]) % Q for i in range(half)]
        self.a = [(x * a[i] + xi * a[half + i]) % Q for i in range(half)]
        self.b = [(xi * b[i] + x * b[half + i]) % Q for i in range(half)]

    def export(self):
        """(dlogs of g, dlogs of h, a, b) of the current round"""
        return list(self.sg), list(self.sh), list(self.a), list(self.b)

    def finish(self):
        assert len(self) == 1
        return self.a[0], self.b[0]


def dlogs_to_le64(dlogs, mul_batch=None):
    """[k] -> [64-byte encoding of k G], one batched multiplication of G over the DISTINCT values (0: 64 zero bytes).
    mul_batch(points, scalars) -> points; default the C oracle's."""
    from oracle.ec import point_to_le64, secp256k1
    if mul_batch is None:
        from oracle import cbind
        mul_batch = cbind.ec_mul_batch
    uniq = sorted({k % Q for k in dlogs} - {0})
    enc = {0: bytes(64)}
    if uniq:
        for k, pt in zip(uniq, mul_batch([secp256k1.G] * len(uniq), uniq)):
            enc[k] = point_to_le64(pt)
    return [enc[k % Q] for k in dlogs]


def pack_scalars(vs):
    return b"".join((v % Q).to_bytes(32, "little") for v in vs)


# ---- scenarios -----------------------------------------------------------------------------------------------------------------
POOL = 16          # distinct dlogs per side before signs: at most 4 POOL distinct generator points in any scenario


def _fold4(i):
    """XOR of the base-16 digits of i.  i -> i + t m (m a power of two, i < m, t < 16) changes four neighbouring bits, which
    fall on four different bit positions of the result: the 16 generators that one output of a 16-way fold adds up, and the two
    that a pairwise fold adds up, get 16 (2) DIFFERENT pool entries."""
    r = 0
    while i:
        r ^= i & 15
        i >>= 4
    return r


def _base(name, n):
    assert n >= 16 and n & (n - 1) == 0
    rnd = random.Random("ipa-dlog/%s/%d" % (name, n))
    pool_g = [rnd.randrange(1, Q) for _ in range(POOL)]
    pool_h = [rnd.randrange(1, Q) for _ in range(POOL)]
    su = rnd.randrange(1, Q)
    a = [rnd.randrange(Q) for _ in range(n)]
    b = [rnd.randrange(Q) for _ in range(n)]
    xs = [rnd.randrange(2, Q - 1) for _ in range(n.bit_length() - 1)]
    return rnd, pool_g, pool_h, su, a, b, xs


def _distinct(pool_g, pool_h, n):
    return [pool_g[_fold4(i)] for i in range(n)], [pool_h[_fold4(i)] for i in range(n)]


def sc_control(n):
    _, pg, ph, su, a, b, xs = _base("control", n)
    sg, sh = _distinct(pg, ph, n)
    return sg, sh, su, a, b, xs, None


def _all_equal(name, n, x):
    _, pg, _, su, a, b, xs = _base(name, n)
    return [pg[0]] * n, [pg[0]] * n, su, a, b, [x] * len(xs), None


def sc_all_equal_ones(n):
    """One point everywhere, x = 1: every coefficient is 1 = (1, 0) in GLV halves, every ladder's second addition adds P to P,
    every folded generator is 2^r P."""
    return _all_equal("all_equal_ones", n, 1)


def sc_all_equal_minus(n):
    """One point everywhere, x = -1 = (-1, 0): the coefficients are (-1)^d -- all -1 after an odd number of deferred folds (the
    scalars of the deferred L / R and of an export), all +1 at the 16-way folds, whose fourth level makes them meet P + P again."""
    return _all_equal("all_equal_minus", n, Q - 1)


def halves_period(n):
    return min(POOL, n // 16)


def sc_halves_equal_iota(n):
    """sg[i + half] = sg[i] at every level down to the period, x = iota, 1 / x = -iota: the coefficients are +-1 and +-iota, the
    ladders add P to P and -P to P, and g' = (xi + x) g = 0, h' = 0 for every i after the FIRST fold: whole waves of identities."""
    _, pg, ph, su, a, b, xs = _base("halves_equal_iota", n)
    p = halves_period(n)
    return [pg[i % p] for i in range(n)], [ph[i % p] for i in range(n)], su, a, b, [IOTA] * len(xs), None


def sc_halves_opposite_ones(n):
    """sg[i + n/2] = -sg[i], x = 1 first: g' = g_lo + g_hi = 0 and h' = 0 after the first fold, behind coefficients 1."""
    _, pg, ph, su, a, b, xs = _base("halves_opposite_ones", n)
    sg, sh = _distinct(pg, ph, n // 2)
    return sg + [Q - v for v in sg], sh + [Q - v for v in sh], su, a, b, [1] + xs[1:], None


def sc_lambda(n):
    """x cycles lambda, lambda^2, -lambda: every coefficient is +-1, +-lambda or +-lambda^2 = -+(1 + lambda): GLV halves 0 and +-1."""
    _, pg, ph, su, a, b, xs = _base("lambda", n)
    sg, sh = _distinct(pg, ph, n)
    cyc = [LAMBDA, LAMBDA * LAMBDA % Q, Q - LAMBDA]
    return sg, sh, su, a, b, [cyc[r % 3] for r in range(len(xs))], None


def sc_undo(n):
    """x, 1/x, x, 1/x, ...: the 2^d coefficients are x^e with few distinct e; after every second fold many are 1 again."""
    _, pg, ph, su, a, b, xs = _base("undo", n)
    sg, sh = _distinct(pg, ph, n)
    x = xs[0]
    return sg, sh, su, a, b, [x if r % 2 == 0 else pow(x, -1, Q) for r in range(len(xs))], None


def identity_positions(n):
    """Where `identities` puts dlog 0 among g (h: the same shifted by one): index 0, index n - 1, one full stride class of the
    16-way fold {i0 + t n/16} (n >= 64), and a run of min(64, n / 4) indices aligned to its length."""
    run = min(64, n // 4)
    start = (n // 2 + run) // run * run % n
    pos = {0, n - 1} | set(range(start, start + run))
    if n >= 64:
        pos |= {n // 16 - 1 + t * (n // 16) for t in range(16)}
    return pos


def sc_identities(n):
    _, pg, ph, su, a, b, xs = _base("identities", n)
    sg, sh = _distinct(pg, ph, n)
    for i in identity_positions(n):
        sg[i] = 0
        sh[(i + 1) % n] = 0
    fixed = [2, (Q + 1) // 2, 1 << 128, A1, Q - MB1]
    return sg, sh, su, a, b, (fixed + xs[len(fixed):])[:len(xs)], None


SMALL = list(range(1, 9)) + [Q - k for k in range(1, 9)]


def sc_small_multiples(n):
    """dlogs +-1 .. +-8, arranged so that the 16 generators under one output are all 16 of them: a table entry 3P, 5P, 7P of one
    base IS another base (or its negative), and small partial sums of the ladders' leading digits collide."""
    _, _, _, su, a, b, xs = _base("small_multiples", n)
    sg = [SMALL[_fold4(i)] for i in range(n)]
    sh = [SMALL[(_fold4(i) + 5) % 16] for i in range(n)]
    fixed = [3, 5, 7, 1]
    return sg, sh, su, a, b, (fixed + xs[len(fixed):])[:len(xs)], None


def sc_zero_vectors(n):
    """a_lo = 0 but a[0] = -1, b = 0 in its third quarter, and b[n - 1] solved so that the FIRST L is the identity: MSMs most of
    whose scalars are zero, one of them with the identity for a result."""
    _, pg, ph, su, a, b, xs = _base("zero_vectors", n)
    sg, sh = _distinct(pg, ph, n)
    half = n // 2
    for i in range(half):
        a[i] = 0
    a[0] = Q - 1
    for i in range(half, half + n // 4):
        b[i] = 0
    # L = -sg[half] - b[half] su + sum_{i < half} b[half + i] sh[i] with b[half] = 0: choose the last term
    rest = sum(b[half + i] * sh[i] for i in range(half - 1))
    b[n - 1] = (sg[half] - rest) * pow(sh[half - 1], -1, Q) % Q
    return sg, sh, su, a, b, xs, None


SCENARIOS = {
    "control": sc_control,
    "all_equal_ones": sc_all_equal_ones,
    "all_equal_minus": sc_all_equal_minus,
    "halves_equal_iota": sc_halves_equal_iota,
    "halves_opposite_ones": sc_halves_opposite_ones,
    "lambda": sc_lambda,
    "undo": sc_undo,
    "identities": sc_identities,
    "small_multiples": sc_small_multiples,
    "zero_vectors": sc_zero_vectors,
}


def hscale_for(n):
    """The per-generator scale of the scaled form: 1, -1, 2 at known places, random elsewhere, never 0."""
    rnd = random.Random("ipa-dlog/hscale/%d" % n)
    c = [rnd.randrange(1, Q) for _ in range(n)]
    for i in range(0, n, 5):
        c[i] = (1, Q - 1, 2)[i // 5 % 3]
    return c


def scenario(name, n, scaled=False):
    sg, sh, su, a, b, xs, hscale = SCENARIOS[name](n)
    assert len({v for v in sg + sh if v}) <= 4 * POOL
    return sg, sh, su, a, b, xs, (hscale_for(n) if scaled else hscale)


def coefficients(xs):
    """The 2^d coefficients of d deferred folds with challenges xs (first fold first), for g and for h, as the engine's tables
    hold them: out[i] = sum_t coef[t] base[i + t m]."""
    cg, ch = [1], [1]
    for x in xs:
        xi = pow(x, -1, Q)
        cg = [c * (x if j else xi) % Q for c in cg for j in (0, 1)]
        ch = [c * (xi if j else x) % Q for c in ch for j in (0, 1)]
    return cg, ch


def expected_trace(name, n, scaled=False, export_max=64):
    """The run every GPU case makes, on the model: per round L, R (while the length is above 1), an export at every length
    <= export_max, the fold; then the final (a, b).  -> (events, case): events are ("LR", length, L64, R64), ("export", length,
    g bytes, h bytes, a bytes, b bytes), ("finish", a, b) with points as wire bytes; case is the scenario's tuple."""
    case = scenario(name, n, scaled)
    sg, sh, su, a, b, xs, hscale = case
    m = DlogIpa(sg, sh, su, a, b, hscale)
    raw, want = [], []
    r = 0
    while True:
        ln = len(m)
        if ln > 1:
            L, R = m.round_LR()
            raw.append(("LR", ln, len(want)))
            want += [L, R]
        if ln <= export_max:
            eg, eh, ea, eb = m.export()
            raw.append(("export", ln, len(want), ea, eb))
            want += eg + eh
        if ln == 1:
            break
        m.fold(xs[r], pow(xs[r], -1, Q))
        r += 1
    enc = dlogs_to_le64(want)
    events = []
    for ev in raw:
        if ev[0] == "LR":
            events.append(("LR", ev[1], enc[ev[2]], enc[ev[2] + 1]))
        else:
            _, ln, at, ea, eb = ev
            events.append(("export", ln, b"".join(enc[at: at + ln]), b"".join(enc[at + ln: at + 2 * ln]), pack_scalars(ea), pack_scalars(eb)))
    events.append(("finish",) + m.finish())
    return events, case
