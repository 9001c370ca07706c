"""Python-integer reference of the batch s-vector sums (bpmi_sc_svector_sum), shared by the CPU test of the host-built kernel bodies
and the GPU test of the kernels:  SA_i = sum_p w_p a_p s_{p,i},  SB_i = c_i sum_p w_p b_p s_{p,i}^-1  with s_{p,i} from oracle.bp_ref.get_ss
(the bit order of Verifier2.get_ss)."""
import random

from oracle import bp_ref as R

Q = R.Q


def draw_proofs(k, proofs, seed, edges=True):
    """`proofs` tuples (xs, a, b, w): random, with the edge values spread over the first proofs when `edges` -- a = 0, b = 0, w = 1,
    w = q - 1, a challenge equal to 1 and one equal to q - 1."""
    rnd = random.Random(seed)
    out = []
    for p in range(proofs):
        xs = [rnd.randrange(1, Q) for _ in range(k)]
        a, b, w = rnd.randrange(Q), rnd.randrange(Q), rnd.randrange(1, Q)
        if edges:
            if p % 5 == 0:
                a, w = 0, 1
            if p % 5 == 1:
                b, w = 0, Q - 1
            if k and p % 5 == 0:
                xs[0] = 1
            if k and p % 5 == 1:
                xs[-1] = Q - 1
            if k > 1 and p % 5 == 2:
                xs[k // 2] = Q - 1
                xs[k // 2 - 1] = 1
        out.append((xs, a, b, w))
    return out


def draw_scale(k, seed):
    rnd = random.Random(seed)
    sc = [rnd.randrange(Q) for _ in range(1 << k)]
    sc[0] = 1
    sc[-1] = 0 if k else sc[-1]
    return sc


def ss_ints(xs):
    """([s_i], [s_i^-1]) as plain integers, by the doubling of oracle.bp_ref.get_ss (the last challenge acts on the lowest index bit);
    one inversion per challenge.  tests/test_ipa_batch_host_cpu.py pins it to get_ss itself."""
    ss, si = [1], [1]
    for x in reversed(xs):
        xi = pow(x, -1, Q)
        ss, si = [s * xi % Q for s in ss] + [s * x % Q for s in ss], [s * x % Q for s in si] + [s * xi % Q for s in si]
    return ss, si


def ref_sums(k, proofs, scale=None):
    n = 1 << k
    sa, sb = [0] * n, [0] * n
    for xs, a, b, w in proofs:
        ss, si = ss_ints(xs)
        assert len(ss) == n
        wa, wb = w * a % Q, w * b % Q
        sa = [(v + wa * s) % Q for v, s in zip(sa, ss)]
        sb = [(v + wb * s) % Q for v, s in zip(sb, si)]
    if scale is not None:
        sb = [v * c % Q for v, c in zip(sb, scale)]
    return sa, sb


def ref_tables(k, proofs):
    """Per proof the records of its table: 2^kl pairs (s_lo, s_lo^-1) over the LAST kl challenges, then 2^kh pairs (w a s_hi, w b s_hi^-1)
    over the first kh -- s_i = s_hi s_lo for i = hi 2^kl + lo."""
    kl = k // 2
    kh = k - kl
    out = []
    for xs, a, b, w in proofs:
        (lo, loi), (hi, hii) = ss_ints(xs[kh:]), ss_ints(xs[:kh])
        tab = list(zip(lo, loi)) + [(w * a * s % Q, w * b * t % Q) for s, t in zip(hi, hii)]
        out.append(tab)
    return out
