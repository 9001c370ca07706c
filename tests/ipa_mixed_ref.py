"""Python-integer reference of the s-vector sums of a batch of proofs of DIFFERENT lengths (bpmi_sc_svector_sum_mixed), shared by the CPU
test of the host-built kernel bodies and the GPU test of the kernels: proof p of 2^ks[p] elements contributes ipa_batch_ref.ref_sums of
itself alone to the first 2^ks[p] elements,
    SA_i = sum_{p : n_p > i} w_p a_p s_{p,i},   SB_i = c_i sum_{p : n_p > i} w_p b_p s_{p,i}^-1,   i < n_top = max n_p."""
from ipa_batch_ref import Q, draw_proofs, draw_scale, ref_sums

# the length lists of the tests, the caller's order as written: n_top = 1 | unsorted, kl = 0 and odd k | a wave boundary | a block
# boundary | one long and many short (block 0 has several units and its lanes diverge, the other block has one proof) | a 64-record
# half table and a last range shorter than the others | one length, many proofs | one length (the capacity is above n_top)
LENGTH_LISTS = [[0, 0, 0], [3, 0, 1, 3, 2], [6] * 3 + [5] * 2, [8, 7, 9, 8], [9] + [2] * 200, [13] * 2 + [6] * 130, [5] * 64, [7] * 3]
# Every list above has at most 1 024 (proof, wave) pairs, so its ranges hold ONE proof and no block is alone with one unit.  Beyond them:
# 2 056 pairs -- ranges of three proofs, a last range of one, and the range [2049, 2052) cut at 2 051 by the lanes of elements 8 .. 63 | one
# proof: one unit, which writes SA / SB itself | 2 049 pairs over two proofs: every block has one unit of both, the lanes of block 0
# clip it, and without a scale the kernel writes SA / SB itself
MORE_LISTS = [[6] * 2051 + [3] * 5, [4], [17, 3]]


def n_gens_of(ks):
    """The capacity a list is tested under: its own n_top, and 2^10 for [7] * 3."""
    return 1 << 10 if ks == [7] * 3 else 1 << max(ks)


def draw_mixed(ks, seed, edges=True):
    """One tuple (xs, a, b, w) per proof with len(xs) = ks[p], from draw_proofs of every length: its edge values (a = 0 and w = 1 | b = 0
    and w = q - 1 | x = 1 and x = q - 1 | none | none, in turn) fall on the first proofs of each length.  A length with ONE proof starts
    two places further on per rank among the lengths, so that single proofs do not all get a = 0."""
    by_k = {}
    for rank, k in enumerate(sorted(set(ks))):
        skip = 2 * rank % 5 if ks.count(k) == 1 else 0
        by_k[k] = iter(draw_proofs(k, skip + ks.count(k), seed + 97 * k, edges)[skip:])
    return [next(by_k[k]) for k in ks]


def draw_scale_mixed(ks, n_gens, seed):
    """n_gens integers c_i: draw_scale over the n_top elements that are read (c_0 = 1, c_(n_top - 1) = 0), then values that are not."""
    import random
    k_top = max(ks)
    rnd = random.Random(seed + 1)
    return draw_scale(k_top, seed) + [rnd.randrange(Q) for _ in range(n_gens - (1 << k_top))]


def ref_sums_mixed(ks, proofs, scale=None):
    """(SA, SB) over n_top = 2^max(ks) elements; scale: at least n_top integers c_i, or None."""
    assert len(ks) == len(proofs) and all(len(p[0]) == k for k, p in zip(ks, proofs))
    n_top = 1 << max(ks)
    sa, sb = [0] * n_top, [0] * n_top
    for k, proof in zip(ks, proofs):
        pa, pb = ref_sums(k, [proof])
        for i in range(1 << k):
            sa[i] = (sa[i] + pa[i]) % Q
            sb[i] = (sb[i] + pb[i]) % Q
    if scale is not None:
        sb = [v * c % Q for v, c in zip(sb, scale)]
    return sa, sb


__all__ = ["Q", "LENGTH_LISTS", "MORE_LISTS", "n_gens_of", "draw_mixed", "draw_scale_mixed", "ref_sums_mixed"]
