// ipa_prove_kernels.hpp -- part of libbpmi (included by bpmi.hip; one translation unit).  DEVICE code.
// A BATCH of inner-product arguments over ONE generator set (g, h of n <= 1 024 points, one u), proved on the GPU from the caller's
// vectors to the proofs' fields.  It replaces a loop of NIProver.prove (src/innerproduct/inner_product_prover.py:11-45) or
// FastNIProver2.prove (:48-110): the same transcripts (src/utils/transcript.py:13-33), the same challenges (mod_hash,
// src/utils/utils.py:84-97), the same proof, byte for byte (tests/test_gpu_ipa_prove_batch.py compares every field with
// the single-proof provers').
//
// The machinery is the Protocol-2 phase of the batched range prover (rp_prove_kernels.hpp, namespace rpp), used as it is: the
// fixed-base tables and their builders, k_pv_msm over base lists, k_pv_affine, the transcript text (put_point, put_number) and
// mod_hash_q.  The rounds never fold a generator: L and R are sums over the ORIGINAL generators with the fold coefficients cg / hf
// in the scalars.  What differs from the range prover, and why these kernels are variants of k_pv_round_wide / k_pv_round_chal
// rather than those kernels (which stay untouched, with their resource lines):
//   * the vectors a, b come from the caller, not from a range proof's algebra (k_ip_round_wide, first call);
//   * Protocol 1 has a challenge PER PROOF, x_p = mod_hash(base64(seed_p) "&") (:30): the u term of every L and R carries uc_p = x_p
//     (1 under Protocol 2) where the range prover has one constant x_ip per batch (its Protocol-1 seed is always empty);
//   * the statement point P_p is no fixed base: P_new = P_p + (x_p c_p) u is one complete mixed addition behind a one-term job (k_ip_head);
//   * the points of a proof are u_new, P_new (`head`) and L_0.. R_0.. (`lr`), two arrays in the order the caller receives them.
// Every kernel's body is a __device__ function of (record, block index), ip_*_block, which the kernel calls with blockIdx.x and its
// `_mixed` twin (ipa_prove_mixed_kernels.hpp: classes of different lengths in one launch) with the block's index inside its class.
// Hoisting the bodies moved no kernel's registers, scratch, LDS or occupancy (profiles/r22_ipa_prove_mixed_resources.txt).
#pragma once

namespace ipp {

using rpp::sc;
using rpp::u8;
using rpp::mulq;
using rpp::addq;
using rpp::invq;
using rpp::sc_u32;
using rpp::ld_sc;
using rpp::st_sc;
using bpmi::u32;
using bpmi::affine;
using bpmi::xyzz;

// Device arrays of one batch (P proofs of n elements, k = log2 n).  Scalars: 8 words little-endian.  Points: 16 words (x, y) little-endian.
struct Batch {
  u32 P, n, k, proto;
  const u8 *dig0; u32 dig0_stride; const u32 *dig0_len;        // the transcript's start as the host staged it: base64(seed) "&" (Protocol 1), "&" prefix (Protocol 2)
  const u32 *a_in, *b_in;    // P x n scalars: the caller's vectors
  const u32 *c_in;           // P scalars, or nullptr: c_p = <a_p, b_p>         (Protocol 1)
  const u32 *P_in;           // P points                                        (Protocol 1)
  const u32 *hscale;         // n scalars, or nullptr: the argument runs over hscale_j h_j (the initial hf_j)
  u8 *tr; u32 tr_stride; u32 *tr_len;                          // the Protocol-2 transcript of every proof
  u32 *uc;                   // P: the coefficient of u in every L and R: x_p, or 1
  u32 *hsc;                  // 2P: the scalars of the head's one-term jobs over u: x_p (u_new), x_p c_p (P_new - P_p)
  u32 *xs;                   // P x k
  u32 *xr;                   // P x 2: the current round's challenge and its inverse
  u32 *a, *b, *cg, *hf;      // P x n each: the state (cg / hf: coefficient of g_j / h_j in the folded generators)
  u32 *jsc;                  // job scalars: 2P x (n + 1) (the L / R of a round)
  u32 *jout;                 // job results, XYZZ: 2P x 36 words
  u32 *head;                 // P x 2 affine points: u_new, P_new
  u32 *lr;                   // P x 2k affine points: L_0.. R_0..
  u32 *ab;                   // P x 2: the proof's scalars
};

// ---- the transcript's start, one lane per proof (inner_product_prover.py:30-31, :58-63) ----------------------------------------------------
// Protocol 1: the outer transcript is base64(seed) "&"; x = mod_hash of it; the inner transcript is "&" || outer || str(x) "&".
// Protocol 2: the inner transcript is "&" || the caller's prefix, staged whole.
__device__ __forceinline__ void ip_begin_block(const Batch &B, const u32 blk) {
  const u32 p = blk * blockDim.x + threadIdx.x;
  if (p >= B.P) return;
  u8 *tr = B.tr + (size_t)p * B.tr_stride;
  const u8 *dg = B.dig0 + (size_t)p * B.dig0_stride;
  const u32 dl = B.dig0_len[p];
  if (B.proto == 1u) {
    tr[0] = '&';
    for (u32 i = 0; i < dl; i++) tr[1u + i] = dg[i];
    const sc x = rpp::mod_hash_q(0, 0, dg, dl);
    u32 len = 1u + dl;
    len += rpp::put_number(tr + len, x);
    B.tr_len[p] = len;
    st_sc(B.uc + 8ull * p, x);
    st_sc(B.hsc + 16ull * p, x);
    if (B.c_in) st_sc(B.hsc + 16ull * p + 8, mulq(x, ld_sc(B.c_in + 8ull * p)));      // (c NULL: k_ip_round_wide's first call writes x <a, b>)
  } else {
    for (u32 i = 0; i < dl; i++) tr[i] = dg[i];
    B.tr_len[p] = dl;
    st_sc(B.uc + 8ull * p, sc_u32(1));
  }
}
__global__ void __launch_bounds__(64) k_ip_begin(Batch B) { ip_begin_block(B, blockIdx.x); }

// ---- the head of a Protocol-1 proof (:32-33): job 2p = x_p u is u_new; job 2p + 1 = (x_p c_p) u, and P_new = P_p + it -- a complete
// mixed addition: P_p may be the identity, the opposite of the job's result (P_new is the identity) or equal to it (a doubling)
__device__ __forceinline__ void ip_head_block(const Batch &B, const u32 blk) {
  const u32 t = blk * blockDim.x + threadIdx.x;
  if (t >= 2u * B.P) return;
  xyzz acc;
  ::xyzz_load_g(acc, B.jout + 36ull * t);
  if (t & 1u) {
    affine Pp;
    ::load_affine(Pp, B.P_in + 16ull * (t >> 1));
    bpmi::xyzz_madd_signed(acc, Pp, false);
  }
  affine r;
  bpmi::xyzz_to_affine(r, acc);
  u32 w[16];
  bpmi::affine_to_words(w, r);
  ::store_words16(B.head + 16ull * t, w);
}
__global__ void __launch_bounds__(256) k_ip_head(Batch B) { ip_head_block(B, blockIdx.x); }

// ---- one round (:94-110) over the UNFOLDED generators: see rp_prove_kernels.hpp, "one round of Protocol 2".  Job 2p is L, job 2p + 1 is
// R, n + 1 terms each in the base order of ipp_plan:
//   L = sum a_(i-half) cg_j g_j + sum b_(i+half) hf_j h_j + (uc_p c_L) u,   i = j mod len
// L, R -> transcript -> x, 1 / x (:100-106); k_pv_round_chal with this layout's points
__device__ __forceinline__ void ip_round_chal_block(const Batch &B, const u32 round, const u32 blk) {
  const u32 p = blk * blockDim.x + threadIdx.x;
  if (p >= B.P) return;
  u8 *tr = B.tr + (size_t)p * B.tr_stride;
  u32 tl = B.tr_len[p];
  const u32 *pt = B.lr + 16ull * (size_t)p * (2u * B.k);
  tl += rpp::put_point(tr + tl, pt + 16u * round);
  tl += rpp::put_point(tr + tl, pt + 16u * (B.k + round));
  const sc x = rpp::mod_hash_q(0, 0, tr, tl);
  tl += rpp::put_number(tr + tl, x);
  B.tr_len[p] = tl;
  st_sc(B.xs + 8ull * ((size_t)p * B.k + round), x);
  st_sc(B.xr + 16ull * p, x);
  st_sc(B.xr + 16ull * p + 8, invq(x));
}
__global__ void __launch_bounds__(64) k_ip_round_chal(Batch B, u32 round) { ip_round_chal_block(B, round, blockIdx.x); }
// n lanes per proof (block = NT threads = NT / n proofs; NT = 1024: 4 x 32 KB of LDS, a block per CU).  first = 1: the state is loaded
// from the caller's vectors with cg = 1, hf = hscale_j or 1, and under Protocol 1 without c the head's scalar x_p <a_p, b_p> is summed
// over the proof's lanes; else the state is folded with the challenge of `round` (:107-110).  Either way the scalars of the NEXT
// round's L and R are written, as k_pv_round_wide writes them with uc_p in the place of x_ip.  After the last fold (or at once, for
// n = 1) a[0], b[0] are the proof's scalars.
template <u32 NT> __device__ __forceinline__ void ip_round_wide_block(const Batch &B, const u32 round, const u32 first, const u32 blk) {
  __shared__ u32 s_a[NT * 8], s_b[NT * 8], s_l[NT * 8], s_r[NT * 8];
  const u32 n = B.n, tid = threadIdx.x;
  const u32 p = blk * (NT / n) + tid / n, j = tid & (n - 1u);
  const bool live = p < B.P;
  const u32 base = tid - j;                                  // first thread of this proof in the block
  u32 len = first ? n : (n >> round);                        // length BEFORE this call's fold
  sc cgj = sc_u32(0), hfj = sc_u32(0);
  if (live) {
    const size_t e = (size_t)p * n + j;
    u32 *a = B.a + 8ull * (size_t)p * n, *b = B.b + 8ull * (size_t)p * n;
    if (first) {
      const sc aj = ld_sc(B.a_in + 8ull * e), bj = ld_sc(B.b_in + 8ull * e);
      cgj = sc_u32(1); hfj = B.hscale ? ld_sc(B.hscale + 8ull * j) : sc_u32(1);
      st_sc(s_a + 8u * tid, aj); st_sc(s_b + 8u * tid, bj);
      st_sc(a + 8ull * j, aj); st_sc(b + 8ull * j, bj);
      st_sc(B.cg + 8ull * e, cgj); st_sc(B.hf + 8ull * e, hfj);
    } else {
      cgj = ld_sc(B.cg + 8ull * e); hfj = ld_sc(B.hf + 8ull * e);
      const u32 half = len >> 1;
      const sc x = ld_sc(B.xr + 16ull * p), xi = ld_sc(B.xr + 16ull * p + 8);
      if (j < half) {
        const sc a0 = ld_sc(a + 8ull * j), a1 = ld_sc(a + 8ull * (half + j)), b0 = ld_sc(b + 8ull * j), b1 = ld_sc(b + 8ull * (half + j));
        const sc an = addq(mulq(x, a0), mulq(xi, a1)), bn = addq(mulq(xi, b0), mulq(x, b1));
        st_sc(s_a + 8u * tid, an); st_sc(s_b + 8u * tid, bn);
      }
      const bool low = (j & (len - 1u)) < half;
      cgj = mulq(cgj, low ? xi : x); hfj = mulq(hfj, low ? x : xi);
      st_sc(B.cg + 8ull * e, cgj); st_sc(B.hf + 8ull * e, hfj);
      len = half;
    }
  }
  __syncthreads();                                           // s_a / s_b [base + i], i < len: the state
  if (live && !first && j < len) {                           // (the folded halves go back in place: nobody reads the old ones any more)
    st_sc(B.a + 8ull * ((size_t)p * n + j), ld_sc(s_a + 8u * tid));
    st_sc(B.b + 8ull * ((size_t)p * n + j), ld_sc(s_b + 8u * tid));
  }
  if (first && B.proto == 1u && !B.c_in) {                   // (block-uniform) c_p = <a_p, b_p>: the head's scalar x_p c_p
    st_sc(s_l + 8u * tid, live ? mulq(ld_sc(s_a + 8u * tid), ld_sc(s_b + 8u * tid)) : sc_u32(0));
    __syncthreads();
    for (u32 d = n >> 1; d > 0u; d >>= 1) {
      if (j < d) st_sc(s_l + 8u * tid, addq(ld_sc(s_l + 8u * tid), ld_sc(s_l + 8u * (tid + d))));
      __syncthreads();
    }
    if (live && j == 0u) st_sc(B.hsc + 16ull * p + 8, mulq(ld_sc(B.uc + 8ull * p), ld_sc(s_l + 8u * tid)));
    __syncthreads();                                         // (s_l is written again below)
  }
  if (len == 1u) {
    if (live && j == 0u) { st_sc(B.ab + 16ull * p, ld_sc(s_a + 8u * tid)); st_sc(B.ab + 16ull * p + 8, ld_sc(s_b + 8u * tid)); }
    return;                                                  // (block-uniform: len depends on the arguments only)
  }
  const u32 half = len >> 1, i = j & (len - 1u);
  // the products of c_L = <a_lo, b_hi>, c_R = <a_hi, b_lo>, summed over the proof's lanes in LDS
  sc pl = sc_u32(0), pr = sc_u32(0);
  if (live && j < half) {
    pl = mulq(ld_sc(s_a + 8u * (base + j)), ld_sc(s_b + 8u * (base + half + j)));
    pr = mulq(ld_sc(s_a + 8u * (base + half + j)), ld_sc(s_b + 8u * (base + j)));
  }
  st_sc(s_l + 8u * tid, pl); st_sc(s_r + 8u * tid, pr);
  __syncthreads();
  for (u32 d = n >> 1; d > 0u; d >>= 1) {
    if (j < d) {
      st_sc(s_l + 8u * tid, addq(ld_sc(s_l + 8u * tid), ld_sc(s_l + 8u * (tid + d))));
      st_sc(s_r + 8u * tid, addq(ld_sc(s_r + 8u * tid), ld_sc(s_r + 8u * (tid + d))));
    }
    __syncthreads();
  }
  if (!live) return;
  u32 *jl = B.jsc + 8ull * (size_t)(2u * p) * (n + 1u), *jr = jl + 8ull * (n + 1u);
  if (j == 0u) {
    const sc uc = ld_sc(B.uc + 8ull * p);
    st_sc(jl + 8ull * n, mulq(uc, ld_sc(s_l + 8u * tid))); st_sc(jr + 8ull * n, mulq(uc, ld_sc(s_r + 8u * tid)));
  }
  // generator j: rank among the generators of its side of the split = (j / len) half + (i mod half)
  const bool up = i >= half;
  const u32 rank = (j / len) * half + (up ? i - half : i);
  const sc ga = ld_sc(s_a + 8u * (base + (up ? i - half : i + half))), hb = ld_sc(s_b + 8u * (base + (up ? i - half : i + half)));
  st_sc((up ? jl : jr) + 8ull * rank, mulq(ga, cgj));                       // L: a_(i-half) cg_j for i >= half; R: a_(i+half) cg_j for i < half
  st_sc((up ? jr : jl) + 8ull * ((n >> 1) + rank), mulq(hb, hfj));          // L: b_(i+half) hf_j for i < half; R: b_(i-half) hf_j for i >= half
}
template <u32 NT> __global__ void __launch_bounds__(NT) k_ip_round_wide(Batch B, u32 round, u32 first) { ip_round_wide_block<NT>(B, round, first, blockIdx.x); }

// ---- the statements of a batch (bpmi_ipa_batch_prover_commit_batch): P_p = sum a_p[j] g_j + sum b_p[j] (c_j h_j) + t_p u, a loop of
// vector_commitment(g, h, a_p, b_p) (src/utils/commitments.py:13) plus inner_product(a, b) * u.  This kernel only lays out the scalars:
// job p of k_pv_msm over the base list of ipp_commit_bases takes the row [a_p | b_p c_j | t_p] of T terms (a NULL half is left out,
// u_mode 0 has no t_p); the points come from the prover's tables.
struct Commit {
  u32 count, n, T;
  u32 u_mode;                // 0: no u term; 1: t_p = <a_p, b_p> over the UNSCALED b, summed here; 2: t_p = t_in[p]
  const u32 *a_in, *b_in;    // count x n scalars each; one of them may be nullptr
  const u32 *t_in;           // count scalars (u_mode 2)
  const u32 *hscale;         // n scalars c_j, or nullptr
  u32 *jsc;                  // count x T
};
__device__ __forceinline__ sc sc_shfl_xor(const sc &a, int mask) {
  sc r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = (u32)__shfl_xor((int)a.v[i], mask, 64);
  return r;
}
// n lanes per proof in blocks of NT (the plan's rule: a proof never straddles a block; n <= 64 divides a wave).  The branches on u_mode,
// the NULL halves and n are uniform over the launch, so every lane of a block -- those of proofs beyond `count` in the last block
// included, which carry zeros -- reaches every shuffle and the barrier.  The dot of u_mode 1: a butterfly of shuffles over the
// min(n, 64) lanes a proof has in a wave; for n > 64 the n / 64 wave sums meet in LDS and the proof's first wave adds them with the
// same butterfly.
template <u32 NT> __device__ __forceinline__ void ip_commit_scalars_block(const Commit &C, const u32 blk) {
  __shared__ u32 s_w[(NT / 64u) * 8u];
  const u32 n = C.n, tid = threadIdx.x;
  const u32 p = blk * (NT / n) + tid / n, j = tid & (n - 1u);
  const bool live = p < C.count;
  const size_t e = (size_t)p * n + j;
  u32 *row = C.jsc + 8ull * (size_t)p * C.T;
  const u32 off_b = C.a_in ? n : 0u, off_t = off_b + (C.b_in ? n : 0u);
  sc aj = sc_u32(0), bj = sc_u32(0);
  if (live) {
    if (C.a_in) { aj = ld_sc(C.a_in + 8ull * e); st_sc(row + 8ull * j, aj); }
    if (C.b_in) { bj = ld_sc(C.b_in + 8ull * e); st_sc(row + 8ull * (off_b + j), C.hscale ? mulq(bj, ld_sc(C.hscale + 8ull * j)) : bj); }
  }
  if (C.u_mode == 2u) {
    if (live && j == 0u) st_sc(row + 8ull * off_t, ld_sc(C.t_in + 8ull * p));
    return;
  }
  if (C.u_mode != 1u) return;
  sc acc = mulq(aj, bj);                                     // (a dead lane: 0 x 0)
  const u32 in_wave = n < 64u ? n : 64u;
  for (u32 d = 1; d < in_wave; d <<= 1) acc = addq(acc, sc_shfl_xor(acc, (int)d));
  if (n > 64u) {
    const u32 wave = tid >> 6, waves = n >> 6;               // waves per proof: 2 .. 16
    if ((tid & 63u) == 0u) st_sc(s_w + 8u * wave, acc);
    __syncthreads();
    acc = j < waves ? ld_sc(s_w + 8u * ((tid - j) / 64u + j)) : sc_u32(0);
    for (u32 d = 1; d < waves; d <<= 1) acc = addq(acc, sc_shfl_xor(acc, (int)d));
  }
  if (live && j == 0u) st_sc(row + 8ull * off_t, acc);
}
template <u32 NT> __global__ void __launch_bounds__(NT) k_ip_commit_scalars(Commit C) { ip_commit_scalars_block<NT>(C, blockIdx.x); }

}  // namespace ipp
