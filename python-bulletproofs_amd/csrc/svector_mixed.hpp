// svector_mixed.hpp -- part of libbpmi; plain C++ (host + device), also compiled for the host by tests/csrc_host.
// The per-thread bodies of the s-vector kernels of a batch of proofs of DIFFERENT lengths (ipa_mixed_kernels.hpp:
// k_sc_svector_tables_mixed, k_sc_svector_sum_mixed, k_sc_svector_sum_finish_mixed).  Proof p has n_p = 2^k_p elements over the first
// n_p generators of one list, with its own k_p challenges (Verifier2.get_ss, src/innerproduct/inner_product_verifier.py:91-102 of the
// reference; MSB first over k_p bits), so generator i collects the proofs that reach it:
//   SA_i = sum_{p : n_p > i} w_p a_p s_{p,i},   SB_i = c_i sum_{p : n_p > i} w_p b_p s_{p,i}^-1,   i < n_top = max_p n_p
// The proofs are sorted by descending k_p: those that cover element i are the prefix [0, C[bitlen(i)]).  Each proof has the half
// tables of svector_batch.hpp for its own (k, kl) -- svb_table_entry unchanged -- at its own offset of one packed array; the layout
// of the descriptors, units and partial sums is ipa_mixed_plan_host.hpp.
#pragma once
#include "svector_batch.hpp"

namespace bpmi {

// a value that is the same in every lane of the wave, told to the compiler: what is indexed with it is read by scalar loads
#if defined(__HIP_DEVICE_COMPILE__)
#define SVM_UNIFORM(x) ((u32)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define SVM_UNIFORM(x) ((u32)(x))
#endif

BPMI_HD u32 svm_bitlen(u32 i) { return i ? 32u - (u32)__builtin_clz(i) : 0u; }

// The proof (sorted position) that record r of the packed table array belongs to: the last s with desc[4 s] <= r.  desc: 4 words per
// proof (offset of its table in records, k, kl, offset of its input record in recs, in words); the offsets rise strictly.
BPMI_HD u32 svm_proof_of_record(const u32 *desc, u32 n_proofs, u32 r) {
  u32 lo = 0, hi = n_proofs;
  while (hi - lo > 1u) {
    const u32 mid = lo + (hi - lo) / 2u;
    if (desc[4ull * mid] <= r) lo = mid; else hi = mid;
  }
  return lo;
}
// Record r of the packed table array, r < the sum of the proofs' 2^kl + 2^kh: record r - offset of its proof's own table, from that
// proof's input record (its own k pairs (x_j, x_j^-1), then a, b, w) -- svb_table_entry with the proof's own (k, kl).
BPMI_HD void svm_table_record(u32 out[16], const u32 *recs, const u32 *desc, u32 n_proofs, u32 r) {
  const u32 *d = desc + 4ull * svm_proof_of_record(desc, n_proofs, r);
  svb_table_entry(out, recs + d[3], d[1], d[2], r - d[0]);
}

// Element i over the proofs [p0, p1) of a unit, clipped to those that cover it: [p0, min(p1, C[bitlen(i)])).  The loop runs to the
// bound of the wave's FIRST element (C falls with the bit length, so that is the largest of the wave) and is wave-uniform: the proof's
// table offset and kl come from the descriptor as scalar loads, the next proof's one iteration ahead; a lane beyond its own bound
// skips the proof -- it neither loads nor multiplies.  Only the wave of elements 0 .. 63 has lanes with different bounds.  The sums
// are those of svb_sum_element: loose sq, one sq_to_sc per output; an empty range gives zeros.
BPMI_HD void svm_sum_element(u32 out_a[8], u32 out_b[8], const u32 *tabs, const u32 *desc, const u32 *C, u32 i, u32 p0, u32 p1) {
  const u32 c_lane = C[svm_bitlen(i)], c_wave = C[svm_bitlen(i & ~63u)];
  const u32 lane_p1 = c_lane < p1 ? c_lane : p1;
  const u32 wave_p1 = SVM_UNIFORM(c_wave < p1 ? c_wave : p1);
  sq A = sq_small(0), B = sq_small(0);
  u32 off = 0, kl = 0;
  if (p0 < wave_p1) { off = SVM_UNIFORM(desc[4ull * p0]); kl = SVM_UNIFORM(desc[4ull * p0 + 2]); }
  for (u32 p = p0; p < wave_p1; p++) {
    const u32 nlo = 1u << kl;
    const u32 *rl = tabs + 16ull * ((uint64_t)off + (i & (nlo - 1u))), *rh = tabs + 16ull * ((uint64_t)off + nlo + (i >> kl));
    const bool mine = p < lane_p1;
    if (p + 1 < wave_p1) { off = SVM_UNIFORM(desc[4ull * (p + 1)]); kl = SVM_UNIFORM(desc[4ull * (p + 1) + 2]); }
    if (mine) {
      sc t;
      sq fl, fh, gl, gh, m;
      svb_load8(t.v, rl); sq_from_sc(fl, t);
      svb_load8(t.v, rh); sq_from_sc(fh, t);
      sq_mul(m, fl, fh);
      sq_add(A, A, m);
      svb_load8(t.v, rl + 8); sq_from_sc(gl, t);
      svb_load8(t.v, rh + 8); sq_from_sc(gh, t);
      sq_mul(m, gl, gh);
      sq_add(B, B, m);
    }
  }
  sc ra, rb;
  sq_to_sc(ra, A);
  sq_to_sc(rb, B);
#pragma unroll
  for (int q = 0; q < 8; q++) { out_a[q] = ra.v[q]; out_b[q] = rb.v[q]; }
}

// Element i: the partial sums of the units [block_first[e], block_first[e + 1]) of its block e = i / 256 (slot u: 256 values of A, then
// 256 of B, canonical; every lane below n_top wrote its own, zeros where no proof of the unit covered it), SB times the shared scale c_i.
BPMI_HD void svm_finish_element(u32 out_a[8], u32 out_b[8], const u32 *part, const u32 *block_first, const u32 *scale, u32 i) {
  const u32 e = i >> 8, lane = i & 255u;
  const u32 u0 = block_first[e], u1 = block_first[e + 1];
  sc A, B, t;
  svb_load8(A.v, part + 4096ull * u0 + 8ull * lane);
  svb_load8(B.v, part + 4096ull * u0 + 8ull * (256u + lane));
  for (u32 u = u0 + 1; u < u1; u++) {
    svb_load8(t.v, part + 4096ull * u + 8ull * lane); sc_add(A, A, t);
    svb_load8(t.v, part + 4096ull * u + 8ull * (256u + lane)); sc_add(B, B, t);
  }
  if (scale) {
    svb_load8(t.v, scale + 8ull * i);
    sc_mul(B, B, t);
  }
#pragma unroll
  for (int q = 0; q < 8; q++) { out_a[q] = A.v[q]; out_b[q] = B.v[q]; }
}

// Lane `lane` of block `block` of k_sc_svector_sum_groups_mixed (bpmi_ipa_group_values_packed_mixed_dev; ipa_group_mixed_plan_host.hpp):
// the rows of every class's groups in one launch.  ctab: 8 words per class that has groups, in rising order of the block start -- block
// start, row offset in scalars (256 block start), k, kl, table base and stride in records, proofs, group.  The block belongs to the last
// class whose block start is <= block: a scan of at most 64 entries with the block's index, the same in every lane, so the entries
// come by scalar loads and the class's eight words stay in scalar registers.  local = 256 (block - block start) + lane is the flat
// (group, element) index of k_sc_svector_sum_groups inside the class: t = local >> k, i = local & (n - 1) -- for n < 64 several groups
// share a wave.  Returns false for a pad lane (t beyond the class's groups), which writes nothing; else the two scalars of
// svb_group_element over the class's own tables, and idx = row offset + local, the scalar they belong to in rows SA / rows SB.
BPMI_HD bool svm_group_row_element(u32 out_a[8], u32 out_b[8], u32 &idx, const u32 *tabs, const u32 *ctab, u32 n_cls, const u32 *scale, u32 block, u32 lane) {
  const u32 b = SVM_UNIFORM(block);
  u32 c = 0;
  for (u32 j = 1; j < n_cls; j++)
    if (SVM_UNIFORM(ctab[8ull * j]) <= b) c = j;
  const u32 *d = ctab + 8ull * c;
  const u32 start = SVM_UNIFORM(d[0]), row_off = SVM_UNIFORM(d[1]), k = SVM_UNIFORM(d[2]), kl = SVM_UNIFORM(d[3]);
  const u32 base = SVM_UNIFORM(d[4]), stride = SVM_UNIFORM(d[5]), count = SVM_UNIFORM(d[6]), group = SVM_UNIFORM(d[7]);
  const u32 local = (b - start) * 256u + lane;
  const u32 t = local >> k, i = local & ((1u << k) - 1u);
  const u32 ngroups = (count + group - 1u) / group;
  if (t >= ngroups) return false;
  svb_group_element(out_a, out_b, tabs + 16ull * base, stride, kl, i, t, group, count, scale);
  idx = row_off + local;
  return true;
}

}  // namespace bpmi
