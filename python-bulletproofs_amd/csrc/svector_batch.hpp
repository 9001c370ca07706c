// svector_batch.hpp -- part of libbpmi; plain C++ (host + device), also compiled for the host by tests/csrc_host.
// The per-thread bodies of the batch s-vector kernels (scalar_kernels.hpp: k_sc_svector_tables_batch, k_sc_svector_sum,
// k_sc_svector_sum_finish).  For proofs p = 0 .. P-1 over the same n = 2^k generators, with challenges x_{p,j}, final scalars
// a_p, b_p and random weights w_p (Verifier2's `a * s_i` / `b * s_i^-1` lists, /root/reference/src/innerproduct/inner_product_verifier.py
// :91-102 and :131-133, summed over the batch):
//   SA_i = sum_p w_p a_p s_{p,i},   SB_i = c_i sum_p w_p b_p s_{p,i}^-1,   s_{p,i} = prod_j x_{p,j}^(+1 if bit (k-1-j) of i is set else -1)
// As in k_sc_svector the index splits as i = hi 2^kl + lo, kl = k / 2: per proof a table of 2^kl records (s_lo, s_lo^-1) and 2^kh records
// (w a s_hi, w b s_hi^-1), 64 bytes each, so an element costs two multiplications per proof.
#pragma once
#include "scalar.hpp"

namespace bpmi {

BPMI_HD void svb_load8(u32 w[8], const u32 *p) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4 *q = reinterpret_cast<const uint4 *>(p);
#pragma unroll
  for (int i = 0; i < 2; i++) { const uint4 t = q[i]; w[4 * i] = t.x; w[4 * i + 1] = t.y; w[4 * i + 2] = t.z; w[4 * i + 3] = t.w; }
#else
  for (int i = 0; i < 8; i++) w[i] = p[i];
#endif
}
BPMI_HD void svb_store8(u32 *p, const u32 w[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint4 *q = reinterpret_cast<uint4 *>(p);
#pragma unroll
  for (int i = 0; i < 2; i++) q[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
#else
  for (int i = 0; i < 8; i++) p[i] = w[i];
#endif
}

// Record t of one proof's table.  rec: the proof's input record -- k pairs (x_j, x_j^-1) of 16 words, then a, b, w (8 words each, in [0, q)).
// t < 2^kl: (s_lo, s_lo^-1) of lo = t; else (w a s_hi, w b s_hi^-1) of hi = t - 2^kl.  The low half covers index bits [0, kl) = challenges
// j in [k - kl, k), the high half bits [kl, k) = j in [0, k - kl); MSB first inside each half: challenge j acts on bit k-1-j of i.
BPMI_HD void svb_table_entry(u32 out[16], const u32 *rec, u32 k, u32 kl, u32 t) {
  const u32 nlo = 1u << kl;
  const bool is_hi = t >= nlo;
  const u32 idx = is_hi ? t - nlo : t;
  sc f, g;                        // f -> s, g -> s^-1
#pragma unroll
  for (int q = 0; q < 8; q++) f.v[q] = g.v[q] = q == 0 ? 1u : 0u;
  if (is_hi) {
    sc a, b, w;
    svb_load8(a.v, rec + 16ull * k);
    svb_load8(b.v, rec + 16ull * k + 8);
    svb_load8(w.v, rec + 16ull * k + 16);
    sc_mul(f, w, a);
    sc_mul(g, w, b);
  }
  const u32 j0 = is_hi ? 0u : k - kl, j1 = is_hi ? k - kl : k;
  const u32 width = j1 - j0;
  for (u32 j = j0; j < j1; j++) {
    const u32 bit = (idx >> (width - 1u - (j - j0))) & 1u;
    sc x, xi;
    svb_load8(x.v, rec + 16ull * j);
    svb_load8(xi.v, rec + 16ull * j + 8);
    sc_mul(f, f, bit ? x : xi);
    sc_mul(g, g, bit ? xi : x);
  }
#pragma unroll
  for (int q = 0; q < 8; q++) { out[q] = f.v[q]; out[8 + q] = g.v[q]; }
}

// Element i over the proofs [p0, p1): A = sum_p fl_p[lo] fh_p[hi], B = sum_p gl_p[lo] gh_p[hi]  (tabs: tab_entries records of 16 words
// per proof).  The products run on 9 x 29-bit limbs (sq_mul: 156 multiply-adds against sc_mul's ~720 instructions) and the sums stay
// in the loose form sq_add returns -- it accepts loose operands, so no sum is ever reduced to [0, q) inside the loop -- ; the one
// canonical reduction per output is sq_to_sc here at the end.  Access pattern: the 64 lanes of a wave read 64 consecutive lo
// records (4 KB, every byte used) and, from 2^kl >= 64, ONE hi record (the same address in every lane: one 64-byte request).
BPMI_HD void svb_sum_element(u32 out_a[8], u32 out_b[8], const u32 *tabs, uint64_t tab_entries, u32 kl, u32 i, u32 p0, u32 p1) {
  const u32 nlo = 1u << kl;
  const u32 lo = i & (nlo - 1u), hi = i >> kl;
  const u32 *rl = tabs + 16ull * (tab_entries * p0 + lo), *rh = tabs + 16ull * (tab_entries * p0 + nlo + hi);
  sq A = sq_small(0), B = sq_small(0);
  for (u32 p = p0; p < p1; p++) {
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
    rl += 16ull * tab_entries; rh += 16ull * tab_entries;
  }
  sc ra, rb;
  sq_to_sc(ra, A);
  sq_to_sc(rb, B);
#pragma unroll
  for (int q = 0; q < 8; q++) { out_a[q] = ra.v[q]; out_b[q] = rb.v[q]; }
}

// Element i: the sums of the `parts` ranges (part j: n values of A, then n values of B, canonical), SB times the shared scale c_i
// -- once per element, not once per proof.
BPMI_HD void svb_finish_element(u32 out_a[8], u32 out_b[8], const u32 *part, u32 parts, uint64_t n, const u32 *scale, u32 i) {
  sc A, B, t;
  svb_load8(A.v, part + 8ull * i);
  svb_load8(B.v, part + 8ull * (n + i));
  for (u32 j = 1; j < parts; j++) {
    const u32 *pj = part + 16ull * n * j;
    svb_load8(t.v, pj + 8ull * i); sc_add(A, A, t);
    svb_load8(t.v, pj + 8ull * (n + i)); sc_add(B, B, t);
  }
  if (scale) {
    svb_load8(t.v, scale + 8ull * i);
    sc_mul(B, B, t);
  }
#pragma unroll
  for (int q = 0; q < 8; q++) { out_a[q] = A.v[q]; out_b[q] = B.v[q]; }
}

// Element i of GROUP t (bpmi_ipa_group_values_packed_dev): svb_sum_element over the group's proofs [t group, min((t + 1) group, n_proofs)),
// then SB times the shared scale c_i (or scale == null).  Canonical output: these are the scalars of row t of the groups' MSMs.
BPMI_HD void svb_group_element(u32 out_a[8], u32 out_b[8], const u32 *tabs, uint64_t tab_entries, u32 kl, u32 i, u32 t, u32 group, u32 n_proofs,
                               const u32 *scale) {
  const u32 p0 = t * group;
  const u32 p1 = n_proofs - p0 < group ? n_proofs : p0 + group;
  svb_sum_element(out_a, out_b, tabs, tab_entries, kl, i, p0, p1);
  if (scale) {
    sc B, c;
#pragma unroll
    for (int q = 0; q < 8; q++) B.v[q] = out_b[q];
    svb_load8(c.v, scale + 8ull * i);
    sc_mul(B, B, c);
#pragma unroll
    for (int q = 0; q < 8; q++) out_b[q] = B.v[q];
  }
}

}  // namespace bpmi
