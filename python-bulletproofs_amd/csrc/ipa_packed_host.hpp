// ipa_packed_host.hpp -- part of libbpmi; plain C++17 over namespace rp of rp_batch_host.hpp (no HIP), also compiled for the host by
// tests/csrc_host.  The per-proof preparation of the batch verifier of PACKED inner-product proofs -- the arrays
// bpmi_ipa_prove_batch writes -- as host code: the native twin of the kernels of ipa_packed_kernels.hpp (same checks, same bytes:
// tests/test_gpu_ipa_packed.py compares the two) and the specification both are tested against
// (tests/test_ipa_packed_host_cpu.py: Python integers and the single-proof oracle verifiers).
//
// What is checked per proof (reference call sites in brackets), bit 0 of its status:
//   a, b, c, xs[j] < q                       (conventions of this ABI)
//   Protocol 1   items 1, 2 exist and item 2 == str(mod_hash(item 1 + "&", q))          (inner_product_verifier.py:36-42)
//   Protocol 2   per round i: items s+3i, s+3i+1 are base64(SEC1(L_i)), base64(SEC1(R_i)) and
//                str(xs[i]) == item s+3i+2 == str(mod_hash(prefix that ends after R_i's "&"))          (:104-125)
//   a transcript of more than 2^17 bytes is invalid
// bit 1: a point of the proof (L_i, R_i, P, the per-proof u or u_new and P_new) is neither the identity nor on the curve.
// A proof with status 0 gets its record (k pairs (x_j, x_j^-1), a, b, w: what k_sc_svector_tables_batch reads) and its extra
// pairs in the order of include/bpmi.h; a flagged one gets zeros: it contributes nothing.
#pragma once
#include <stdio.h>

#include "rp_batch_host.hpp"
#include "ipa_packed_plan_host.hpp"

namespace ipap {

using rp::Sq;

// 32 little-endian bytes; false when the value is not below q
static inline bool load_lt_q(Sq &r, const uint8_t *b) { memcpy(r.v, b, 32); return !rp::ge_q(r.v); }
// the 33-byte SEC1 form of a 64-byte affine little-endian point (x and the parity of y); 33 zero bytes for the identity, as
// rp::point_item expects
static inline void sec1_of(uint8_t comp[33], const uint8_t pt[64]) {
  uint8_t any = 0;
  for (int i = 0; i < 64; i++) any |= pt[i];
  memset(comp, 0, 33);
  if (!any) return;
  comp[0] = 2 | (pt[32] & 1);
  for (int i = 0; i < 32; i++) comp[1 + i] = pt[31 - i];
}
static inline bool point_ok(const uint8_t pt[64]) {
  u32 w[16];
  memcpy(w, pt, 64);
  return bpmi::wire_point_valid(w);
}
static inline bool item_is_point(const rp::Items &it, size_t j, const uint8_t pt[64]) {
  uint8_t comp[33], item[48];
  sec1_of(comp, pt);
  const size_t l = rp::point_item(item, comp);
  return it.equals(j, item, l);
}

// the byte-level checks of proof p (bit 0); x1: Verifier1's challenge (Protocol 1)
static inline bool text_checks(u32 k, int protocol, uint64_t p, const IpaPackedIn &in, const Sq *xs, Sq &x1, rp::Items &it) {
  const uint64_t tlen = in.tr_off[p + 1] - in.tr_off[p];
  if (tlen > IPAP_MAX_TRANSCRIPT) return false;
  if (protocol == 2 && k == 0) return true;                       // no round: Verifier2 never looks at the transcript
  const uint8_t *ts = in.transcripts + in.tr_off[p];
  it.split(ts, (size_t)tlen);
  if (protocol == 1) {
    if (it.count() < 3) return false;
    rp::Sha s;
    rp::sha_init(s);
    rp::sha_update(s, (const uint8_t *)"1", 1);
    rp::sha_update(s, it.ptr(1), it.off[2] - it.off[1]);          // item 1 and its '&'
    Sq h;
    rp::mod_hash_q(h, s, it.ptr(1), it.off[2] - it.off[1]);
    if (!rp::parse_decimal(x1, it.ptr(2), it.len(2)) || !rp::q_eq(x1, h)) return false;
  }
  const size_t start = protocol == 1 ? 3 : (in.start ? in.start[p] : 1);
  const uint8_t *LR = in.LR + 128ull * k * p;
  rp::Sha run;
  rp::sha_init(run);
  rp::sha_update(run, (const uint8_t *)"1", 1);
  size_t hashed = 0;
  for (u32 i = 0; i < k; i++) {
    const size_t j = start + 3 * (size_t)i;
    if (j + 2 >= it.count()) return false;
    if (!item_is_point(it, j, LR + 64 * i) || !item_is_point(it, j + 1, LR + 64 * (k + i))) return false;
    const size_t upto = it.off[j + 2];                            // prefix incl. the '&' after item j+1
    rp::sha_update(run, ts + hashed, upto - hashed);
    hashed = upto;
    Sq h, xi;
    rp::mod_hash_q(h, run, ts, upto);
    if (!rp::parse_decimal(xi, it.ptr(j + 2), it.len(j + 2))) return false;
    if (!rp::q_eq(xi, h) || !rp::q_eq(xi, xs[i])) return false;
  }
  return true;
}

// proof p: its status byte; rec: 64 k + 96 bytes, pts / sc: ipap_pairs(k, protocol) x 64 / 32 bytes.  gbase: a class of a mixed batch
// (prepare_all_mixed): the call-wide index of the class's proof 0, added only to the index a seed weight is derived from
static inline uint8_t prepare_one(u32 k, int protocol, uint64_t p, const IpaPackedIn &in, uint8_t *rec, uint8_t *pts, uint8_t *sc, rp::Items &it, uint64_t gbase = 0) {
  const u32 pairs = ipap_pairs(k, protocol);
  Sq a, b, c = rp::q_small(0), x1 = rp::q_small(0), xs[IPAB_K_MAX], xinv[IPAB_K_MAX], pre[IPAB_K_MAX];
  bool ok = load_lt_q(a, in.ab + 64 * p);
  ok &= load_lt_q(b, in.ab + 64 * p + 32);
  if (protocol == 1) ok &= load_lt_q(c, in.c + 32 * p);
  for (u32 j = 0; j < k; j++) { ok &= load_lt_q(xs[j], in.xs + 32 * ((uint64_t)k * p + j)); ok &= !rp::q_is_zero(xs[j]); }      // a zero challenge cannot come out of mod_hash
  ok = ok && text_checks(k, protocol, p, in, xs, x1, it);
  // the points in the order of the extra pairs
  const uint8_t *src[2 * IPAB_K_MAX + 4];
  src[0] = protocol == 1 ? in.head + 128 * p : in.u + 64 * p;
  for (u32 j = 0; j < 2 * k; j++) src[1 + j] = in.LR + 64 * (2ull * k * p + j);
  src[2 * k + 1] = protocol == 1 ? in.head + 128 * p + 64 : in.P + 64 * p;
  if (protocol == 1) { src[2 * k + 2] = in.P + 64 * p; src[2 * k + 3] = in.u; }
  bool curve = true;
  for (u32 t = 0; t < pairs - (protocol == 1 ? 1u : 0u); t++) curve &= point_ok(src[t]);      // Protocol 1's shared u: the entry point's, once
  const uint8_t status = (uint8_t)((ok ? 0 : 1) | (curve ? 0 : 2));
  if (status) {
    memset(rec, 0, 64 * (size_t)k + 96); memset(pts, 0, 64 * (size_t)pairs); memset(sc, 0, 32 * (size_t)pairs);
    return status;
  }
  Sq w[3];
  for (u32 t = 0; t < ipap_weights(protocol); t++) {
    if (in.weights) rp::q_from_le(w[t], in.weights + 32 * (ipap_weights(protocol) * p + t));
    else rp::derive_weight(w[t], in.seed, gbase + p, (int)t);
  }
  // one inversion for the k challenges (Montgomery's trick)
  Sq run = rp::q_small(1);
  for (u32 j = 0; j < k; j++) { pre[j] = run; rp::q_mul(run, run, xs[j]); }
  Sq rinv;
  rp::q_inv(rinv, run);
  for (u32 j = k; j-- > 0;) { rp::q_mul(xinv[j], rinv, pre[j]); rp::q_mul(rinv, rinv, xs[j]); }
  for (u32 j = 0; j < k; j++) { rp::q_to_le(rec + 64 * j, xs[j]); rp::q_to_le(rec + 64 * j + 32, xinv[j]); }
  rp::q_to_le(rec + 64 * k, a); rp::q_to_le(rec + 64 * k + 32, b); rp::q_to_le(rec + 64 * k + 64, w[0]);
  Sq t, v;
  rp::q_mul(t, w[0], a); rp::q_mul(t, t, b);
  if (protocol == 1) rp::q_add(t, t, w[2]);
  rp::q_to_le(sc, t);                                                                    // u: w a b (+ r2)
  for (u32 j = 0; j < k; j++) {
    rp::q_mul(t, w[0], xs[j]); rp::q_mul(t, t, xs[j]); rp::q_neg(v, t); rp::q_to_le(sc + 32 * (1 + j), v);              // L_j: -w x_j^2
    rp::q_mul(t, w[0], xinv[j]); rp::q_mul(t, t, xinv[j]); rp::q_neg(v, t); rp::q_to_le(sc + 32 * (1 + k + j), v);     // R_j: -w x_j^-2
  }
  if (protocol == 1) {
    rp::q_sub(t, w[1], w[0]); rp::q_to_le(sc + 32 * (2 * k + 1), t);                     // P_new: r1 - w
    rp::q_neg(t, w[1]); rp::q_to_le(sc + 32 * (2 * k + 2), t);                           // P: -r1
    rp::q_mul(t, w[1], c); rp::q_add(t, t, w[2]); rp::q_mul(t, t, x1); rp::q_neg(v, t); rp::q_to_le(sc + 32 * (2 * k + 3), v);      // u: -(r1 c + r2) x
  } else {
    rp::q_neg(t, w[0]); rp::q_to_le(sc + 32 * (2 * k + 1), t);                           // P: -w
  }
  for (u32 t2 = 0; t2 < pairs; t2++) memcpy(pts + 64 * t2, src[t2], 64);
  return 0;
}

// ---- a MIXED batch: classes of different k in one call (include/bpmi.h, bpmi_ipa_batch_prepare_mixed).  The specification the
// kernels k_ipap_roles_mixed / k_ipap_finish_mixed are compared with byte for byte (tests/test_gpu_ipa_packed_mixed.py).
// One class: its arrays (in.weights: the class's slice of the explicit weights, or null), where its blocks of the outputs begin, and
// the global index of its proof 0 (status and seed weights).
struct MixedClass {
  u32 k = 0;
  uint64_t n_proofs = 0, gbase = 0;
  IpaPackedIn in;
  uint8_t *rec = nullptr, *pts = nullptr, *sc = nullptr;
};
// every proof of every class on `threads` host threads: contiguous ranges of the GLOBAL index, so the threads share the whole call,
// not one class after the other; status: the call's array.  The arguments have passed ipa_packed_mixed_plan.
static inline void prepare_all_mixed(int protocol, const std::vector<MixedClass> &cls, int threads, uint8_t *status) {
  uint64_t total = 0;
  for (const MixedClass &c : cls) total += c.n_proofs;
  auto range = [&](uint64_t lo, uint64_t hi) {
    rp::Items it;
    for (const MixedClass &c : cls) {
      const uint64_t a = lo > c.gbase ? lo - c.gbase : 0, b = hi < c.gbase + c.n_proofs ? (hi > c.gbase ? hi - c.gbase : 0) : c.n_proofs;
      const u32 pairs = ipap_pairs(c.k, protocol);
      const size_t rec_bytes = 64 * (size_t)c.k + 96;
      for (uint64_t p = a; p < b; p++)
        status[c.gbase + p] = prepare_one(c.k, protocol, p, c.in, c.rec + rec_bytes * p, c.pts + 64ull * pairs * p, c.sc + 32ull * pairs * p, it, c.gbase);
    }
  };
  uint64_t T = threads < 1 ? 1 : (uint64_t)threads;
  if (T > total) T = total ? total : 1;
  if (T == 1) { range(0, total); return; }
  std::vector<std::thread> pool;
  const uint64_t per = (total + T - 1) / T;
  for (uint64_t t = 0; t < T; t++) {
    const uint64_t lo = t * per, hi = lo + per < total ? lo + per : total;
    if (lo < hi) pool.emplace_back(range, lo, hi);
  }
  for (auto &th : pool) th.join();
}
// a UNIFORM call (bpmi_ipa_batch_prepare): one class at gbase 0; the arguments have passed ipa_packed_plan
static inline void prepare_all(u32 k, int protocol, uint64_t n_proofs, const IpaPackedIn &in, int threads, uint8_t *records, uint8_t *extra_pts,
                               uint8_t *extra_scalars, uint8_t *status) {
  MixedClass c;
  c.k = k; c.n_proofs = n_proofs; c.in = in; c.rec = records; c.pts = extra_pts; c.sc = extra_scalars;
  prepare_all_mixed(protocol, std::vector<MixedClass>(1, c), threads, status);
}

}  // namespace ipap
