// ipa_wire_host.hpp -- part of libbpmi; plain C++17 over namespace rp of rp_batch_host.hpp and the host build of field.hpp (no HIP),
// also compiled for the host by tests/csrc_host.  The wire format BPIP2 of a Protocol-2 inner-product proof of n = 2^k elements:
//   "BPIP2" | k (1 B)                              k <= 22
//   a | b | xs[0..k)                               (2 + k) x 32 B big-endian
//   L_0 .. L_(k-1) R_0 .. R_(k-1)                  2k x 33 B SEC1 compressed; 33 zero bytes = the identity
//   start (4 B big-endian)                         Proof2.start_transcript
//   prefix_len (4 B big-endian) | prefix           the transcript's bytes before item `start`
// 78 + 98 k + prefix_len bytes: the packed form (include/bpmi.h, bpmi_ipa_prove_batch) without what a verifier can rebuild -- the
// y coordinates, and the rounds' text, which spells the same points in base64 and the same challenges in decimal.  A blob stands
// for the packed proof with ab, xs little-endian, LR the decompressed points, `start`, and the transcript
//   prefix || for each round j:  item(L_j) "&" item(R_j) "&" decimal(x_j) "&"          item = base64(SEC1(point)), "AA==" for the identity
// which is what FastNIProver2 writes (/root/reference/src/innerproduct/inner_product_prover.py:94-110 over
// src/utils/transcript.py:13-29); a wire proof is valid exactly when that packed proof is valid for the packed verifier.
// encode(): packed -> blobs, refusing a proof whose transcript is not that text (trailing text, too few '&', a non-canonical item)
// or whose values have no wire form (a scalar >= q, a point off the curve).  expand(): blobs -> packed arrays and a status byte
//   bit 0   malformed: wrong magic, a k byte that is not the call's, a length that is not 78 + 98 k + prefix_len, a, b or x_j >= q,
//           an expansion above 2^17 bytes.  Nothing of it is expanded: zero rows in ab and xs, start 0, an empty transcript
//   bit 1   a point that does not decode: a tag other than 0, 2, 3, tag 0 with a non-zero x, x >= p, an x with no y.  Its LR row is zero
// The points are decoded whenever the blob carries the call's header and is long enough for its fixed part (the device decodes
// them beside the expansion, before the scalars are looked at), so both bits can be set.  The device twins are the kernels of
// ipa_wire_kernels.hpp, compared with expand() byte for byte (tests/test_gpu_ipa_wire.py).
#pragma once
#include "rp_batch_host.hpp"
#include "ipa_wire_plan_host.hpp"

namespace ipaw {

static inline uint32_t be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
static inline void put_be32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }
static inline void reverse32(uint8_t *dst, const uint8_t *src) { for (int i = 0; i < 32; i++) dst[i] = src[31 - i]; }

// SEC1 compressed -> 64 bytes affine little-endian (zero: the identity, or an encoding that does not decode: false).  The host
// twin of ec_decompress_one (point_kernels.hpp): y = (x^3 + 7)^((p+1)/4), then the root of the tag's parity
// (/root/reference/src/utils/utils.py:119-131).
static inline bool decompress(const uint8_t comp[33], uint8_t pt[64]) {
  using namespace bpmi;
  memset(pt, 0, 64);
  u32 w[8], any = 0;
  for (int k = 0; k < 8; k++) {
    const uint8_t *q = comp + 1 + 28 - 4 * k;
    w[k] = ((u32)q[0] << 24) | ((u32)q[1] << 16) | ((u32)q[2] << 8) | (u32)q[3];
    any |= w[k];
  }
  if (comp[0] == 0) return any == 0;
  if (comp[0] != 2 && comp[0] != 3) return false;
  u64 c = (u64)w[0] + 977u; c >>= 32;           // x < p:  x + (2^32 + 977) must not carry out of 256 bits
  c += (u64)w[1] + 1u; c >>= 32;
  for (int k = 2; k < 8; k++) { c += w[k]; c >>= 32; }
  if (c) return false;
  fe x, y, a, t, seven, cx, cy;
  fe_from_words(x, w);
  fe_sqr(t, x); fe_mul(a, t, x);
  fe_set_zero(seven); seven.v[0] = 7;
  fe_add(a, a, seven); fe_carry(a, a);
  fe_sqrt_candidate(y, a);
  fe_sqr(t, y);
  if (!fe_equal(t, a)) return false;
  fe_canon(cy, y);
  if ((cy.v[0] & 1u) != (comp[0] & 1u)) { fe_neg(t, cy); fe_canon(cy, t); }
  fe_canon(cx, x);
  u32 w16[16];
  fe_to_words(w16, cx); fe_to_words(w16 + 8, cy);
  memcpy(pt, w16, 64);
  return true;
}

// decimal digits of x (no leading zeros; "0" for zero), then '&'
static inline void put_decimal(std::vector<uint8_t> &o, const rp::Sq &x) {
  uint64_t v[4] = {x.v[0], x.v[1], x.v[2], x.v[3]};
  char buf[80];
  int pos = 80;
  do {
    unsigned __int128 rem = 0;
    for (int k = 3; k >= 0; k--) { const unsigned __int128 cur = (rem << 64) | v[k]; v[k] = (uint64_t)(cur / 10); rem = cur % 10; }
    buf[--pos] = (char)('0' + (int)rem);
  } while (v[0] | v[1] | v[2] | v[3]);
  o.insert(o.end(), buf + pos, buf + 80);
  o.push_back('&');
}
static inline void put_point_item(std::vector<uint8_t> &o, const uint8_t comp[33]) {
  uint8_t item[48];
  const size_t l = rp::point_item(item, comp);
  o.insert(o.end(), item, item + l);
  o.push_back('&');
}
// the text of the rounds from the blob's own fields: comps = L_0 .. R_(k-1), 33 bytes each
static inline void rounds_text(std::vector<uint8_t> &o, u32 k, const uint8_t *comps, const rp::Sq *xs) {
  for (u32 j = 0; j < k; j++) { put_point_item(o, comps + 33 * (size_t)j); put_point_item(o, comps + 33 * (size_t)(k + j)); put_decimal(o, xs[j]); }
}

// ---- packed -> wire.  One proof: ab 64 B, xs 32 k B, LR 128 k B, its transcript and start; false: not encodable (blob untouched)
static inline bool encode_one(u32 k, const uint8_t *ab, const uint8_t *xs, const uint8_t *LR, const uint8_t *ts, uint64_t tlen, uint32_t start,
                              std::vector<uint8_t> &blob, rp::Items &it) {
  if (tlen > IPAP_MAX_TRANSCRIPT) return false;
  rp::Sq s, x[IPAB_K_MAX];
  auto below_q = [](rp::Sq &r, const uint8_t *p) { memcpy(r.v, p, 32); return !rp::ge_q(r.v); };
  if (!below_q(s, ab) || !below_q(s, ab + 32)) return false;
  for (u32 j = 0; j < k; j++) if (!below_q(x[j], xs + 32 * (size_t)j)) return false;
  std::vector<uint8_t> comps(33 * 2 * (size_t)k + 1);
  for (u32 j = 0; j < 2 * k; j++) {
    const uint8_t *pt = LR + 64 * (size_t)j;
    u32 w[16];
    memcpy(w, pt, 64);
    if (!bpmi::wire_point_valid(w)) return false;
    uint8_t *c = comps.data() + 33 * (size_t)j, any = 0;
    for (int i = 0; i < 64; i++) any |= pt[i];
    memset(c, 0, 33);
    if (any) { c[0] = 2 | (pt[32] & 1); reverse32(c + 1, pt); }
  }
  it.split(ts, (size_t)tlen);
  if ((uint64_t)start + 1 > it.count()) return false;               // fewer than `start` '&'
  const size_t prefix_len = it.off[start];
  std::vector<uint8_t> text;
  rounds_text(text, k, comps.data(), x);
  if (tlen - prefix_len != text.size() || (text.size() && memcmp(ts + prefix_len, text.data(), text.size()) != 0)) return false;
  blob.assign((size_t)ipaw_wire_bytes(k, prefix_len), 0);
  uint8_t *b = blob.data();
  memcpy(b, "BPIP2", 5); b[5] = (uint8_t)k;
  reverse32(b + 6, ab); reverse32(b + 38, ab + 32);
  for (u32 j = 0; j < k; j++) reverse32(b + 70 + 32 * (size_t)j, xs + 32 * (size_t)j);
  memcpy(b + ipaw_points_at(k), comps.data(), 66 * (size_t)k);
  put_be32(b + ipaw_start_at(k), start);
  put_be32(b + ipaw_start_at(k) + 4, (uint32_t)prefix_len);
  if (prefix_len) memcpy(b + ipaw_prefix_at(k), ts, prefix_len);
  return true;
}

// ---- wire -> packed.  One blob: its rows of ab (64 B), xs (32 k B), LR (128 k B), start, and its transcript in `text`; the status byte
static inline uint8_t expand_one(u32 k, const uint8_t *b, uint64_t len, uint8_t *ab, uint8_t *xs, uint8_t *LR, uint32_t *start, std::vector<uint8_t> &text) {
  text.clear();
  memset(ab, 0, 64);
  if (k) { memset(xs, 0, 32 * (size_t)k); memset(LR, 0, 128 * (size_t)k); }
  *start = 0;
  const bool head = len >= ipaw_fixed_bytes(k) && memcmp(b, "BPIP2", 5) == 0 && b[5] == k;
  if (!head) return 1;
  uint8_t status = 0;
  const uint8_t *comps = b + ipaw_points_at(k);
  for (u32 j = 0; j < 2 * k; j++)
    if (!decompress(comps + 33 * (size_t)j, LR + 64 * (size_t)j)) status |= 2;
  const uint64_t prefix_len = be32(b + ipaw_start_at(k) + 4);
  bool ok = ipaw_wire_bytes(k, prefix_len) == len;
  rp::Sq s[2], x[IPAB_K_MAX];
  bool lt;
  for (int i = 0; i < 2; i++) { rp::q_from_be(s[i], b + 6 + 32 * i, lt); ok &= lt; }
  for (u32 j = 0; j < k; j++) { rp::q_from_be(x[j], b + 70 + 32 * (size_t)j, lt); ok &= lt; }
  if (ok) {
    text.assign(b + ipaw_prefix_at(k), b + ipaw_prefix_at(k) + prefix_len);
    rounds_text(text, k, comps, x);
    ok = text.size() <= IPAP_MAX_TRANSCRIPT;
  }
  if (!ok) { text.clear(); return status | 1; }
  reverse32(ab, b + 6); reverse32(ab + 32, b + 38);
  for (u32 j = 0; j < k; j++) reverse32(xs + 32 * (size_t)j, b + 70 + 32 * (size_t)j);
  *start = be32(b + ipaw_start_at(k));
  return status;
}


// ---- a batch.  The arguments have passed the checks of the entry points (ipa_wire_dev_host.hpp).
// blobs back to back into blobs[0, cap) with off[0 .. n_proofs]; status[p] = 1 and an empty blob for a proof that is not encodable.
// false: cap ran out
static inline bool encode_all(u32 k, uint64_t n_proofs, const uint8_t *ab, const uint8_t *xs, const uint8_t *LR, const uint8_t *transcripts, const uint64_t *tr_off,
                              const uint32_t *start, uint8_t *blobs, uint64_t cap, uint64_t *off, uint8_t *status) {
  std::vector<uint8_t> blob;
  rp::Items it;
  uint64_t at = 0;
  off[0] = 0;
  for (uint64_t p = 0; p < n_proofs; p++) {
    const bool ok = encode_one(k, ab + 64 * p, xs + 32ull * k * p, LR + 128ull * k * p, transcripts + tr_off[p], tr_off[p + 1] - tr_off[p], start ? start[p] : 1u, blob, it);
    status[p] = ok ? 0 : 1;
    if (ok) {
      if (at + blob.size() > cap) return false;
      memcpy(blobs + at, blob.data(), blob.size());
      at += blob.size();
    }
    off[p + 1] = at;
  }
  return true;
}
// the expansions back to back into transcripts (which holds the plan's text_bound) with tr_off[0 .. n_proofs]
static inline void expand_all(u32 k, uint64_t n_proofs, const uint8_t *blobs, const uint64_t *off, uint8_t *ab, uint8_t *xs, uint8_t *LR, uint8_t *transcripts,
                              uint64_t *tr_off, uint32_t *start, uint8_t *status) {
  std::vector<uint8_t> text;
  uint64_t at = 0;
  tr_off[0] = 0;
  for (uint64_t p = 0; p < n_proofs; p++) {
    status[p] = expand_one(k, blobs + off[p], off[p + 1] - off[p], ab + 64 * p, xs + 32ull * k * p, LR + 128ull * k * p, start + p, text);
    if (!text.empty()) memcpy(transcripts + at, text.data(), text.size());
    at += text.size();
    tr_off[p + 1] = at;
  }
}

}  // namespace ipaw
