// h2c.hpp -- part of libbpmi; plain C++ (BPMI_HD: host and device), also compiled by g++ behind tests/csrc_host/h2c_host_main.cpp.
// The per-candidate bodies of the reference's try-and-increment hash to the curve, elliptic_hash
// (/root/reference/src/utils/elliptic_curve_hash.py:7-23), which derives every generator of every protocol here.
//
// For a message msg the counters c = 1, 2, ... are tried in turn:
//   pre = str(c) || msg                       (decimal ASCII, no padding)
//   x   = SHA-256(pre), read big-endian;      x >= p: next c
//   rhs = x^3 + 7,  r = rhs^((p+1)/4);        r^2 != rhs: next c
//   bit = the low bit of the last byte of MD5(pre)
//   the point is (x, r) when bit = 1, else (x, p - r)
// THE SIGN IS NOT THE PARITY OF y: it is chosen by MD5 of the same prefixed message and by WHICH root the exponentiation returns.
//
// One text for both compilers: the kernels of h2c_kernels.hpp and the host twin of the tests run these bodies (rpd::sha_compress_v
// of rp_batch_kernels.hpp is device code only, so the SHA-256 compression is written out here once more, in plain C++).  MD5 is
// little-endian throughout -- message words and the 64-bit length -- where SHA-256 is big-endian; the padding geometry (0x80, zeros,
// eight length bytes) is the same, so ONE block feeder serves both.  MD5 is computed only for an accepted candidate: it is less than
// 1 % of the square root (253 squarings + 13 multiplications).
#pragma once
#include "field.hpp"

namespace bpmi {

typedef unsigned char h2c_u8;

// ---- the text in front of the message: <= 3 counter digits, and in the range form <= 10 index digits, as bytes in two registers ----
struct H2cPre { u64 lo, hi; u32 len; };                        // byte k of the prefix = bits 8k .. of lo (k < 8) or of hi (k >= 8)
BPMI_HD void h2c_pre_put(H2cPre &p, u32 byte) {
  if (p.len < 8u) p.lo |= (u64)byte << (8u * p.len);
  else p.hi |= (u64)byte << (8u * (p.len - 8u));
  p.len++;
}
BPMI_HD void h2c_pre_decimal(H2cPre &p, u32 v) {                // str(v): no padding, "0" for 0
  const u32 P10[10] = {1u, 10u, 100u, 1000u, 10000u, 100000u, 1000000u, 10000000u, 100000000u, 1000000000u};
  bool started = false;
#pragma unroll
  for (int e = 9; e >= 0; e--) {
    const u32 d = (v / P10[e]) % 10u;
    started = started || d != 0u || e == 0;
    if (started) h2c_pre_put(p, (u32)'0' + d);
  }
}
BPMI_HD u32 h2c_pre_byte(const H2cPre &p, u32 k) { return (u32)(k < 8u ? p.lo >> (8u * k) : p.hi >> (8u * (k - 8u))) & 0xFFu; }

// A message: bytes[0, len), and in the range form str(idx) in front of them (message i of a range call is str(lo + i) || tail)
struct H2cMsg { const h2c_u8 *bytes; u32 len; u32 idx; bool ranged; };
BPMI_HD H2cPre h2c_prefix(const H2cMsg &m, u32 c) {
  H2cPre p = {0, 0, 0};
  h2c_pre_decimal(p, c);
  if (m.ranged) h2c_pre_decimal(p, m.idx);
  return p;
}

// ---- the block feeder: block blk of the padded text  prefix || bytes[0, mlen)  as 16 words, MD5's way or SHA-256's -------------------
BPMI_HD u32 h2c_blocks(u32 total) { return (total + 9u + 63u) / 64u; }           // 0x80 and eight length bytes behind the text
template <bool MD5> BPMI_HD void h2c_block(u32 w[16], u32 blk, const H2cPre &pre, const h2c_u8 *bytes, u32 mlen) {
  const u32 total = pre.len + mlen;                             // <= 13 + 65 535: the length in bits fits one word
#pragma unroll
  for (int i = 0; i < 16; i++) {
    u32 word = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const u32 pos = blk * 64u + (u32)(4 * i + k);
      u32 byte = 0;
      if (pos < pre.len) byte = h2c_pre_byte(pre, pos);
      else if (pos < total) byte = bytes[pos - pre.len];
      else if (pos == total) byte = 0x80u;
      word = MD5 ? (word | (byte << (8 * k))) : ((word << 8) | byte);
    }
    w[i] = word;
  }
  if (blk + 1u == h2c_blocks(total)) {
    w[14] = MD5 ? total << 3 : total >> 29;
    w[15] = MD5 ? total >> 29 : total << 3;
  }
}

// ---- the two compressions ------------------------------------------------------------------------------------------------------------
BPMI_HD u32 h2c_rotl(u32 x, int n) { return (x << n) | (x >> (32 - n)); }
BPMI_HD void h2c_sha256_compress(u32 h[8], const u32 m[16]) {
  const u32 K[64] = {
      0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
      0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
      0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
      0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
      0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
      0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
  u32 w[16];
#pragma unroll
  for (int i = 0; i < 16; i++) w[i] = m[i];
  u32 a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
  for (int i = 0; i < 64; i++) {
    if (i >= 16) {                                              // the block as a 16-word shift register (static indices when unrolled)
      const u32 x = w[(i - 15) & 15], y = w[(i - 2) & 15];
      const u32 s0 = h2c_rotl(x, 25) ^ h2c_rotl(x, 14) ^ (x >> 3);
      const u32 s1 = h2c_rotl(y, 15) ^ h2c_rotl(y, 13) ^ (y >> 10);
      w[i & 15] = w[i & 15] + s0 + w[(i - 7) & 15] + s1;
    }
    const u32 S1 = h2c_rotl(e, 26) ^ h2c_rotl(e, 21) ^ h2c_rotl(e, 7);
    const u32 ch = (e & f) ^ (~e & g);
    const u32 t1 = hh + S1 + ch + K[i] + w[i & 15];
    const u32 S0 = h2c_rotl(a, 30) ^ h2c_rotl(a, 19) ^ h2c_rotl(a, 10);
    const u32 mj = (a & b) ^ (a & c) ^ (b & c);
    const u32 t2 = S0 + mj;
    hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
  }
  h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}
BPMI_HD void h2c_md5_compress(u32 h[4], const u32 m[16]) {
  const u32 K[64] = {                                           // floor(2^32 |sin(i + 1)|)
      0xd76aa478u, 0xe8c7b756u, 0x242070dbu, 0xc1bdceeeu, 0xf57c0fafu, 0x4787c62au, 0xa8304613u, 0xfd469501u, 0x698098d8u, 0x8b44f7afu, 0xffff5bb1u,
      0x895cd7beu, 0x6b901122u, 0xfd987193u, 0xa679438eu, 0x49b40821u, 0xf61e2562u, 0xc040b340u, 0x265e5a51u, 0xe9b6c7aau, 0xd62f105du, 0x02441453u,
      0xd8a1e681u, 0xe7d3fbc8u, 0x21e1cde6u, 0xc33707d6u, 0xf4d50d87u, 0x455a14edu, 0xa9e3e905u, 0xfcefa3f8u, 0x676f02d9u, 0x8d2a4c8au, 0xfffa3942u,
      0x8771f681u, 0x6d9d6122u, 0xfde5380cu, 0xa4beea44u, 0x4bdecfa9u, 0xf6bb4b60u, 0xbebfbc70u, 0x289b7ec6u, 0xeaa127fau, 0xd4ef3085u, 0x04881d05u,
      0xd9d4d039u, 0xe6db99e5u, 0x1fa27cf8u, 0xc4ac5665u, 0xf4292244u, 0x432aff97u, 0xab9423a7u, 0xfc93a039u, 0x655b59c3u, 0x8f0ccc92u, 0xffeff47du,
      0x85845dd1u, 0x6fa87e4fu, 0xfe2ce6e0u, 0xa3014314u, 0x4e0811a1u, 0xf7537e82u, 0xbd3af235u, 0x2ad7d2bbu, 0xeb86d391u};
  const int S[16] = {7, 12, 17, 22, 5, 9, 14, 20, 4, 11, 16, 23, 6, 10, 15, 21};
  u32 a = h[0], b = h[1], c = h[2], d = h[3];
#pragma unroll
  for (int i = 0; i < 64; i++) {
    u32 f;
    int g;
    if (i < 16) { f = (b & c) | (~b & d); g = i; }
    else if (i < 32) { f = (d & b) | (~d & c); g = (5 * i + 1) & 15; }
    else if (i < 48) { f = b ^ c ^ d; g = (3 * i + 5) & 15; }
    else { f = c ^ (b | ~d); g = (7 * i) & 15; }
    const u32 t = a + f + K[i] + m[g];
    a = d; d = c; c = b;
    b = b + h2c_rotl(t, S[4 * (i >> 4) + (i & 3)]);
  }
  h[0] += a; h[1] += b; h[2] += c; h[3] += d;
}

// SHA-256 (8 words: word 0 holds the digest's first four bytes) or MD5 (4 words: byte k of the digest = bits 8 (k mod 4) .. of word
// k / 4) of  prefix || bytes[0, mlen)
template <bool MD5> BPMI_HD void h2c_digest(u32 *h, const H2cPre &pre, const h2c_u8 *bytes, u32 mlen) {
  const u32 SHA0[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  const u32 MD50[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};
#pragma unroll
  for (int i = 0; i < (MD5 ? 4 : 8); i++) h[i] = MD5 ? MD50[i & 3] : SHA0[i];
  const u32 nblocks = h2c_blocks(pre.len + mlen);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (u32 blk = 0; blk < nblocks; blk++) {
    u32 w[16];
    h2c_block<MD5>(w, blk, pre, bytes, mlen);
    if (MD5) h2c_md5_compress(h, w);
    else h2c_sha256_compress(h, w);
  }
}

// ---- the candidate test ---------------------------------------------------------------------------------------------------------------
// d: the SHA-256 digest's 8 words (d[0] the most significant of x).  Accepted: x < p and x^3 + 7 a square; then wx = x as 8
// little-endian words and r = the CANONICAL root rhs^((p+1)/4).  No real digest is ever >= p (probability 2^-224): the host test
// calls this body directly to pin that branch.
BPMI_HD bool h2c_candidate_root(const u32 d[8], u32 wx[8], fe &r) {
#pragma unroll
  for (int k = 0; k < 8; k++) wx[k] = d[7 - k];
  // x < p:  x + (2^32 + 977) must not carry out of 256 bits
  u64 c = (u64)wx[0] + 977u; c >>= 32;
  c += (u64)wx[1] + 1u; c >>= 32;
#pragma unroll
  for (int k = 2; k < 8; k++) { c += wx[k]; c >>= 32; }
  const bool below = (c == 0);
  fe x, a, t, y;
  fe_from_words(x, wx);
  fe_sqr(t, x); fe_mul(a, t, x);
  fe seven; fe_set_zero(seven); seven.v[0] = 7;
  fe_add(a, a, seven); fe_carry(a, a);        // a = x^3 + 7
  fe_sqrt_candidate(y, a);
  fe_sqr(t, y);
  const bool square = fe_equal(t, a);
  fe_canon(r, y);
  return below && square;
}
// the point of an accepted candidate as 16 wire words (x || y, little-endian): the root itself when bit = 1, else p - root
// (the root 0, x^3 = -7, would leave as y = 0 either way; no digest is known to reach it)
BPMI_HD void h2c_candidate_point(u32 w16[16], const u32 wx[8], const fe &r, u32 bit) {
  fe y = r;
  if (!bit) { fe t; fe_neg(t, r); fe_canon(y, t); }
#pragma unroll
  for (int k = 0; k < 8; k++) w16[k] = wx[k];
  fe_to_words(w16 + 8, y);
}
// both halves at once (the host test's way in): 16 zero words when the candidate is rejected
BPMI_HD bool h2c_candidate(const u32 d[8], u32 bit, u32 w16[16]) {
  u32 wx[8];
  fe r;
  const bool ok = h2c_candidate_root(d, wx, r);
#pragma unroll
  for (int k = 0; k < 16; k++) w16[k] = 0;
  if (ok) h2c_candidate_point(w16, wx, r, bit);
  return ok;
}

// ---- one try, and the whole function --------------------------------------------------------------------------------------------------
// candidate c of message m: true and its point in w16 when it is accepted (w16 is untouched otherwise)
BPMI_HD bool h2c_try(const H2cMsg &m, u32 c, u32 w16[16]) {
  const H2cPre pre = h2c_prefix(m, c);
  u32 d[8], wx[8];
  fe r;
  h2c_digest<false>(d, pre, m.bytes, m.len);
  if (!h2c_candidate_root(d, wx, r)) return false;
  u32 h[4];
  h2c_digest<true>(h, pre, m.bytes, m.len);
  h2c_candidate_point(w16, wx, r, (h[3] >> 24) & 1u);          // the digest's 16th byte
  return true;
}
// the counter that succeeded (1 .. max_tries) and its point, or 0 and 16 zero words when none did; max_tries <= 255
BPMI_HD u32 h2c_hash(const H2cMsg &m, u32 max_tries, u32 w16[16]) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (u32 c = 1; c <= max_tries; c++)
    if (h2c_try(m, c, w16)) return c;
#pragma unroll
  for (int k = 0; k < 16; k++) w16[k] = 0;
  return 0;
}

}  // namespace bpmi
