// field.hpp -- arithmetic in F_p, p = 2^256 - 2^32 - 977 (secp256k1 base field),
// for gfx950.  Replaces what the reference reaches through fastecdsa/GMP on every
// `Point + Point` (/root/reference/src/pippenger/group.py:31-32).
//
// Representation: 9 limbs of 29 bits in u32 (value = sum v[k] * 2^(29k)).
// Why not 8x32: on gfx950 v_mad_u64_u32 adds a full 64-bit value for free but has
// no carry-in, and a carry through VCC costs wait states (profiles/r01_fe_microbench.txt:
// 9x29 carry-free 171 G mul/s vs 8x32 137-165 G).  With 29-bit limbs nine products
// (< 2^58 each) accumulate in one u64 column with no carry handling at all.
//
// Magnitudes.  A value has magnitude m when every limb is < m * 2^29.
//   tight  = magnitude 1, limb 8 <= 2^24 + 2^20        (output of fe_carry)
//   loose  = limb 0 < 2^29 + 2^22, limb 1 < 2^29 + 2^15, limbs 2..7 < 2^29, limb 8 < 2^24 (output of the
//            multiplication family; counts as magnitude 1 -- every bound below has the 1 % of room it needs)
//   fe_add / fe_sub are LAZY (no carry): magnitudes add; fe_sub adds 2 (a bias of 2p)
//   the multiplication family needs  9 * (sum of mag(a) mag(b) over its products) <= 63
// Values are kept only weakly reduced (any representative < 2^257); fe_canon gives
// the unique representative in [0, p) for comparison and output.
//
// Everything here is plain C++ so the same header is unit-tested on the host
// (tests/csrc_host) before it ever runs on a GPU.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BPMI_HD __host__ __device__ __forceinline__
#else
#define BPMI_HD inline
#endif

namespace bpmi {

typedef uint32_t u32;
typedef uint64_t u64;

struct fe { u32 v[9]; };

constexpr u32 M29 = 0x1FFFFFFFu;
constexpr u32 M24 = 0x00FFFFFFu;

#define BPMI_FE_P     {0x1FFFFC2Fu, 0x1FFFFFF7u, 0x1FFFFFFFu, 0x1FFFFFFFu, 0x1FFFFFFFu, 0x1FFFFFFFu, 0x1FFFFFFFu, 0x1FFFFFFFu, 0x00FFFFFFu}
#define BPMI_FE_2P    {0x1FFFF85Eu, 0x1FFFFFEFu, 0x1FFFFFFFu, 0x1FFFFFFFu, 0x1FFFFFFFu, 0x1FFFFFFFu, 0x1FFFFFFFu, 0x1FFFFFFFu, 0x01FFFFFFu}
// 2p written with every limb >= the largest tight limb, so (a + BIAS2 - b) never borrows
#define BPMI_FE_BIAS2 {0x3FFFF85Eu, 0x3FFFFFEEu, 0x3FFFFFFEu, 0x3FFFFFFEu, 0x3FFFFFFEu, 0x3FFFFFFEu, 0x3FFFFFFEu, 0x3FFFFFFEu, 0x01FFFFFEu}
// 4p written so that a magnitude-2 value can be subtracted
#define BPMI_FE_BIAS4 {0x5FFFF0BCu, 0x5FFFFFDDu, 0x5FFFFFFDu, 0x5FFFFFFDu, 0x5FFFFFFDu, 0x5FFFFFFDu, 0x5FFFFFFDu, 0x5FFFFFFDu, 0x03FFFFFDu}
// 8p written with every limb about 6 * 2^29 (< 2^32): three loose values can be subtracted from it and the
// difference is still a valid 32-bit column addend
#define BPMI_FE_BIAS8 {0xBFFFE178u, 0xBFFFFFBAu, 0xBFFFFFFAu, 0xBFFFFFFAu, 0xBFFFFFFAu, 0xBFFFFFFAu, 0xBFFFFFFAu, 0xBFFFFFFAu, 0x07FFFFFAu}

BPMI_HD void fe_set_zero(fe &r) {
#pragma unroll
  for (int k = 0; k < 9; k++) r.v[k] = 0;
}
BPMI_HD void fe_set_one(fe &r) { fe_set_zero(r); r.v[0] = 1; }

// ---- 32-byte little-endian <-> limbs (the C-ABI layout: 8 x u32 LE words) ----
BPMI_HD void fe_from_words(fe &r, const u32 w[8]) {
#pragma unroll
  for (int k = 0; k < 9; k++) {
    const int bit = 29 * k, i = bit >> 5, s = bit & 31;
#if defined(__HIP_DEVICE_COMPILE__)
    // one v_alignbit_b32 per limb; the 64-bit form below made the vectoriser park the words in private memory and
    // reload them at odd offsets (80-140 B of scratch in k_ec_sum, k_ec_lincomb2, k_tail)
    const u32 hi = (i + 1 < 8) ? w[i + 1] : 0u;
    r.v[k] = (s ? __builtin_amdgcn_alignbit(hi, w[i], (u32)s) : w[i]) & M29;
#else
    u64 x = w[i];
    if (i + 1 < 8) x |= (u64)w[i + 1] << 32;
    r.v[k] = (u32)(x >> s) & M29;
#endif
  }
}
// a must be canonical (fe_canon) -- limbs < 2^29, value < 2^256
BPMI_HD void fe_to_words(u32 w[8], const fe &a) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const int bit = 32 * i, k = bit / 29, s = bit - 29 * k;
    u64 x = (u64)a.v[k] >> s;
    x |= (u64)a.v[k + 1] << (29 - s);
    if (k + 2 < 9) x |= (u64)a.v[k + 2] << (58 - s);
    w[i] = (u32)x;
  }
}

// ---- lazy add / sub ----------------------------------------------------------
BPMI_HD void fe_add(fe &r, const fe &a, const fe &b) {
#pragma unroll
  for (int k = 0; k < 9; k++) r.v[k] = a.v[k] + b.v[k];
}
// r = a - b + 2p ; b tight or loose; mag(r) = mag(a) + 2
BPMI_HD void fe_sub(fe &r, const fe &a, const fe &b) {
  const u32 bias[9] = BPMI_FE_BIAS2;
#pragma unroll
  for (int k = 0; k < 9; k++) r.v[k] = a.v[k] + bias[k] - b.v[k];
}
// r = a - b + 4p ; b of magnitude <= 2; mag(r) = mag(a) + 3
BPMI_HD void fe_sub_m2(fe &r, const fe &a, const fe &b) {
  const u32 bias[9] = BPMI_FE_BIAS4;
#pragma unroll
  for (int k = 0; k < 9; k++) r.v[k] = a.v[k] + bias[k] - b.v[k];
}
// r = 8p - a - 2b, as a column addend (limbs in [2^31, 2^32)); a, b loose
BPMI_HD void fe_bias8_sub_a_2b(fe &r, const fe &a, const fe &b) {
  const u32 bias[9] = BPMI_FE_BIAS8;
#pragma unroll
  for (int k = 0; k < 9; k++) r.v[k] = bias[k] - a.v[k] - (b.v[k] << 1);
}
// r = 4p - 2a, a column addend; a loose
BPMI_HD void fe_bias4_sub_2a(fe &r, const fe &a) {
  const u32 bias[9] = BPMI_FE_BIAS4;
#pragma unroll
  for (int k = 0; k < 9; k++) r.v[k] = bias[k] - (a.v[k] << 1);
}
// r = 4p - a - b, a column addend; a, b loose
BPMI_HD void fe_bias4_sub_a_b(fe &r, const fe &a, const fe &b) {
  const u32 bias[9] = BPMI_FE_BIAS4;
#pragma unroll
  for (int k = 0; k < 9; k++) r.v[k] = bias[k] - a.v[k] - b.v[k];
}
// r = 8p - 4a, a column addend; a loose
BPMI_HD void fe_bias8_sub_4a(fe &r, const fe &a) {
  const u32 bias[9] = BPMI_FE_BIAS8;
#pragma unroll
  for (int k = 0; k < 9; k++) r.v[k] = bias[k] - (a.v[k] << 2);
}
// r = 2a - b + 2p ; a, b loose; magnitude 4
BPMI_HD void fe_dbl_sub(fe &r, const fe &a, const fe &b) {
  const u32 bias[9] = BPMI_FE_BIAS2;
#pragma unroll
  for (int k = 0; k < 9; k++) r.v[k] = (a.v[k] << 1) + bias[k] - b.v[k];
}
// r = 2p - a ; a tight or loose; mag 2
BPMI_HD void fe_neg(fe &r, const fe &a) {
  const u32 bias[9] = BPMI_FE_BIAS2;
#pragma unroll
  for (int k = 0; k < 9; k++) r.v[k] = bias[k] - a.v[k];
}

// ---- carry: any limbs (< 2^32) -> tight -----------------------------------------
BPMI_HD void fe_carry(fe &r, const fe &a) {
  const u32 h = a.v[8] >> 24;                      // units of 2^256 == 2^32 + 977
  u64 c = (u64)a.v[0] + (u64)h * 977u;
  r.v[0] = (u32)c & M29; c >>= 29;
  c += (u64)a.v[1] + ((u64)h << 3);                // 2^32 = 2^29 * 8
  r.v[1] = (u32)c & M29; c >>= 29;
#pragma unroll
  for (int k = 2; k < 8; k++) { c += a.v[k]; r.v[k] = (u32)c & M29; c >>= 29; }
  r.v[8] = (a.v[8] & M24) + (u32)c;
}

// ---- the multiplication family: ONE reduction for a sum of limb products -----------------------------------
//   fe_mul(r, a, b)            r = a b
//   fe_sqr(r, a)               r = a^2
//   fe_mul_add(r, a, b, add)   r = a b + add         add: any 9 limbs < 2^32 (e.g. BIAS - x: a fused subtraction)
//   fe_sqr_add(r, a, add)      r = a^2 + add
//   fe_mul2(r, a, b, c, d)     r = a b + c d
//   fe_sqr3(r, a)              r = 3 a^2                 (the tangent slope numerator, without a lazy x3 and a carry)
//   fe_mul_add8(r, a, b, add)  r = a b + 8 add           (the - 8 Y^4 of a Jacobian doubling as 8 (2p - Y^4))
// All of them build the 17 product columns (a column of products and addends must stay below 2^64:
// 9 * (mag(a) mag(b) + mag(c) mag(d)) <= 63) and reduce ONCE, so a subtraction or a second product that feeds a
// multiplication result costs no carry pass and no second reduction (the mixed addition needs 9 reductions
// for its 8M + 2S instead of 10 plus four carry passes).
//
// The reduction (fe_mac_c below is its definition; csrc/field_gen.hpp is the same thing as chained v_mad_u64_u32):
//   columns 9..16  s = 8 hi32(previous s) + products; the limb th = lo32(s) stays a DIRTY 32-bit value, which is all
//                  the fold needs:  2^261 == 2^37 + 31264 (mod p), 2^37 = 2^8 2^29, so th[j] adds 31264 th[j] to
//                  column j and 256 th[j] to column j + 1 (hp, the carry out of column 16, is 8 hp at column
//                  17 = 8 + 9: 31264 * 8 hp to column 8; its 256 * 8 hp part, column 9, folds once more into columns 0, 1)
//   column 8       raw sum; its high 32 bits h8 are units of 2^264 == 2^40 + 250112 and are folded into columns 0, 1
//                  BEFORE the low chain runs; its low 32 bits s8m are kept as they are (no mask, no shift)
//   columns 0..7   s = carry + products + addend + fold terms; limb = s & M29, carry = s >> 29
//   end            limb 8 keeps 24 bits of (s8m + the last carry, < 2^35 + 2^32); the < 2^12 above them go to limbs
//                  0 and 1 WITHOUT a carry ripple.
// Output ("loose"): limb 0 < 2^29 + 2^22, limb 1 < 2^29 + 2^15, limbs 2..7 < 2^29, limb 8 < 2^24; value < 2^256 + 2^45.
// A loose value is a fine operand everywhere a tight one is (the biases below dominate its limbs, its magnitude is
// 1.008); its limb vector is still unique for a given integer, so 0 (mod p) is exactly "all limbs 0" or "the limbs
// of p" -- fe_is_zero_tight works on it unchanged.
struct fe_dcols { u64 c[17]; };
BPMI_HD void fe_cols_add_product(fe_dcols &q, const fe &a, const fe &b, u32 times = 1) {
#pragma unroll
  for (int i = 0; i < 9; i++)
#pragma unroll
    for (int j = 0; j < 9; j++) q.c[i + j] += (u64)(a.v[i] * times) * b.v[j];
}
BPMI_HD void fe_cols_reduce(fe &r, const fe_dcols &q) {
  u32 th[8], t[8];
  u64 s = q.c[9];
  th[0] = (u32)s;
  u32 hp = (u32)(s >> 32);
#pragma unroll
  for (int k = 10; k < 17; k++) {
    s = q.c[k] + ((u64)hp << 3);
    th[k - 9] = (u32)s;
    hp = (u32)(s >> 32);
  }
  // hp: the carry out of column 16, weight 2^(29*16+32) = 2^496 == 250112 * 2^232 + 64028672 + 524288 * 2^29
  s = q.c[8] + (u64)hp * 250112u + (u64)th[7] * 256u;
  // column 8's high half h8 has weight 2^264 == 250112 + 2048 * 2^29; its low half s8m waits for the last carry
  const u32 s8m = (u32)s, h8 = (u32)(s >> 32);
  s = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    s += q.c[k] + (u64)th[k] * 31264u;
    if (k >= 1) s += (u64)th[k - 1] * 256u;
    if (k == 0) s += (u64)hp * 64028672u + (u64)h8 * 250112u;
    if (k == 1) s += (u64)hp * 524288u + (u64)h8 * 2048u;
    t[k] = (u32)s & M29;
    s >>= 29;
  }
  s += s8m;
  const u32 v2 = (u32)(s >> 24);
  r.v[0] = t[0] + v2 * 977u;
  r.v[1] = t[1] + (v2 << 3);
#pragma unroll
  for (int k = 2; k < 8; k++) r.v[k] = t[k];
  r.v[8] = (u32)s & M24;
}
// r = times a b (+ c d) (+ add_scale add); c, d, add may be null
BPMI_HD void fe_mac_c(fe &r, const fe &a, const fe &b, const fe *c, const fe *d, const fe *add, u32 times = 1, u32 add_scale = 1) {
  fe_dcols q;
#pragma unroll
  for (int k = 0; k < 17; k++) q.c[k] = (add && k < 9) ? (u64)add->v[k] * add_scale : 0;
  fe_cols_add_product(q, a, b, times);
  if (c) fe_cols_add_product(q, *c, *d);
  fe_cols_reduce(r, q);
}

#include "field_gen.hpp"      // inside namespace bpmi: the generated device bodies (tools/gen_field_asm.py)

// The device runs the generated bodies, the host -- unit tests, host tail helpers -- the C body.  They are the
// same function: tests/test_csrc_host.py checks the C body against Python integers on adversarial limb patterns,
// tests/test_gpu_field.py checks on the GPU that both give identical limbs.
BPMI_HD void fe_mul(fe &r, const fe &a, const fe &b) {
#if defined(__HIP_DEVICE_COMPILE__)
  fe_mul_dev(r, a, b);
#else
  fe_mac_c(r, a, b, nullptr, nullptr, nullptr);
#endif
}
BPMI_HD void fe_sqr(fe &r, const fe &a) {
#if defined(__HIP_DEVICE_COMPILE__)
  fe_sqr_dev(r, a);
#else
  fe_mac_c(r, a, a, nullptr, nullptr, nullptr);
#endif
}
BPMI_HD void fe_sqr3(fe &r, const fe &a) {            // a loose or tight (6 x limb must fit 32 bits)
#if defined(__HIP_DEVICE_COMPILE__)
  fe_sqr3_dev(r, a);
#else
  fe_mac_c(r, a, a, nullptr, nullptr, nullptr, 3);
#endif
}
BPMI_HD void fe_mul_add8(fe &r, const fe &a, const fe &b, const fe &add) {
#if defined(__HIP_DEVICE_COMPILE__)
  fe_mul_add8_dev(r, a, b, add);
#else
  fe_mac_c(r, a, b, nullptr, nullptr, &add, 1, 8);
#endif
}
BPMI_HD void fe_mul_add(fe &r, const fe &a, const fe &b, const fe &add) {
#if defined(__HIP_DEVICE_COMPILE__)
  fe_mul_add_dev(r, a, b, add);
#else
  fe_mac_c(r, a, b, nullptr, nullptr, &add);
#endif
}
BPMI_HD void fe_sqr_add(fe &r, const fe &a, const fe &add) {
#if defined(__HIP_DEVICE_COMPILE__)
  fe_sqr_add_dev(r, a, add);
#else
  fe_mac_c(r, a, a, nullptr, nullptr, &add);
#endif
}
BPMI_HD void fe_mul2(fe &r, const fe &a, const fe &b, const fe &c, const fe &d) {
#if defined(__HIP_DEVICE_COMPILE__)
  fe_mul2_dev(r, a, b, c, d);
#else
  fe_mac_c(r, a, b, &c, &d, nullptr);
#endif
}

// r = a * k for a small constant, lazy: k * mag(a) must stay < 8, and k <= 7 when a is loose (limb 0 < 2^29 + 2^22)
BPMI_HD void fe_mul_small(fe &r, const fe &a, u32 k) {
#pragma unroll
  for (int i = 0; i < 9; i++) r.v[i] = a.v[i] * k;
}

// ---- canonical form in [0, p) ----------------------------------------------------
BPMI_HD void fe_canon(fe &r, const fe &a) {
  fe t;
  fe_carry(t, a);
  fe_carry(t, t);                                   // now value < 2^256 + tiny, tight
  // t >= p  <=>  t + (2^32 + 977) >= 2^256
  u32 s[9];
  u64 c = (u64)t.v[0] + 977u; s[0] = (u32)c & M29; c >>= 29;
  c += (u64)t.v[1] + 8u;      s[1] = (u32)c & M29; c >>= 29;
#pragma unroll
  for (int k = 2; k < 8; k++) { c += t.v[k]; s[k] = (u32)c & M29; c >>= 29; }
  c += t.v[8]; s[8] = (u32)c;
  const bool ge = (s[8] >> 24) != 0;
#pragma unroll
  for (int k = 0; k < 8; k++) r.v[k] = ge ? s[k] : t.v[k];
  r.v[8] = ge ? (s[8] & M24) : t.v[8];
}

// a tight: is it == 0 (mod p)?  The tight representatives of 0 below 2^257 are 0, p, 2p.
// Kept branch-free: a limb-0 pre-filter with an early return was measured and made the
// kernels that inline the general addition markedly slower (bucket reduce 0.41 -> 0.68 ms).
BPMI_HD bool fe_is_zero_tight(const fe &a) {
  const u32 P1[9] = BPMI_FE_P, P2[9] = BPMI_FE_2P;
  u32 z = 0, d1 = 0, d2 = 0;
#pragma unroll
  for (int k = 0; k < 9; k++) { z |= a.v[k]; d1 |= a.v[k] ^ P1[k]; d2 |= a.v[k] ^ P2[k]; }
  return (z == 0) | (d1 == 0) | (d2 == 0);
}
BPMI_HD bool fe_is_zero(const fe &a) {
  fe t;
  fe_carry(t, a);
  return fe_is_zero_tight(t);
}
BPMI_HD bool fe_equal(const fe &a, const fe &b) {   // both tight
  fe d;
  fe_sub(d, a, b);
  return fe_is_zero(d);
}

// r = a^(p-2): 255 squarings + 15 multiplications (addition chain on the run
// structure of p - 2 = 2^256 - 2^32 - 979: blocks of 223, 22, 1, 1 ones ...)
BPMI_HD void fe_inv(fe &r, const fe &a) {
  fe x2, x3, x6, x9, x11, x22, x44, x88, x176, x220, x223, t1;
  fe_sqr(x2, a); fe_mul(x2, x2, a);
  fe_sqr(x3, x2); fe_mul(x3, x3, a);
  x6 = x3; for (int j = 0; j < 3; j++) fe_sqr(x6, x6); fe_mul(x6, x6, x3);
  x9 = x6; for (int j = 0; j < 3; j++) fe_sqr(x9, x9); fe_mul(x9, x9, x3);
  x11 = x9; for (int j = 0; j < 2; j++) fe_sqr(x11, x11); fe_mul(x11, x11, x2);
  x22 = x11; for (int j = 0; j < 11; j++) fe_sqr(x22, x22); fe_mul(x22, x22, x11);
  x44 = x22; for (int j = 0; j < 22; j++) fe_sqr(x44, x44); fe_mul(x44, x44, x22);
  x88 = x44; for (int j = 0; j < 44; j++) fe_sqr(x88, x88); fe_mul(x88, x88, x44);
  x176 = x88; for (int j = 0; j < 88; j++) fe_sqr(x176, x176); fe_mul(x176, x176, x88);
  x220 = x176; for (int j = 0; j < 44; j++) fe_sqr(x220, x220); fe_mul(x220, x220, x44);
  x223 = x220; for (int j = 0; j < 3; j++) fe_sqr(x223, x223); fe_mul(x223, x223, x3);
  // p - 2 = 1^223 0 1^22 0000 101101
  t1 = x223; for (int j = 0; j < 23; j++) fe_sqr(t1, t1); fe_mul(t1, t1, x22);
  for (int j = 0; j < 5; j++) fe_sqr(t1, t1); fe_mul(t1, t1, a);
  for (int j = 0; j < 3; j++) fe_sqr(t1, t1); fe_mul(t1, t1, x2);
  for (int j = 0; j < 2; j++) fe_sqr(t1, t1); fe_mul(r, t1, a);
}

// r = a^((p+1)/4): a square root of a when a is a quadratic residue (p = 3 mod 4); the
// caller checks r^2 == a.  Same addition-chain prefix as fe_inv; (p+1)/4 = 1^223 0 1^22 0000 11 00.
BPMI_HD void fe_sqrt_candidate(fe &r, const fe &a) {
  fe x2, x3, x6, x9, x11, x22, x44, x88, x176, x220, x223, t1;
  fe_sqr(x2, a); fe_mul(x2, x2, a);
  fe_sqr(x3, x2); fe_mul(x3, x3, a);
  x6 = x3; for (int j = 0; j < 3; j++) fe_sqr(x6, x6); fe_mul(x6, x6, x3);
  x9 = x6; for (int j = 0; j < 3; j++) fe_sqr(x9, x9); fe_mul(x9, x9, x3);
  x11 = x9; for (int j = 0; j < 2; j++) fe_sqr(x11, x11); fe_mul(x11, x11, x2);
  x22 = x11; for (int j = 0; j < 11; j++) fe_sqr(x22, x22); fe_mul(x22, x22, x11);
  x44 = x22; for (int j = 0; j < 22; j++) fe_sqr(x44, x44); fe_mul(x44, x44, x22);
  x88 = x44; for (int j = 0; j < 44; j++) fe_sqr(x88, x88); fe_mul(x88, x88, x44);
  x176 = x88; for (int j = 0; j < 88; j++) fe_sqr(x176, x176); fe_mul(x176, x176, x88);
  x220 = x176; for (int j = 0; j < 44; j++) fe_sqr(x220, x220); fe_mul(x220, x220, x44);
  x223 = x220; for (int j = 0; j < 3; j++) fe_sqr(x223, x223); fe_mul(x223, x223, x3);
  t1 = x223; for (int j = 0; j < 23; j++) fe_sqr(t1, t1); fe_mul(t1, t1, x22);
  for (int j = 0; j < 6; j++) fe_sqr(t1, t1); fe_mul(t1, t1, x2);
  fe_sqr(t1, t1); fe_sqr(r, t1);
}

}  // namespace bpmi
