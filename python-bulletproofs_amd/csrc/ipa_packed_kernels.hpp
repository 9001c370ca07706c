// ipa_packed_kernels.hpp -- part of libbpmi (included by bpmi.hip; one translation unit).  DEVICE code.
// The per-proof preparation of the batch verifier of PACKED inner-product proofs (the arrays bpmi_ipa_prove_batch writes) on
// the GPU: every proof's Fiat-Shamir transcript is re-hashed (SHA-256), the byte-level checks of the reference's verifiers run
// (inner_product_verifier.py:36-42 and :104-125), and the record of the s-vector sum (what k_sc_svector_tables_batch reads) and
// the weighted scalars of the proof's extra pairs are written where the batch's one MSM reads them.  It is the device twin of
// ipa_packed_host.hpp (same checks, same bytes: tests/test_gpu_ipa_packed.py); see that file for what each check means.
//
// Shape of the work: that of rp_batch_kernels.hpp, whose helpers (Sha, sha_feed, mod_hash_q, Walk, parse_decimal, the mod-q limb
// arithmetic) are used as they are.  A proof is a few SERIAL chains and a wave64 instruction costs the same whatever its
// active-lane count, so every chain runs with one lane per proof in full waves, one wave per kind of chain:
//   k_ipap_roles   role 0  the SHA-256 chain over the transcript: one running state that has absorbed "1", a digest of a copy
//                          after every R_i "&", compared with the x_i item and with xs[i]
//                  role 1  the text, range and on-curve checks: a, b, c < q; Verifier1's challenge re-hashed from item 1; the
//                          L_i / R_i items against base64(SEC1(point)); every point of the proof on the curve
//                  role 2  the inversion (Montgomery's trick over the k challenges, prefix products in LDS) and what hangs off
//                          it: the record (x_j, x_j^-1, a, b, w) and the R_j scalars
//                  role 3  the inverse-free scalars: u (and u_new), L_j, P (and P_new, u)
//   k_ipap_finish  one lane per extra pair: the status byte from the roles' verdicts; the pair's point copied (a valid proof) or
//                  the identity, a zero scalar and a zero record (a flagged one: it contributes nothing)
// A call over classes of different k (bpmi_ipa_verify_batch_packed_mixed_dev) runs the same bodies from k_ipap_roles_mixed -- one
// launch over the row chunks of every class -- and k_ipap_finish_mixed; see "a MIXED batch" below.
// Layout.  The fixed-size arrays (ab, xs, LR, P, ...) are read in place: a lane's 32- or 64-byte row is whole cache lines' worth
// of aligned words, and a row is read once.  The transcripts are TRANSPOSED first (k_ipap_transpose, the layout of k_rp_transpose
// with this ABI's 2^17-byte cap): the chain walks every transcript front to back, eight bytes at a time, and the proofs of a
// batch have the same shape, so word-major rows make a wave's load a few coalesced 512-byte lines instead of 64 scattered ones
// -- and the unchanged helpers of the range-proof path address exactly that layout (rpd::BPtr).
#pragma once

namespace ipad {

using namespace rpd;

struct Params {
  const u64 *T;              // the transcripts of this launch as 8-byte words, word-major over its proofs
  u32 Tstride;               // proofs of this launch
  const u64 *tr_off;         // whole call: n_proofs + 1 offsets
  const u32 *start;          // whole call, or null: 1 (Protocol 2) / 3 (Protocol 1) for every proof
  const uint8_t *ab, *xs, *LR, *u, *P, *c, *head;      // whole call
  const uint8_t *weights;    // whole call: P x 1 (Protocol 2) or P x 3 (Protocol 1) x 32 bytes, or null: derived from `seed`
  u32 seed[8];               // the 32 seed bytes as big-endian words
  u32 k, protocol, P_launch, Pall, validate;
  u64 first;                 // index of proof 0 of this launch inside the call
  u32 *records;              // whole call: 16 k + 24 words per proof
  u32 *extra_sc;             // whole call: pairs x 8 words per proof
  uint8_t *roles;            // [role * Pall + proof]: 0 = passed, bit 0 / bit 1 as in the status byte
  u64 gbase;                 // a class of a mixed batch (k_ipap_roles_mixed): the call-wide index of the class's proof 0 -- added only to the index a
                             // seed weight is derived from; explicit weights and every array stay class-local.  0: one class
};

extern __shared__ u32 ipap_slots[];        // role 2: k prefix products of 9 limbs per lane, limb-major

__device__ __forceinline__ bool load_le(sc &r, const uint8_t *p) {         // 32 little-endian bytes (8-byte aligned); false when >= q
  const u64 *s = reinterpret_cast<const u64 *>(p);
#pragma unroll
  for (int i = 0; i < 4; i++) { const u64 x = s[i]; r.v[2 * i] = (u32)x; r.v[2 * i + 1] = (u32)(x >> 32); }
  const u32 qq[8] = BPMI_SC_Q;
  u32 t[8];
  return bpmi::words_sub(t, r.v, qq) != 0;
}
__device__ __forceinline__ sc load_le_reduced(const uint8_t *p) { sc r; (void)load_le(r, p); bpmi::sc_reduce_once(r); return r; }

// does the item [p, p + n) spell base64(SEC1(point))?  pt: 64 bytes affine little-endian; the identity (all zero) is "AA=="
__device__ __noinline__ bool point_item_equals_le(const uint8_t *pt, const BPtr p, u32 n) {
  const u64 *s = reinterpret_cast<const u64 *>(pt);
  u64 x[4], any = 0, t[6];
#pragma unroll
  for (int i = 0; i < 4; i++) { x[i] = s[i]; any |= x[i]; }
  const u64 y0 = s[4];
  any |= y0 | s[5] | s[6] | s[7];
#pragma unroll
  for (int i = 0; i < 6; i++) t[i] = ld8(p + 8 * i);
  if (!any) return n == 4 && (u32)t[0] == 0x3D3D4141u;      // "AA=="
  if (n != 44) return false;
  // the 33 bytes 02|03, x big-endian, as little-endian words of a byte stream
  const u64 b0 = __builtin_bswap64(x[3]), b1 = __builtin_bswap64(x[2]), b2 = __builtin_bswap64(x[1]), b3 = __builtin_bswap64(x[0]);
  const u64 c[5] = {(2u | (y0 & 1u)) | (b0 << 8), (b0 >> 56) | (b1 << 8), (b1 >> 56) | (b2 << 8), (b2 >> 56) | (b3 << 8), b3 >> 56};
  bool same = true;
#pragma unroll
  for (int i = 0; i < 11; i++) {
    const u32 v = (byte_of(c, 3 * i) << 16) | (byte_of(c, 3 * i + 1) << 8) | byte_of(c, 3 * i + 2);
    same &= byte_of(t, 4 * i) == b64_char((v >> 18) & 63) && byte_of(t, 4 * i + 1) == b64_char((v >> 12) & 63) &&
            byte_of(t, 4 * i + 2) == b64_char((v >> 6) & 63) && byte_of(t, 4 * i + 3) == b64_char(v & 63);
  }
  return same;
}
__device__ __noinline__ bool point_on_curve(const uint8_t *pt) {
  u32 w[16];
  ::load_words16(w, reinterpret_cast<const u32 *>(pt));
  return bpmi::wire_point_valid(w);
}

struct Proof {
  BPtr ts;            // the transcript
  u32 tlen;           // its length (<= IPAP_MAX_TRANSCRIPT)
  u32 start;          // item at which the rounds begin
  u64 G;              // index inside the call
};

// the walker at item `start`
__device__ __forceinline__ void walk_to_rounds(Walk &w, const Proof &pr) {
  walk_init(w, pr.ts, pr.tlen);
  for (u32 j = 0; j < pr.start && w.have; j++) walk_next(w, walk_end(w));
}

// ---- role 0: per round i the prefix that ends after R_i's '&' is re-hashed and must spell the x_i item, which must be xs[i]
__device__ __forceinline__ bool role_hash(const Params &q, const Proof &pr) {
  Walk w;
  walk_to_rounds(w, pr);
  Sha run;
  sha_init(run);
  sha_push_byte(run, '1');
  u32 hashed = 0;
  for (u32 i = 0; i < q.k; i++) {
    if (!w.have) return false;
    walk_next(w, walk_end(w));                                     // L_i and R_i: role 1
    if (!w.have) return false;
    walk_next(w, walk_end(w));
    if (!w.have) return false;
    const u32 upto = w.pos;                                        // prefix incl. the '&' after R_i
    sha_feed(run, pr.ts + hashed, upto - hashed);
    hashed = upto;
    sc h, xi;
    mod_hash_q(h, run, pr.ts, upto);
    const u32 e = walk_end(w);
    const Dec d = parse_decimal(w.p + w.pos, e - w.pos);
    const bool lt = load_le(xi, q.xs + 32 * ((u64)q.k * pr.G + i));
    if (!(lt && d.ok && sc_eq(d.v, h) && sc_eq(d.v, xi))) return false;
    walk_next(w, e);
  }
  return true;
}

// ---- role 1: the ranges, Verifier1's challenge, the L_i / R_i items, the points.  Returns the two status bits it can set.
__device__ __forceinline__ u32 role_text(const Params &q, const Proof &pr, bool too_long) {
  const u32 k = q.k;
  sc v;
  bool ok = !too_long;
  ok &= load_le(v, q.ab + 64 * pr.G);
  ok &= load_le(v, q.ab + 64 * pr.G + 32);
  if (q.protocol == 1) ok &= load_le(v, q.c + 32 * pr.G);
  const uint8_t *LR = q.LR + 128ull * k * pr.G;
  if (ok && q.protocol == 1) {                                       // item 2 = str(mod_hash(item 1 + "&"))
    Walk w;
    walk_init(w, pr.ts, pr.tlen);
    walk_next(w, walk_end(w));
    ok = w.have;
    if (ok) {
      const u32 b1 = w.pos;
      walk_next(w, walk_end(w));
      ok = w.have;
      if (ok) {
        Sha s;
        sha_init(s);
        sha_push_byte(s, '1');
        sha_feed(s, pr.ts + b1, w.pos - b1);
        sc h;
        mod_hash_q(h, s, pr.ts + b1, w.pos - b1);
        const Dec d = parse_decimal(w.p + w.pos, walk_end(w) - w.pos);
        ok = d.ok && sc_eq(d.v, h);
      }
    }
  }
  if (ok && k) {                                                     // items s+3i, s+3i+1 are base64(SEC1(L_i)), base64(SEC1(R_i))
    Walk w;
    walk_to_rounds(w, pr);
    for (u32 i = 0; i < k && ok; i++) {
      ok = w.have;
      if (!ok) break;
      u32 e = walk_end(w);
      ok = point_item_equals_le(LR + 64 * i, w.p + w.pos, e - w.pos);
      walk_next(w, e);
      ok = ok && w.have;
      if (!ok) break;
      e = walk_end(w);
      ok = point_item_equals_le(LR + 64 * (k + i), w.p + w.pos, e - w.pos);
      walk_next(w, e);
      ok = ok && w.have;
      if (!ok) break;
      walk_next(w, walk_end(w));                                     // x_i: role 0
    }
  }
  bool curve = true;
  if (q.validate) {
    for (u32 j = 0; j < 2 * k; j++) curve &= point_on_curve(LR + 64 * j);
    curve &= point_on_curve(q.P + 64 * pr.G);
    if (q.protocol == 1) { curve &= point_on_curve(q.head + 128 * pr.G); curve &= point_on_curve(q.head + 128 * pr.G + 64); }
    else curve &= point_on_curve(q.u + 64 * pr.G);
  }
  return (ok ? 0u : 1u) | (curve ? 0u : 2u);
}

__device__ __forceinline__ sq weight_of(const Params &q, u64 G, u32 t) {
  sc ws;
  if (q.weights) ws = load_le_reduced(q.weights + 32 * ((q.protocol == 1 ? 3 : 1) * G + t));
  else ws = derive_weight(q.seed, q.gbase + G, t);
  return to_sq(ws);
}

// ---- role 2: Montgomery's trick inside the lane: prefix products of x_0 .. x_(k-1) (LDS), one inversion, then the backward
// pass hands out x_t^-1 for t = k-1 .. 0; the record and the R_t scalars (-w x_t^-2) are stored as they appear
__device__ __forceinline__ bool role_inverse(const Params &q, const Proof &pr) {
  const u32 k = q.k, lane = threadIdx.x;
  auto slot_store = [&](u32 slot, const sq &x) {
#pragma unroll
    for (int wd = 0; wd < 9; wd++) ipap_slots[(slot * 9 + wd) * 64 + lane] = x.v[wd];
  };
  auto slot_load = [&](sq &x, u32 slot) {
#pragma unroll
    for (int wd = 0; wd < 9; wd++) x.v[wd] = ipap_slots[(slot * 9 + wd) * 64 + lane];
  };
  const uint8_t *xs = q.xs + 32ull * k * pr.G;
  u32 *rec = q.records + (size_t)(16 * k + 24) * pr.G;
  u32 *op = q.extra_sc + (size_t)(2 * k + (q.protocol == 1 ? 4 : 2)) * 8 * pr.G;
  bool nonzero = true;
  sq run = bpmi::sq_small(1);
  for (u32 t = 0; t < k; t++) {
    const sc xv = load_le_reduced(xs + 32 * t);
    nonzero &= !bpmi::sc_is_zero(xv);
    slot_store(t, run);
    mq(run, run, to_sq(xv));
  }
  if (!nonzero) return false;                                // a zero challenge cannot come out of mod_hash
  sq rinv = to_sq(invq_v(to_sc(run)));
  const sq w = weight_of(q, pr.G, 0);
  for (u32 t = k; t-- > 0;) {
    const sc xv = load_le_reduced(xs + 32 * t);
    sq pre, xi, u;
    slot_load(pre, t);
    mq(xi, rinv, pre);                                       // x_t^-1
    if (t) mq(rinv, rinv, to_sq(xv));
    ::store_words8(rec + 16 * t, xv.v);
    store_canon(rec + 16 * t + 8, xi);
    mq(u, xi, xi); mq(u, w, u); bpmi::sq_neg(u, u);
    store_canon(op + (1 + k + t) * 8, u);
  }
  const sc a = load_le_reduced(q.ab + 64 * pr.G), b = load_le_reduced(q.ab + 64 * pr.G + 32);
  ::store_words8(rec + 16 * k, a.v);
  ::store_words8(rec + 16 * k + 8, b.v);
  store_canon(rec + 16 * k + 16, w);
  return true;
}

// ---- role 3: the scalars that need no inverse
__device__ __forceinline__ bool role_scalars(const Params &q, const Proof &pr, bool too_long) {
  const u32 k = q.k;
  u32 *op = q.extra_sc + (size_t)(2 * k + (q.protocol == 1 ? 4 : 2)) * 8 * pr.G;
  const sq w = weight_of(q, pr.G, 0);
  sq t, u;
  {
    const sc a = load_le_reduced(q.ab + 64 * pr.G), b = load_le_reduced(q.ab + 64 * pr.G + 32);
    mq(t, w, to_sq(a)); mq(t, t, to_sq(b));                          // w a b
  }
  for (u32 j = 0; j < k; j++) {
    const sq xj = to_sq(load_le_reduced(q.xs + 32 * ((u64)k * pr.G + j)));
    mq(u, xj, xj); mq(u, w, u); bpmi::sq_neg(u, u);
    store_canon(op + (1 + j) * 8, u);                                // L_j: -w x_j^2
  }
  if (q.protocol == 2) {
    store_canon(op, t);
    bpmi::sq_neg(u, w); store_canon(op + (2 * k + 1) * 8, u);        // P: -w
    return true;
  }
  const sq r1 = weight_of(q, pr.G, 1), r2 = weight_of(q, pr.G, 2);
  bpmi::sq_add(t, t, r2); store_canon(op, t);                        // u_new: w a b + r2
  bpmi::sq_sub(u, r1, w); store_canon(op + (2 * k + 1) * 8, u);      // P_new: r1 - w
  bpmi::sq_neg(u, r1); store_canon(op + (2 * k + 2) * 8, u);         // P: -r1
  if (too_long) return false;
  Walk wk;                                                           // x = item 2
  walk_init(wk, pr.ts, pr.tlen);
  walk_next(wk, walk_end(wk));
  if (!wk.have) return false;
  walk_next(wk, walk_end(wk));
  if (!wk.have) return false;
  const Dec d = parse_decimal(wk.p + wk.pos, walk_end(wk) - wk.pos);
  if (!d.ok) return false;
  const sc c = load_le_reduced(q.c + 32 * pr.G);
  mq(t, r1, to_sq(c)); bpmi::sq_add(t, t, r2); mq(t, t, to_sq(d.v)); bpmi::sq_neg(t, t);
  store_canon(op + (2 * k + 3) * 8, t);                              // u: -(r1 c + r2) x
  return true;
}

// Four waves per 64 proofs, one per role.  roles[role * Pall + proof] = the status bits that role found.
// (the body of block `blk` of the launch: k_ipap_roles runs it for its own blocks, k_ipap_roles_mixed for the blocks of a unit)
__device__ __forceinline__ void ipap_roles_block(const Params &q, u32 blk) {
  const u32 role = blk & (IPAP_ROLES - 1);
  const u32 g = (blk / IPAP_ROLES) * 64 + threadIdx.x;
  if (g >= q.P_launch) return;
  Proof pr;
  pr.G = q.first + g;
  pr.ts.base = q.T + g; pr.ts.stride = q.Tstride; pr.ts.off = 0;
  const u64 len64 = q.tr_off[pr.G + 1] - q.tr_off[pr.G];
  const bool too_long = len64 > IPAP_MAX_TRANSCRIPT;
  pr.tlen = too_long ? 0u : (u32)len64;
  pr.start = q.protocol == 1 ? 3u : (q.start ? q.start[pr.G] : 1u);
  u32 bits;
  if (role == 0) bits = too_long || role_hash(q, pr) ? 0u : 1u;
  else if (role == 1) bits = role_text(q, pr, too_long);
  else if (role == 2) bits = role_inverse(q, pr) ? 0u : 1u;
  else bits = role_scalars(q, pr, too_long) ? 0u : 1u;
  q.roles[(size_t)role * q.Pall + pr.G] = (uint8_t)bits;
}
__global__ void __launch_bounds__(64) k_ipap_roles(Params q) { ipap_roles_block(q, blockIdx.x); }

// Extra pair `idx` (= proof * pairs + t) of the class q describes.  A proof some role flagged contributes nothing: identity points, zero
// scalars, a zero record.  extra_pts: the class's block; status: the byte of the class's proof 0.
__device__ __forceinline__ void ipap_finish_pair(const Params &q, u32 pairs, u64 idx, u32 *extra_pts, uint8_t *status) {
  const u32 p = (u32)(idx / pairs), t = (u32)(idx % pairs), k = q.k;
  u32 bits = 0;
#pragma unroll
  for (u32 r = 0; r < IPAP_ROLES; r++) bits |= q.roles[(size_t)r * q.Pall + p];
  u32 w[16];
#pragma unroll
  for (int i = 0; i < 16; i++) w[i] = 0;
  if (!bits) {
    const uint8_t *src;
    if (t == 0) src = q.protocol == 1 ? q.head + 128ull * p : q.u + 64ull * p;
    else if (t <= 2 * k) src = q.LR + 64 * (2ull * k * p + (t - 1));
    else if (t == 2 * k + 1) src = q.protocol == 1 ? q.head + 128ull * p + 64 : q.P + 64ull * p;
    else if (t == 2 * k + 2) src = q.P + 64ull * p;
    else src = q.u;
    ::load_words16(w, reinterpret_cast<const u32 *>(src));
  } else {
    ::store_words8(q.extra_sc + 8 * idx, w);
    if (t == 0) {
      u32 *rec = q.records + (size_t)(16 * k + 24) * p;
      for (u32 i = 0; i < 2 * k + 3; i++) ::store_words8(rec + 8 * i, w);
    }
  }
  ::store_words16(extra_pts + 16 * idx, w);
  if (t == 0) status[p] = (uint8_t)bits;
}
// One lane per extra pair of the call.
__global__ void __launch_bounds__(256) k_ipap_finish(Params q, u32 pairs, u32 *extra_pts, uint8_t *status) {
  const u64 idx = (u64)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (u64)q.Pall * pairs) return;
  ipap_finish_pair(q, pairs, idx, extra_pts, status);
}

// ---- a MIXED batch (bpmi_ipa_verify_batch_packed_mixed_dev, ipa_packed_mixed_dev_host.hpp): classes of different k in one call.
// k_ipap_roles is single-wave serial chains and a class of a few hundred proofs fills a few percent of the chip: queued class after
// class the chains of the classes would run one behind the other.  Here ONE launch runs the row chunks of every class of a round
// (the shape of rpd::k_rp_roles_mixed): a device table of units {the class's Params for this round, the unit's first block}, read
// with plain loads at an index that depends on blockIdx alone (uniform per block: scalar loads), then the SAME per-lane bodies.  A
// class's records / extra_sc / roles pointers point at its own blocks, so the bodies' addressing holds unchanged.  The dynamic LDS
// of the launch is that of the round's largest k (role 2's prefix products: k x 9 x 64 words).
struct MixedUnit { Params q; u32 first_block, pad; };      // blocks [first_block, next unit's first_block) of the launch are this unit's
static_assert(sizeof(MixedUnit) <= IPAPM_UNIT_STRIDE, "the plan lays the unit table out in IPAPM_UNIT_STRIDE-byte slots (ipa_packed_mixed_plan_host.hpp)");
__device__ __forceinline__ const MixedUnit *mixed_unit_at(const uint8_t *units, u32 i) { return (const MixedUnit *)(units + (size_t)IPAPM_UNIT_STRIDE * i); }
// the unit whose blocks hold blockIdx.x: the last one with first_block <= blockIdx.x (at most 64 units per round; the firsts ascend from 0)
__global__ void __launch_bounds__(64) k_ipap_roles_mixed(const uint8_t *__restrict__ units, u32 n_units) {
  u32 u = 0;
  while (u + 1 < n_units && mixed_unit_at(units, u + 1)->first_block <= blockIdx.x) u++;
  const MixedUnit *mu = mixed_unit_at(units, u);
  const Params q = mu->q;
  ipap_roles_block(q, blockIdx.x - mu->first_block);
}
// One lane per extra pair of the call; the lane's class by bisection over the pair offsets (n_cls + 1 ascending words, pair_off[0] = 0).
// classes: slot j = the Params of non-empty class j (Pall = its proofs, gbase = its first global index; first_block is not used);
// extra_pts: the call's array (the classes' blocks back to back); status: the call's array, global index.
__global__ void __launch_bounds__(256) k_ipap_finish_mixed(const uint8_t *__restrict__ classes, const u32 *__restrict__ pair_off, u32 n_cls, u32 *extra_pts, uint8_t *status) {
  const u64 idx = (u64)blockIdx.x * 256 + threadIdx.x;
  if (idx >= pair_off[n_cls]) return;
  u32 lo = 0, hi = n_cls;                                     // pair_off[lo] <= idx < pair_off[hi]
  while (hi - lo > 1) {
    const u32 mid = (lo + hi) / 2;
    if (pair_off[mid] <= idx) lo = mid; else hi = mid;
  }
  const Params q = mixed_unit_at(classes, lo)->q;
  const u32 first = pair_off[lo];
  ipap_finish_pair(q, 2u * q.k + (q.protocol == 1 ? 4u : 2u), idx - first, extra_pts + 16ull * first, status + q.gbase);
}

// T[w * P + g] = bytes [8w, 8w + 8) of the transcript of proof first + g for w < W, zero beyond its end (or beyond `cap`).  64 x 64
// tiles through LDS, as k_rp_transpose: rows (proofs) are read as 512 contiguous bytes, columns written as 512 contiguous bytes.
// `text` holds the call's transcripts from byte `origin` (= tr_off[0]) on, with 8 readable bytes behind the last one; `off` points at
// the offsets of this launch's first proof.
__global__ void __launch_bounds__(256) k_ipap_transpose(const uint8_t *__restrict__ text, const u64 *__restrict__ off, u64 origin, u32 P, u32 W, u32 cap, u64 *__restrict__ T) {
  __shared__ u64 tile[64][65];
  const u32 g0 = blockIdx.x * 64, w0 = blockIdx.y * 64, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (u32 r = wave; r < 64; r += 4) {
    const u32 g = g0 + r;
    u64 x = 0;
    if (g < P) {
      const u64 beg = off[g];
      u64 len = off[g + 1] - beg;
      if (len > cap) len = 0;                                    // an invalid proof: nothing of it is read
      const u64 o = 8ull * (w0 + lane);
      if (o < len) {
        __builtin_memcpy(&x, text + (beg - origin) + o, 8);
        const u64 left = len - o;
        if (left < 8) x &= (1ull << (8 * left)) - 1ull;
      }
    }
    tile[r][lane] = x;
  }
  __syncthreads();
  for (u32 c = wave; c < 64; c += 4) {
    const u32 w = w0 + c, g = g0 + lane;
    if (w < W && g < P) T[(size_t)w * P + g] = tile[lane][c];
  }
}

}  // namespace ipad
