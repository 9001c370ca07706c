// ipa_packed_plan_host.hpp -- part of libbpmi; plain C++17 (no HIP, no bpmi_ctx), also compiled for the host by tests/csrc_host.
// The plan of a batch of PACKED inner-product proofs (what bpmi_ipa_prove_batch writes) on its way through the preparation
// (bpmi_ipa_batch_prepare, bpmi_ipa_batch_prepare_dev) and the whole verification (bpmi_ipa_verify_batch_packed_dev): the argument
// errors with their messages, the extra pairs a proof brings, and the upload regions -- the packed arrays, the offsets, the
// weights, the verdicts and the transposed transcripts -- laid out BEHIND the regions of the unchanged ipa_batch_plan, whose
// records, extra points and extra scalars the preparation kernels write in place.  tests/test_ipa_packed_plan_cpu.py checks it
// without a GPU; ipa_packed_dev_host.hpp consumes it.  Host twin: ipa_packed_host.hpp; kernels: ipa_packed_kernels.hpp.
#pragma once
#include "ipa_batch_plan_host.hpp"

#define IPAP_ROLES 4u                                 // waves per 64 proofs of k_ipap_roles, one per kind of chain
#define IPAP_MAX_TRANSCRIPT (1u << 17)                // a longer transcript is an invalid proof (the prover's longest: a 65 535-byte seed at k = 22)
#define IPAP_TRANSCRIPTS_MAX (1ull << 32)             // bytes of all transcripts of a call
#define IPAP_T_BYTES_MAX (1ull << 28)                 // the transposed transcripts of ONE launch; more proofs run as further launches
#define IPAP_T_PAD_WORDS 16u                          // zero words behind a transcript: the item walkers load up to 80 bytes past its end

// the packed proof form and the statements (include/bpmi.h); host pointers
struct IpaPackedIn {
  const uint8_t *ab = nullptr, *xs = nullptr, *LR = nullptr, *transcripts = nullptr;
  const uint64_t *tr_off = nullptr;
  const uint32_t *start = nullptr;
  const uint8_t *u = nullptr, *P = nullptr, *c = nullptr, *head = nullptr;
  const uint8_t *weights = nullptr, *seed = nullptr;
};

static inline IpaPackedIn ipap_in(const uint8_t *ab, const uint8_t *xs, const uint8_t *LR, const uint8_t *transcripts, const uint64_t *tr_off, const uint32_t *start,
                                  const uint8_t *u, const uint8_t *P, const uint8_t *c, const uint8_t *head, const uint8_t *weights, const uint8_t *seed) {
  IpaPackedIn in;
  in.ab = ab; in.xs = xs; in.LR = LR; in.transcripts = transcripts; in.tr_off = tr_off; in.start = start;
  in.u = u; in.P = P; in.c = c; in.head = head; in.weights = weights; in.seed = seed;
  return in;
}

static inline u32 ipap_pairs(u32 k, int protocol) { return 2u * k + (protocol == 1 ? 4u : 2u); }       // extra pairs of one proof
static inline u32 ipap_weights(int protocol) { return protocol == 1 ? 3u : 1u; }                       // explicit weights of one proof

// The upload regions of ONE class of proofs of one k (a whole uniform call, or a class of a mixed one): byte offsets into
// ctx->stage_in and sizes, every region on a 256-byte line
//   ab 64 P | xs 32 k P | LR 128 k P | transcripts (+ 8 bytes the transpose may read) | tr_off 8 (P + 1) | start 4 P (Protocol 2 with starts) |
//   u 64 P or 64 | P 64 P | c 32 P | head 128 P (Protocol 1) | weights 32 P or 96 P (explicit) | role verdicts 4 P
// and T, 8 W rows: the transposed transcripts of one launch, which the owner sizes (its rows) and places (behind its status)
struct IpapRegions {
  uint64_t o_ab = 0, o_xs = 0, o_lr = 0, o_tr = 0, o_troff = 0, o_start = 0, o_u = 0, o_P = 0, o_c = 0, o_head = 0, o_w = 0, o_roles = 0, o_T = 0;
  uint64_t b_ab = 0, b_xs = 0, b_lr = 0, b_tr = 0, b_troff = 0, b_start = 0, b_u = 0, b_P = 0, b_c = 0, b_head = 0, b_w = 0, b_roles = 0, b_T = 0;
};
// the sizes, all but b_T
static inline void ipap_region_sizes(IpapRegions &r, u32 k, int protocol, uint64_t n_proofs, bool has_start, bool has_weights, uint64_t tr_bytes) {
  r.b_ab = 64 * n_proofs; r.b_xs = 32ull * k * n_proofs; r.b_lr = 128ull * k * n_proofs;
  r.b_tr = tr_bytes + 8; r.b_troff = 8 * (n_proofs + 1); r.b_start = has_start ? 4 * n_proofs : 0;
  r.b_u = protocol == 1 ? 64 : 64 * n_proofs; r.b_P = 64 * n_proofs;
  r.b_c = protocol == 1 ? 32 * n_proofs : 0; r.b_head = protocol == 1 ? 128 * n_proofs : 0;
  r.b_w = has_weights ? 32ull * ipap_weights(protocol) * n_proofs : 0;
  r.b_roles = IPAP_ROLES * n_proofs;
}
// ab .. role verdicts in this order behind the cursor (take(bytes): the offset of the next region of `bytes`)
template <class Take> static inline void ipap_place_regions(IpapRegions &r, Take &take) {
  r.o_ab = take(r.b_ab); r.o_xs = take(r.b_xs); r.o_lr = take(r.b_lr); r.o_tr = take(r.b_tr); r.o_troff = take(r.b_troff); r.o_start = take(r.b_start);
  r.o_u = take(r.b_u); r.o_P = take(r.b_P); r.o_c = take(r.b_c); r.o_head = take(r.b_head); r.o_w = take(r.b_w); r.o_roles = take(r.b_roles);
}

struct IpapPlan : IpapRegions {
  int err = 0; const char *msg = nullptr;      // an argument error: nothing else is set
  IpabPlan base;                               // the unchanged plan: SA, SB, records, tables, partial sums, extra pairs (, scale)
  int protocol = 0;
  u32 pairs = 0;                               // extra pairs per proof
  uint64_t tr_bytes = 0;                       // all transcripts
  u32 longest = 0;                             // the longest transcript, cut at IPAP_MAX_TRANSCRIPT
  u32 W = 0;                                   // 8-byte rows of the transposed array: ceil(longest / 8) + IPAP_T_PAD_WORDS
  u32 rows = 0;                                // proofs per launch of the preparation kernels (a multiple of 64, or all)
  // behind base.total_bytes: the regions ab .. role verdicts | status P | T 8 W rows
  uint64_t o_status = 0, b_status = 0;
  uint64_t total_bytes = 0;
};

static inline IpapPlan ipap_plan_error(const char *msg) { IpapPlan p; p.err = BPMI_E_ARG; p.msg = msg; return p; }

// has_scale: as ipa_batch_plan (0 for the preparation alone).  Reads in.tr_off[0 .. n_proofs] and nothing else of the arrays.
static inline IpapPlan ipa_packed_plan(const BpmiOptions &opt, u32 k, int protocol, uint64_t n_proofs, const IpaPackedIn &in, int has_scale) {
  if (protocol != 1 && protocol != 2) return ipap_plan_error("protocol must be 1 or 2");
  if (k > IPAB_K_MAX) return ipap_plan_error("n must be 2^k, k <= 22");
  if (!in.ab || !in.transcripts || !in.tr_off || !in.u || !in.P || (k && (!in.xs || !in.LR))) return ipap_plan_error("null argument (xs and LR may be NULL only at k = 0)");
  if (protocol == 1 && (!in.c || !in.head)) return ipap_plan_error("protocol 1 needs c and head");
  if (protocol == 1 && in.start) return ipap_plan_error("start must be NULL under protocol 1 (the rounds begin at item 3)");
  if (protocol == 2 && (in.c || in.head)) return ipap_plan_error("c and head must be NULL under protocol 2");
  if (!in.weights && !in.seed) return ipap_plan_error("weights or a 32-byte seed");
  const u32 pairs = ipap_pairs(k, protocol);
  if (n_proofs <= IPAB_PROOFS_MAX && n_proofs * pairs > IPAB_EXTRA_MAX) return ipap_plan_error("at most 2^22 extra points per call");
  IpapPlan p;
  p.base = ipa_batch_plan(opt, 1ull << k, n_proofs, n_proofs <= IPAB_PROOFS_MAX ? n_proofs * pairs : 0, has_scale);
  if (p.base.err) return ipap_plan_error(p.base.msg);
  uint64_t longest = 0;
  for (uint64_t i = 0; i < n_proofs; i++) {
    if (in.tr_off[i + 1] < in.tr_off[i]) return ipap_plan_error("tr_off must not decrease");
    const uint64_t len = in.tr_off[i + 1] - in.tr_off[i];
    if (len > longest) longest = len;
  }
  if (in.tr_off[n_proofs] - in.tr_off[0] > IPAP_TRANSCRIPTS_MAX) return ipap_plan_error("at most 4 GiB of transcripts per call");
  p.protocol = protocol; p.pairs = pairs;
  p.tr_bytes = in.tr_off[n_proofs] - in.tr_off[0];
  p.longest = (u32)(longest < IPAP_MAX_TRANSCRIPT ? longest : IPAP_MAX_TRANSCRIPT);
  p.W = (p.longest + 7u) / 8u + IPAP_T_PAD_WORDS;
  uint64_t rows = IPAP_T_BYTES_MAX / (8ull * p.W) / 64 * 64;
  p.rows = (u32)(rows < n_proofs ? rows : n_proofs);
  ipap_region_sizes(p, k, protocol, n_proofs, in.start != nullptr, in.weights != nullptr, p.tr_bytes);
  p.b_status = n_proofs;
  p.b_T = 8ull * p.W * p.rows;
  uint64_t at = p.base.total_bytes;
  auto take = [&at](uint64_t bytes) { const uint64_t o = at; at += align_up(bytes, 256); return o; };
  ipap_place_regions(p, take);
  p.o_status = take(p.b_status); p.o_T = take(p.b_T);
  p.total_bytes = at;
  return p;
}
