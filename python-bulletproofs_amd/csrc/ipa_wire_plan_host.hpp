// ipa_wire_plan_host.hpp -- part of libbpmi; plain C++17 (no HIP, no bpmi_ctx), also compiled for the host by tests/csrc_host.
// The plan of a batch of inner-product proofs in the wire format BPIP2 (include/bpmi.h; host twin and format: ipa_wire_host.hpp) on
// its way through the device expander (bpmi_ipa_wire_expand_dev) and the whole verification (bpmi_ipa_verify_batch_wire_dev): the
// argument errors with their messages, the wire region, the regions of the EXPANSION -- the packed arrays the kernels of
// ipa_wire_kernels.hpp write in device memory, described as an IpapRegions so that ipad::Params and the unchanged preparation
// kernels read them -- the rows W of the word-major transcript array and the proofs per launch under the T budget.  It reads
// off[0 .. n_proofs] and never a blob.  tests/test_ipa_wire_plan_cpu.py checks it without a GPU; ipa_wire_dev_host.hpp consumes it.
#pragma once
#include "ipa_packed_plan_host.hpp"

#define IPAW_HEAD 6u                                  // "BPIP2" | k
#define IPAW_ROUND_TEXT (45u + 45u + 79u)             // the longest text of one round: two point items and a 78-digit challenge, each with its '&'
#define IPAW_BLOBS_MAX (1ull << 32)                   // bytes of all blobs of a call
static inline uint64_t ipaw_fixed_bytes(u32 k) { return 78ull + 98ull * k; }                  // a blob without its prefix
static inline uint64_t ipaw_wire_bytes(u32 k, uint64_t prefix_len) { return ipaw_fixed_bytes(k) + prefix_len; }
static inline u32 ipaw_scalars_at() { return IPAW_HEAD; }
static inline u32 ipaw_points_at(u32 k) { return IPAW_HEAD + 32u * (2u + k); }
static inline u32 ipaw_start_at(u32 k) { return ipaw_points_at(k) + 66u * k; }
static inline u32 ipaw_prefix_at(u32 k) { return ipaw_start_at(k) + 8u; }
// the longest expansion a blob of `len` bytes can stand for, cut at the packed verifier's cap (a longer one is an invalid proof)
static inline uint64_t ipaw_expansion_bound(u32 k, uint64_t len) {
  const uint64_t fixed = ipaw_fixed_bytes(k);
  if (len < fixed) return 0;
  const uint64_t e = len - fixed + (uint64_t)IPAW_ROUND_TEXT * k;
  return e < IPAP_MAX_TRANSCRIPT ? e : IPAP_MAX_TRANSCRIPT;
}

struct IpaWireIn {
  const uint8_t *blobs = nullptr;
  const uint64_t *off = nullptr;
  const uint8_t *u = nullptr, *P = nullptr, *weights = nullptr, *seed = nullptr;
};

struct IpawPlan : IpapRegions {
  int err = 0; const char *msg = nullptr;      // an argument error: nothing else is set
  IpabPlan base;                               // verification only: SA, SB, records, tables, partial sums, extra pairs
  u32 k = 0, pairs = 0;
  uint64_t n_proofs = 0;
  uint64_t wire_bytes = 0;                     // all blobs: off[n_proofs] - off[0]
  uint64_t text_bound = 0;                     // sum of the proofs' expansion bounds: a transcripts buffer of this size holds every expansion
  u32 longest = 0;                             // the largest expansion bound
  u32 W = 0;                                   // 8-byte rows of the word-major array: ceil(longest / 8) + IPAP_T_PAD_WORDS
  u32 rows = 0;                                // proofs per launch (a multiple of 64, or all)
  // behind base.total_bytes: wire (+ 8) | off 8 (P + 1) | the regions ab .. role verdicts (no byte transcripts: b_tr holds nothing) |
  // lengths 4 P | wire verdicts 2 P (malformed, then undecodable point) | status P | T 8 W rows
  uint64_t o_wire = 0, b_wire = 0, o_off = 0, b_off = 0, o_lens = 0, b_lens = 0, o_flags = 0, b_flags = 0, o_status = 0, b_status = 0;
  uint64_t total_bytes = 0;
};

static inline IpawPlan ipaw_plan_error(const char *msg) { IpawPlan p; p.err = BPMI_E_ARG; p.msg = msg; return p; }

// verify: the statements and the weights are part of the call (bpmi_ipa_verify_batch_wire_dev); otherwise the expansion alone.
// t_budget: bytes of the T region of one launch (0: IPAP_T_BYTES_MAX; never fewer than 64 proofs per launch).
static inline IpawPlan ipa_wire_plan(const BpmiOptions &opt, u32 k, int protocol, uint64_t n_proofs, const IpaWireIn &in, bool verify, int has_scale, uint64_t t_budget) {
  if (protocol != 2) return ipaw_plan_error("the wire format holds Protocol-2 proofs only");
  if (k > IPAB_K_MAX) return ipaw_plan_error("n must be 2^k, k <= 22");
  if (!in.blobs || !in.off || (verify && (!in.u || !in.P))) return ipaw_plan_error("null argument");
  if (verify && !in.weights && !in.seed) return ipaw_plan_error("weights or a 32-byte seed");
  if (n_proofs < 1 || n_proofs > IPAB_PROOFS_MAX) return ipaw_plan_error("between 1 and 2^16 proofs per call");
  const u32 pairs = ipap_pairs(k, 2);
  IpawPlan p;
  if (verify) {                                  // (2^16 proofs x 46 pairs stay below the 2^22 extra points of a call)
    p.base = ipa_batch_plan(opt, 1ull << k, n_proofs, n_proofs * pairs, has_scale);
    if (p.base.err) return ipaw_plan_error(p.base.msg);
  }
  uint64_t longest = 0, bound = 0;
  for (uint64_t i = 0; i < n_proofs; i++) {
    if (in.off[i + 1] < in.off[i]) return ipaw_plan_error("off must not decrease");
    const uint64_t e = ipaw_expansion_bound(k, in.off[i + 1] - in.off[i]);
    bound += e;
    if (e > longest) longest = e;
  }
  if (in.off[n_proofs] - in.off[0] > IPAW_BLOBS_MAX) return ipaw_plan_error("at most 4 GiB of blobs per call");
  p.k = k; p.pairs = pairs; p.n_proofs = n_proofs;
  p.wire_bytes = in.off[n_proofs] - in.off[0];
  p.text_bound = bound;
  p.longest = (u32)longest;
  p.W = (p.longest + 7u) / 8u + IPAP_T_PAD_WORDS;
  const uint64_t budget = t_budget && t_budget < IPAP_T_BYTES_MAX ? t_budget : IPAP_T_BYTES_MAX;
  uint64_t rows = budget / (8ull * p.W) / 64 * 64;
  if (rows < 64) rows = 64;
  p.rows = (u32)(rows < n_proofs ? rows : n_proofs);
  ipap_region_sizes(p, k, 2, n_proofs, true, verify && in.weights != nullptr, 0);
  if (!verify) p.b_u = p.b_P = p.b_roles = 0;
  p.b_wire = p.wire_bytes + 8; p.b_off = 8 * (n_proofs + 1);
  p.b_lens = 4 * n_proofs; p.b_flags = 2 * n_proofs; p.b_status = n_proofs;
  p.b_T = 8ull * p.W * p.rows;
  uint64_t at = verify ? p.base.total_bytes : 0;
  auto take = [&at](uint64_t bytes) { const uint64_t o = at; at += align_up(bytes, 256); return o; };
  p.o_wire = take(p.b_wire); p.o_off = take(p.b_off);
  ipap_place_regions(p, take);
  p.o_lens = take(p.b_lens); p.o_flags = take(p.b_flags); p.o_status = take(p.b_status); p.o_T = take(p.b_T);
  p.total_bytes = at;
  return p;
}
