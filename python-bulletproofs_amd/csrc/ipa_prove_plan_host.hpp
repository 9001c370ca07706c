// ipa_prove_plan_host.hpp -- part of libbpmi; plain C++17 (no HIP, no bpmi_ctx), also compiled for the host by tests/csrc_host.
// The plan of a batched inner-product prover as a pure function of (vector length, option values): the argument errors, the block
// size of the n-lanes-per-proof kernel, the window bits and the size of the fixed-base tables, the per-call caps, the bound of a
// proof's transcript text and the base lists of every job kind -- at the end those of the statements call (ipp_commit_error,
// ipp_commit_bases; tests/test_ipa_commit_plan_cpu.py).  tests/test_ipa_prove_plan_cpu.py checks it without a GPU;
// ipa_prove_host.hpp consumes it.  The geometry is the range prover's (rp_prove_plan_host.hpp): the same tables over 2n + 1 bases
// instead of 2n + 3, the same block sizes, caps and job-lane rule.
#pragma once
#include <vector>

#include "rp_prove_plan_host.hpp"

#define IPP_SEED_MAX 0xFFFFull                 // bytes of a proof's seed (Protocol 1) or transcript prefix (Protocol 2)
#define IPP_NUMBER_TEXT 79u                    // a scalar in a transcript: up to 78 decimal digits (q - 1 has 78) and '&'
#define IPP_POINT_TEXT 45u                     // a point: base64 of its 33 compressed bytes (44 characters) and '&'; the identity is "AA==&"

struct IppPlan {
  int err = 0; const char *msg = nullptr;      // an argument error: nothing else is set
  u32 n = 0, k = 0;                            // elements of a proof's vectors, k = log2 n rounds
  u32 NT = 0, per_block = 0;                   // threads of a block of the n-lanes-per-proof kernel, proofs it holds
  u32 nbases = 0;                              // 1 + 2n: u, g_0.., h_0..
  u32 tw = 0, wt = 0, bt = 0;                  // table windows: tw bits, wt = ceil(256 / tw) per scalar, bt = 2^(tw-1) entries each
  uint64_t table_bytes = 0;
  uint64_t max_proofs = 0;                     // per call: min(2^20, 2^27 / n)
  // the base lists, in entries of `bases`: the head's one term (u), then round r: L then R, n + 1 each
  u32 off_head = 0, off_round = 0;
  std::vector<unsigned short> bases;
};

static inline IppPlan ipp_plan_error(const char *msg) { IppPlan p; p.err = BPMI_E_ARG; p.msg = msg; return p; }

// The base lists of a proof of n elements over the first n of N generators each (n = N: a prover of its own; n < N: a class of a
// capacity, ipa_prove_mixed_plan_host.hpp): u = 0, g_j = 1 + j, h_j = 1 + N + j -- the capacity enters in the base of h_j and nowhere
// else.  The head's one term (u) at entry 0, then from entry 1 round r: L then R, n + 1 each, by the rule of rpp_plan: L holds the g_j
// with (j mod len) >= half, then the h_j with (j mod len) < half, then u; R the complements (ipa_prove_kernels.hpp k_ip_round_wide)
static inline size_t ipp_class_bases_len(u32 n) {
  u32 k = 0;
  while ((1u << k) < n) k++;
  return 1 + (size_t)k * 2 * (n + 1);
}
static inline std::vector<unsigned short> ipp_class_bases(u32 n, u32 N) {
  std::vector<unsigned short> bl;
  bl.reserve(ipp_class_bases_len(n));
  bl.push_back(0);
  for (u32 len = n; len > 1; len >>= 1) {
    const u32 half = len >> 1;
    for (int side = 0; side < 2; side++) {               // 0: L, 1: R
      for (u32 j = 0; j < n; j++) if (((j & (len - 1)) >= half) == (side == 0)) bl.push_back((unsigned short)(1 + j));
      for (u32 j = 0; j < n; j++) if (((j & (len - 1)) < half) == (side == 0)) bl.push_back((unsigned short)(1 + N + j));
      bl.push_back(0);
    }
  }
  return bl;
}

// opt_tw: option "prover_table_bits" (0, or 4 .. 16: bpmi_set_option checks it)
static inline IppPlan ipp_plan(uint32_t n, int opt_tw) {
  if (n < 1 || n > PROVER_ELEMS_MAX || (n & (n - 1)))
    return ipp_plan_error("the vector length must be a power of two with 1 <= n <= 1024 (longer vectors: the single-proof prover)");
  IppPlan p;
  p.n = n;
  while ((1u << p.k) < n) p.k++;
  p.NT = n <= 256u ? 256u : n;                                   // 256, 512 or 1 024: a proof never straddles blocks
  p.per_block = p.NT / n;
  p.nbases = 1 + 2 * n;
  p.tw = opt_tw ? (u32)opt_tw : rpp_default_table_bits(n);
  p.wt = (256u + p.tw - 1u) / p.tw; p.bt = 1u << (p.tw - 1u);
  p.table_bytes = rpp_table_bytes_of(p.nbases, p.tw);
  p.max_proofs = PROVER_BATCH_ELEMS_MAX / n < PROVER_PROOFS_MAX ? PROVER_BATCH_ELEMS_MAX / n : PROVER_PROOFS_MAX;
  p.off_head = 0;
  p.off_round = 1;
  p.bases = ipp_class_bases(n, n);
  return p;
}

// the per-call caps of bpmi_ipa_prove_batch (max_proofs: the plan's): nullptr, or the text of the BPMI_E_ARG
static inline const char *ipp_batch_error(uint64_t max_proofs, uint64_t n_proofs) {
  if (n_proofs > PROVER_PROOFS_MAX) return "at most 2^20 proofs per call";
  if (n_proofs > max_proofs) return "at most 2^27 elements (proofs x n) per call";
  return nullptr;
}

// which arrays a call hands in (true: non-NULL)
struct IppCall {
  int protocol = 0;
  bool a = false, b = false, c = false, P = false, seed_off = false, ab = false, xs = false, LR = false, head = false, transcripts = false, tr_off = false;
};
// nullptr, or the text of the BPMI_E_ARG: the protocol, NULL where an array is required, non-NULL where it must be NULL.  k: rounds
// (a proof of one element has no xs and no L, R: those two may be NULL then)
static inline const char *ipp_call_error(u32 k, const IppCall &c) {
  if (c.protocol != 1 && c.protocol != 2) return "protocol must be 1 or 2";
  if (!c.a || !c.b || !c.seed_off || !c.ab || !c.transcripts || !c.tr_off || (k && (!c.xs || !c.LR))) return "null argument";
  if (c.protocol == 1 && (!c.P || !c.head)) return "null argument (Protocol 1 takes P and writes head)";
  if (c.protocol == 2 && (c.c || c.P || c.head)) return "c, P and head must be NULL under Protocol 2 (its prover never reads P)";
  return nullptr;
}

// the longest text the transcript of a proof can reach (its final digest, transcript.py:13-33):
//   Protocol 1:  "&" base64(seed) "&" str(x) "&"  then per round  L "&" R "&" str(x_r) "&"
//   Protocol 2:  "&" prefix                       then per round  the same
static inline uint64_t ipp_transcript_bytes(u32 k, int protocol, uint64_t seed_len) {
  const uint64_t start = protocol == 1 ? 1 + ((seed_len + 2) / 3) * 4 + 1 + IPP_NUMBER_TEXT : 1 + seed_len;
  return start + (uint64_t)k * (2 * IPP_POINT_TEXT + IPP_NUMBER_TEXT);
}

// the seeds of a call: nullptr, or the text of the BPMI_E_ARG; *longest <- the longest seed
static inline const char *ipp_seeds_error(uint64_t n_proofs, const uint64_t *seed_off, bool have_seeds, uint64_t *longest) {
  uint64_t mx = 0;
  for (uint64_t p = 0; p < n_proofs; p++) {
    if (seed_off[p + 1] < seed_off[p]) return "seed offsets must not decrease";
    const uint64_t sl = seed_off[p + 1] - seed_off[p];
    if (sl > IPP_SEED_MAX) return "a seed is longer than 65535 bytes";
    if (sl > mx) mx = sl;
  }
  if (!have_seeds && mx) return "null argument (seeds)";
  *longest = mx;
  return nullptr;
}
static inline const char *ipp_cap_error(u32 k, int protocol, uint64_t n_proofs, uint64_t longest, uint64_t cap) {
  return cap < n_proofs * ipp_transcript_bytes(k, protocol, longest) ? "the transcript buffer is too small (n_proofs x bpmi_ipa_prove_batch_transcript_bytes of the longest seed)" : nullptr;
}

// log2 of the lanes k_pv_msm gives a job: the range prover's rule (rpp_job_lanes_log2), a round's launch has 2 x proofs jobs
static inline int ipp_job_lanes_log2(u32 n, uint64_t njobs, int opt) { return rpp_job_lanes_log2(n, njobs, opt); }

// ---- the statements of a batch (bpmi_ipa_batch_prover_commit_batch): out[p] = sum a_p[j] g_j + sum b_p[j] (c_j h_j) + t_p u -------------
// which arrays a call hands in (true: non-NULL), and its u_mode: 0 no u term, 1 t_p = <a_p, b_p> summed on the device, 2 t given
struct IppCommitCall {
  bool pv = false, out = false, a = false, b = false, t = false;
  int u_mode = 0;
};
// nullptr, or the text of the BPMI_E_ARG: the NULL rules and u_mode, before anything is read
static inline const char *ipp_commit_error(const IppCommitCall &c) {
  if (!c.pv) return "null argument (pv)";
  if (!c.out) return "null argument (out)";
  if (c.u_mode < 0 || c.u_mode > 2) return "u_mode must be 0 (no u term), 1 (t = <a, b>) or 2 (t given)";
  if (c.u_mode != 2 && c.t) return "t must be NULL unless u_mode is 2";
  if (c.u_mode == 2 && !c.t) return "null argument (u_mode 2 takes t)";
  if (!c.a && !c.b) return "a and b are both NULL (one of them may be: all zeros)";
  if (c.u_mode == 1 && (!c.a || !c.b)) return "u_mode 1 sums <a, b>: it takes both a and b";
  return nullptr;
}
// the base list of a statement's job: g_0 .. g_(n-1) (bases 1 + j) when a is given, h_0 .. h_(n-1) (1 + n + j) when b is, then u (0)
// LAST: of 2n + 1 terms it is the one that does not fill a round of the job's 16 lanes, the remainder term k_pv_msm shares out by
// windows.  A NULL half is dropped from the list, not multiplied by zero.
// N: the generators of the prover's table (h_j at base 1 + N + j); N = n unless the statements are a class of a capacity
static inline std::vector<unsigned short> ipp_commit_class_bases(u32 n, u32 N, bool have_a, bool have_b, bool have_u) {
  std::vector<unsigned short> bl;
  bl.reserve((size_t)n * ((have_a ? 1u : 0u) + (have_b ? 1u : 0u)) + (have_u ? 1u : 0u));
  if (have_a) for (u32 j = 0; j < n; j++) bl.push_back((unsigned short)(1 + j));
  if (have_b) for (u32 j = 0; j < n; j++) bl.push_back((unsigned short)(1 + N + j));
  if (have_u) bl.push_back(0);
  return bl;
}
static inline std::vector<unsigned short> ipp_commit_bases(u32 n, bool have_a, bool have_b, bool have_u) { return ipp_commit_class_bases(n, n, have_a, have_b, have_u); }
// the device copy: the lists (a, b, u), (a, u), (b, u) one after the other; a call without a u term takes its list one entry short
static inline u32 ipp_commit_bases_offset(u32 n, bool have_a, bool have_b) { return have_a && have_b ? 0u : have_a ? 2u * n + 1u : 3u * n + 2u; }
static inline std::vector<unsigned short> ipp_commit_bases_all(u32 n, u32 N = 0) {
  if (!N) N = n;
  std::vector<unsigned short> all = ipp_commit_class_bases(n, N, true, true, true);
  const std::vector<unsigned short> a_only = ipp_commit_class_bases(n, N, true, false, true), b_only = ipp_commit_class_bases(n, N, false, true, true);
  all.insert(all.end(), a_only.begin(), a_only.end());
  all.insert(all.end(), b_only.begin(), b_only.end());
  return all;
}
