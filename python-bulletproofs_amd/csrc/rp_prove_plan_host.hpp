// rp_prove_plan_host.hpp -- part of libbpmi; plain C++17 (no HIP, no bpmi_ctx), also compiled for the host by tests/csrc_host.
// The plan of a batched range-proof prover as a pure function of (bits per value, values per proof, option values): the argument
// errors, the block size of the n-lanes-per-proof kernels, the window bits and the size of the fixed-base tables, the per-call caps
// and the base lists of every job kind.  tests/test_rp_prove_plan_cpu.py checks it without a GPU; rp_prove_host.hpp consumes it.
#pragma once
#include <vector>

#include "shared_defs.hpp"

#define PROVER_ELEMS_MAX 1024u                 // elements of a proof's vectors (bits x values): one lane each in a block of at most 1 024 threads
#define PROVER_ELEMS_SMALL 128u                // up to here: 16-bit table windows, 16 lanes per job -- the shapes of rounds 5 and 6, unchanged
#define PROVER_TW_DEFAULT 16u                  // 16 additions per term, 4.4 GB and 72 ms to build for 64-bit proofs (profiles/r06_batch_prover_table_bits.txt); 12: 22 additions, 378 MB, 17 ms
#define PROVER_PROOFS_MAX (1ull << 20)         // proofs per call
#define PROVER_BATCH_ELEMS_MAX (1ull << 27)    // proofs x elements per call: 2^20 proofs of 128 elements; the scratch is ~256 B per element
#define PROVER_COMMIT_MAX (1ull << 24)         // commitments per call of bpmi_rp_prover_commit_batch
// k_pv_msm<6> against <4>, measured over 2^4 .. 2^12 proofs of 256 / 512 / 1 024 elements (profiles/r07_batch_prover_wide.txt): a
// wave per job is 2-3 x faster up to 2^9 proofs, where 16 lanes per job leave most SIMDs without a wave, and still 2-8 % ahead in
// launches of 4 096 jobs; at 8 192 jobs (the rounds of 2^12 proofs) 16 lanes are level (512, 1 024 elements) or 11 % ahead (256)
#define PROVER_WAVE_JOBS_MAX 4096u

struct RppPlan {
  int err = 0; const char *msg = nullptr;      // an argument error: nothing else is set
  u32 nb = 0, m = 0, n = 0, k = 0;             // bits per value, values per proof, n = nb m elements, k = log2 n rounds
  u32 NT = 0, per_block = 0;                   // threads of a block of the n-lanes-per-proof kernels, proofs it holds
  u32 nbases = 0;                              // 3 + 2n: g, h, u, gs, hs
  u32 tw = 0, wt = 0, bt = 0;                  // table windows: tw bits, wt = ceil(256 / tw) per scalar, bt = 2^(tw-1) entries each
  uint64_t table_bytes = 0;
  uint64_t max_proofs = 0;                     // per call: min(2^20, 2^27 / n)
  // the base lists, in entries of `bases`: S and P_new 2n + 1 (gs_0.., hs_0.., then h / u), T 2 (g, h), round r: L then R, n + 1 each
  u32 off_S = 0, off_T = 0, off_P = 0, off_round = 0;
  std::vector<unsigned short> bases;
};

// nbases bases x ceil(256 / w) windows x 2^(w-1) entries of 64 bytes (the range prover: 3 + 2 elems bases; ipa_prove_plan_host.hpp: 1 + 2 elems)
static inline uint64_t rpp_table_bytes_of(u32 nbases, u32 w) { return (uint64_t)nbases * ((256 + w - 1) / w) * ((uint64_t)1 << (w - 1)) * 64; }
static inline uint64_t rpp_table_bytes(u32 elems, u32 w) { return rpp_table_bytes_of(3 + 2 * elems, w); }
// Window bits under option "prover_table_bits" = 0.  Up to 128 elements: 16.  Above: the widest width whose table is no larger than
// the largest one of those -- 128 elements at 16 bits, 8.7 GB (256 elements: 14 bits, 5.1 GB; 16 bits would be 69 GB at 1 024)
static inline u32 rpp_default_table_bits(u32 elems) {
  if (elems <= PROVER_ELEMS_SMALL) return PROVER_TW_DEFAULT;
  const uint64_t bound = rpp_table_bytes(PROVER_ELEMS_SMALL, PROVER_TW_DEFAULT);
  for (u32 w = 16; w > 4; w--) if (rpp_table_bytes(elems, w) <= bound) return w;
  return 4;
}

static inline RppPlan rpp_plan_error(const char *msg) { RppPlan p; p.err = BPMI_E_ARG; p.msg = msg; return p; }

// opt_tw: option "prover_table_bits" (0, or 4 .. 16: bpmi_set_option checks it)
static inline RppPlan rpp_plan(uint32_t nbits, uint32_t m, int opt_tw) {
  if (nbits < 1 || nbits > 128 || (nbits & (nbits - 1)) || m < 1 || (m & (m - 1)) || (uint64_t)nbits * m < 2 || (uint64_t)nbits * m > PROVER_ELEMS_MAX)
    return rpp_plan_error("the bit width (at most 128) and the number of values must be powers of two with 2 <= bits x values <= 1024");
  RppPlan p;
  p.nb = nbits; p.m = m; p.n = nbits * m;
  while ((1u << p.k) < p.n) p.k++;
  const u32 n = p.n;
  p.NT = n <= 256u ? 256u : n;                                   // 256, 512 or 1 024: a proof never straddles blocks
  p.per_block = p.NT / n;
  p.nbases = 3 + 2 * n;
  p.tw = opt_tw ? (u32)opt_tw : rpp_default_table_bits(n);
  p.wt = (256u + p.tw - 1u) / p.tw; p.bt = 1u << (p.tw - 1u);
  p.table_bytes = rpp_table_bytes(n, p.tw);
  p.max_proofs = PROVER_BATCH_ELEMS_MAX / n < PROVER_PROOFS_MAX ? PROVER_BATCH_ELEMS_MAX / n : PROVER_PROOFS_MAX;
  // base lists: S / P_new: gs_0.., hs_0.., then h (S) or u (P_new); T: g, h; round r: L then R (rp_prove_kernels.hpp k_pv_round_wide)
  std::vector<unsigned short> &bl = p.bases;
  bl.reserve((size_t)(2 * (2 * n + 1) + 2) + (size_t)p.k * 2 * (n + 1));
  p.off_S = 0;
  for (u32 i = 0; i < n; i++) bl.push_back((unsigned short)(3 + i));
  for (u32 i = 0; i < n; i++) bl.push_back((unsigned short)(3 + n + i));
  bl.push_back(1);
  p.off_T = (u32)bl.size();
  bl.push_back(0); bl.push_back(1);
  p.off_P = (u32)bl.size();
  for (u32 i = 0; i < n; i++) bl.push_back((unsigned short)(3 + i));
  for (u32 i = 0; i < n; i++) bl.push_back((unsigned short)(3 + n + i));
  bl.push_back(2);
  p.off_round = (u32)bl.size();
  for (u32 r = 0; r < p.k; r++) {
    const u32 len = n >> r, half = len >> 1;
    for (int side = 0; side < 2; side++) {               // 0: L, 1: R
      for (u32 j = 0; j < n; j++) if (((j & (len - 1)) >= half) == (side == 0)) bl.push_back((unsigned short)(3 + j));
      for (u32 j = 0; j < n; j++) if (((j & (len - 1)) < half) == (side == 0)) bl.push_back((unsigned short)(3 + n + j));
      bl.push_back(2);
    }
  }
  return p;
}

// the per-call caps of bpmi_rp_prove_batch (max_proofs: the plan's): nullptr, or the text of the BPMI_E_ARG (checked before anything is allocated)
static inline const char *rpp_batch_error(uint64_t max_proofs, uint64_t n_proofs) {
  if (n_proofs > PROVER_PROOFS_MAX) return "at most 2^20 proofs per call";
  if (n_proofs > max_proofs) return "at most 2^27 elements (proofs x bits x values) per call";
  return nullptr;
}

// log2 of the lanes k_pv_msm gives a job: 4, or 6 (a wave).  opt: option "prover_job_lanes" (0 automatic, 16, 64).  Automatic: 16 for
// proofs of up to 128 elements whatever the batch; above, a wave while the launch has at most PROVER_WAVE_JOBS_MAX jobs
static inline int rpp_job_lanes_log2(u32 elems, uint64_t njobs, int opt) {
  if (opt == 16) return 4;
  if (opt == 64) return 6;
  return elems > PROVER_ELEMS_SMALL && njobs <= PROVER_WAVE_JOBS_MAX ? 6 : 4;
}
