// ipa_batch_plan_host.hpp -- part of libbpmi; plain C++17 (no HIP, no bpmi_ctx), also compiled for the host by tests/csrc_host.
// The plan of a batch of inner-product verifications over shared generators (bpmi_sc_svector_sum, bpmi_ipa_verify_batch_dev) as a
// pure function of the sizes: the argument errors, the split of the index, the number of proof ranges ("parts") of the summing
// kernel, the layout of the workspace in ctx->stage_in and the pair count of the one MSM.  tests/test_ipa_batch_plan_cpu.py checks
// it without a GPU; ipa_batch_host.hpp consumes it.  Kernels: scalar_kernels.hpp (k_sc_svector_tables_batch, k_sc_svector_sum,
// k_sc_svector_sum_finish) over the bodies of svector_batch.hpp.
#pragma once
#include "shared_defs.hpp"

#define IPAB_K_MAX 22u                         // n = 2^k, what bpmi_ipa_verify_dev takes
#define IPAB_PROOFS_MAX (1ull << 16)           // proofs per call
#define IPAB_WORK_MAX (1ull << 32)             // proofs x n per call: (proof, element) products of the summing kernel
#define IPAB_TABLE_BYTES_MAX (1ull << 30)      // the half tables of all proofs
#define IPAB_EXTRA_MAX (1ull << 22)            // extra (point, scalar) pairs of all proofs together
#define IPAB_SIMDS 1024u                       // SIMDs of the chip (256 CUs x 4): the summing kernel wants a wave on each
#define IPAB_THREADS 256u                      // threads of a block of the three kernels
#define IPAB_TABLE_GRID_Y 32768u               // k_sc_svector_tables_batch: proof = blockIdx.y + IPAB_TABLE_GRID_Y * blockIdx.z (a grid's y is < 2^16)

// The rule for `parts`.  k_sc_svector_sum runs one lane per element i, so a launch over the n elements alone has ceil(n / 64)
// waves: 16 at n = 1 024, however many proofs it sums.  blockIdx.y therefore splits the proofs into `parts` ranges, each with its
// own partial sums, so that the launch has at least one wave per SIMD where the number of proofs allows it:
//   waves    = ceil(n / 64)
//   want     = ceil(IPAB_SIMDS / waves)              ranges that bring the launch to 1 024 waves
//   per_part = ceil(n_proofs / min(want, n_proofs))  proofs of a range
//   parts    = ceil(n_proofs / per_part)             no range is empty; range j is [j per_part, min((j + 1) per_part, n_proofs))
// n >= 2^16 gives parts = 1; with one range and no shared scale the summing kernel writes SA and SB itself (`direct`), there are
// no partial sums and k_sc_svector_sum_finish is not launched.
struct IpabPlan {
  int err = 0; const char *msg = nullptr;      // an argument error: nothing else is set
  u32 k = 0, kl = 0, kh = 0;                   // n = 2^k; the index splits as i = hi 2^kl + lo, kl = k / 2, kh = k - kl
  uint64_t n = 0, n_proofs = 0, n_extra = 0;
  uint64_t tab_entries = 0;                    // per proof: 2^kl + 2^kh records of 64 bytes
  u32 rec_words = 0;                           // per proof: k pairs (x_j, x_j^-1), then a, b, w: 16 k + 24 words
  u32 parts = 0, per_part = 0;
  bool direct = false;
  // the workspace: byte offsets into ctx->stage_in, every region on a 256-byte line
  //   SA 32 n | SB 32 n | records 4 rec_words n_proofs | tables 64 tab_entries n_proofs | partial sums 2 x 32 n parts (none when direct) |
  //   extra points 64 n_extra | extra scalars 32 n_extra | scale 32 n (only when the scale comes from the host: has_scale = 2)
  uint64_t o_sa = 0, o_sb = 0, o_rec = 0, o_tab = 0, o_part = 0, o_expt = 0, o_exsc = 0, o_scale = 0;
  uint64_t b_sa = 0, b_sb = 0, b_rec = 0, b_tab = 0, b_part = 0, b_expt = 0, b_exsc = 0, b_scale = 0;
  uint64_t total_bytes = 0;
  uint64_t msm_pairs = 0;                      // 2 n + n_extra
};

static inline IpabPlan ipab_plan_error(const char *msg) { IpabPlan p; p.err = BPMI_E_ARG; p.msg = msg; return p; }

// n_extra: the extra pairs of ALL proofs (a Protocol-2 proof brings 2 k + 2, one that came through Protocol 1 five more).
// has_scale: 0 none, 1 a shared scale that is in device memory already, 2 one that is staged from the host (bpmi_sc_svector_sum).
// No option changes the plan today; the parameter keeps the signature of the other planners.
static inline IpabPlan ipa_batch_plan(const BpmiOptions &, uint64_t n, uint64_t n_proofs, uint64_t n_extra, int has_scale) {
  u32 k;
  if (!log2_exact(n, k) || k > IPAB_K_MAX) return ipab_plan_error("n must be 2^k, k <= 22");
  if (n_proofs < 1 || n_proofs > IPAB_PROOFS_MAX) return ipab_plan_error("between 1 and 2^16 proofs per call");
  if (n_proofs * n > IPAB_WORK_MAX) return ipab_plan_error("at most 2^32 elements (proofs x n) per call");
  const u32 kl = k / 2, kh = k - kl;
  const uint64_t tab_entries = (1ull << kl) + (1ull << kh);
  if (64 * tab_entries * n_proofs > IPAB_TABLE_BYTES_MAX) return ipab_plan_error("the half tables of the batch (proofs x 64 (2^(k/2) + 2^(k - k/2)) bytes) exceed 1 GiB");
  if (n_extra > IPAB_EXTRA_MAX) return ipab_plan_error("at most 2^22 extra points per call");
  IpabPlan p;
  p.k = k; p.kl = kl; p.kh = kh; p.n = n; p.n_proofs = n_proofs; p.n_extra = n_extra;
  p.tab_entries = tab_entries;
  p.rec_words = 16u * k + 24u;
  const uint64_t waves = (n + 63) / 64, want = (IPAB_SIMDS + waves - 1) / waves;
  const uint64_t ranges = want < n_proofs ? want : n_proofs;
  p.per_part = (u32)((n_proofs + ranges - 1) / ranges);
  p.parts = (u32)((n_proofs + p.per_part - 1) / p.per_part);
  p.direct = p.parts == 1 && !has_scale;
  p.b_sa = p.b_sb = 32 * n;
  p.b_rec = 4ull * p.rec_words * n_proofs;
  p.b_tab = 64 * tab_entries * n_proofs;
  p.b_part = p.direct ? 0 : 2 * 32 * n * p.parts;
  p.b_expt = 64 * n_extra; p.b_exsc = 32 * n_extra;
  p.b_scale = has_scale == 2 ? 32 * n : 0;
  uint64_t at = 0;
  auto take = [&at](uint64_t bytes) { const uint64_t o = at; at += align_up(bytes, 256); return o; };
  p.o_sa = take(p.b_sa); p.o_sb = take(p.b_sb); p.o_rec = take(p.b_rec); p.o_tab = take(p.b_tab); p.o_part = take(p.b_part);
  p.o_expt = take(p.b_expt); p.o_exsc = take(p.b_exsc); p.o_scale = take(p.b_scale);
  p.total_bytes = at;
  p.msm_pairs = 2 * n + n_extra;
  return p;
}
