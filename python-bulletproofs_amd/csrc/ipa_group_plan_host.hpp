// ipa_group_plan_host.hpp -- part of libbpmi; plain C++17 (no HIP, no bpmi_ctx), also compiled for the host by tests/csrc_host.
// The plan of bpmi_ipa_group_values_packed_dev: a batch of PACKED inner-product proofs whose weighted combination is taken per GROUP
// of `group` consecutive proofs, so that one call says which groups hold an invalid proof.  It is the unchanged ipa_packed_plan (the
// uploads, the preparation's regions, the half tables; its plain SA / SB and partial sums are laid out and not used) followed by the
// groups' regions, every one on a 256-byte line:
//   rows SA[t][i] 32 n ngroups | rows SB[t][i] 32 n ngroups | E[t][w] 144 W ngroups (window sums, W windows of MID_C bits) | values 64 ngroups
// and the route of the groups' MSMs over [g | h | the group's extra pairs] by pairs = 2 n + group per (per = 2k + 2 under Protocol 2,
// 2k + 4 under Protocol 1): one launch of k_msm_ipa_group in its light shape (<= GROUP_LIGHT_NMAX) or its k_msm_mid shape
// (<= MID_NMAX), or msm_run group by group.  tests/test_ipa_group_plan_cpu.py checks it without a GPU; ipa_group_dev_host.hpp
// consumes it.  Kernels: k_sc_svector_sum_groups (scalar_kernels.hpp), k_msm_ipa_group (msm_kernels.hpp).
#pragma once
#include "ipa_packed_plan_host.hpp"

#define IPAG_ROWS_MAX (1ull << 26)             // group scalars of one array: ngroups x 2 n (the cap of bpmi_rp_batch_group_values_dev's rows)
#define IPAG_ROUTE_LIGHT 1u
#define IPAG_ROUTE_MID 2u
#define IPAG_ROUTE_MSM_RUN 3u

struct IpagPlan {
  int err = 0; const char *msg = nullptr;      // an argument error: nothing else is set
  IpapPlan packed;                             // the unchanged plan of the packed verifier (packed.rows: cut to the transposition budget)
  u32 group = 0, ngroups = 0;                  // proofs per group (at most the batch), groups
  u32 per = 0;                                 // extra pairs per proof
  u32 W = 0;                                   // windows of MID_C bits
  uint64_t pairs = 0;                          // 2 n + group per: the pairs of a full group's MSM
  u32 route = 0;
  uint64_t o_gsa = 0, o_gsb = 0, o_E = 0, o_vals = 0;
  uint64_t b_gsa = 0, b_gsb = 0, b_E = 0, b_vals = 0;
  uint64_t total_bytes = 0;
};

static inline IpagPlan ipag_plan_error(const char *msg) { IpagPlan p; p.err = BPMI_E_ARG; p.msg = msg; return p; }

// n: the generator count as the caller gave it; have_outputs: `values` and `status` are both there.  t_budget: bytes of one launch's
// transposed transcripts (IPAP_T_BYTES_MAX, or the test hook's value: fewer proofs per preparation launch, never fewer than 64).
// Reads in.tr_off[0 .. n_proofs] and nothing else of the arrays, and only after the sizes have passed.
static inline IpagPlan ipa_group_plan(const BpmiOptions &opt, uint64_t n, int protocol, uint64_t n_proofs, const IpaPackedIn &in, int has_scale, uint64_t group,
                                      bool have_outputs, uint64_t t_budget) {
  u32 k;
  if (!have_outputs) return ipag_plan_error("null argument (values and status)");
  if (!log2_exact(n, k) || k > IPAB_K_MAX) return ipag_plan_error("n must be 2^k, k <= 22");
  if (group < 1) return ipag_plan_error("group must be at least 1");
  if (n_proofs >= 1 && n_proofs <= IPAB_PROOFS_MAX) {
    const uint64_t g = group < n_proofs ? group : n_proofs;
    if ((n_proofs + g - 1) / g * 2 * n > IPAG_ROWS_MAX) return ipag_plan_error("too many groups: n_groups x 2 n must not exceed 2^26");
  }
  IpagPlan p;
  p.packed = ipa_packed_plan(opt, k, protocol, n_proofs, in, has_scale);
  if (p.packed.err) return ipag_plan_error(p.packed.msg);
  if (t_budget && t_budget < IPAP_T_BYTES_MAX) {
    uint64_t rows = t_budget / (8ull * p.packed.W) / 64 * 64;
    if (rows < 64) rows = 64;
    if (rows < p.packed.rows) p.packed.rows = (u32)rows;
  }
  p.group = (u32)(group < n_proofs ? group : n_proofs);
  p.ngroups = (u32)((n_proofs + p.group - 1) / p.group);
  p.per = p.packed.pairs;
  p.W = 255u / MID_C + 1u;
  p.pairs = 2 * n + (uint64_t)p.group * p.per;
  p.route = p.pairs <= GROUP_LIGHT_NMAX ? IPAG_ROUTE_LIGHT : (p.pairs <= MID_NMAX ? IPAG_ROUTE_MID : IPAG_ROUTE_MSM_RUN);
  p.b_gsa = p.b_gsb = 32 * n * p.ngroups;
  p.b_E = 4ull * XYZZ_WORDS * p.W * p.ngroups;                  // (laid out on every route; msm_run writes the caller's values itself)
  p.b_vals = 64ull * p.ngroups;
  uint64_t at = p.packed.total_bytes;
  auto take = [&at](uint64_t bytes) { const uint64_t o = at; at += align_up(bytes, 256); return o; };
  p.o_gsa = take(p.b_gsa); p.o_gsb = take(p.b_gsb); p.o_E = take(p.b_E); p.o_vals = take(p.b_vals);
  p.total_bytes = at;
  return p;
}
