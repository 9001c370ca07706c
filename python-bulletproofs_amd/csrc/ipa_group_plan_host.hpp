// ipa_group_plan_host.hpp -- part of libbpmi; plain C++17 (no HIP, no bpmi_ctx), also compiled for the host by tests/csrc_host.
// The plan of bpmi_ipa_group_values_packed_dev: a batch of PACKED inner-product proofs whose weighted combination is taken per GROUP
// of `group` consecutive proofs, so that one call says which groups hold an invalid proof.  It is the unchanged ipa_packed_plan (the
// uploads, the preparation's regions, the half tables; its plain SA / SB and partial sums are laid out and not used) followed by the
// groups' regions (ipag_place), with the groups' shape and the route of their MSMs (ipag_shape) under the rows cap (ipag_rows_fit).
// ipa_group_mixed_plan (ipa_group_mixed_plan_host.hpp) calls the same three per class: they hold those rules once.
// tests/test_ipa_group_plan_cpu.py checks the plan without a GPU; ipa_group_dev_host.hpp consumes it.
// Kernels: k_sc_svector_sum_groups (scalar_kernels.hpp), k_msm_ipa_group (msm_kernels.hpp).
#pragma once
#include "ipa_packed_plan_host.hpp"

#define IPAG_ROWS_MAX (1ull << 26)             // group scalars of one array: ngroups x 2 n (the cap of bpmi_rp_batch_group_values_dev's rows)
#define IPAG_ROUTE_LIGHT 1u
#define IPAG_ROUTE_MID 2u
#define IPAG_ROUTE_MSM_RUN 3u

// The groups of P proofs of n = 2^k elements: `group` consecutive proofs each (at most P), the last one possibly short.  The MSM of
// a full group runs over [g | h | the group's extra pairs], pairs = 2 n + group per (per = 2k + 2 under Protocol 2, 2k + 4 under
// Protocol 1: ipap_pairs), and that number names the route: one launch of the group kernel in its light shape (<= GROUP_LIGHT_NMAX)
// or its k_msm_mid shape (<= MID_NMAX), or msm_run group by group.  n_proofs >= 1, group >= 1.
struct IpagShape { u32 group = 0, ngroups = 0; uint64_t pairs = 0; u32 route = 0; };
static inline IpagShape ipag_shape(uint64_t n_proofs, uint64_t group, u32 k, u32 per) {
  IpagShape s;
  s.group = (u32)(group < n_proofs ? group : n_proofs);
  s.ngroups = (u32)((n_proofs + s.group - 1) / s.group);
  s.pairs = (2ull << k) + (uint64_t)s.group * per;
  s.route = s.pairs <= GROUP_LIGHT_NMAX ? IPAG_ROUTE_LIGHT : (s.pairs <= MID_NMAX ? IPAG_ROUTE_MID : IPAG_ROUTE_MSM_RUN);
  return s;
}
// the cap of one call's rows: row_scalars = ngroups n, summed over the classes where there are several
static inline bool ipag_rows_fit(uint64_t row_scalars) { return 2 * row_scalars <= IPAG_ROWS_MAX; }

// The groups' regions, every one on a 256-byte line:
//   rows SA[t][i] 32 rows_scalars | rows SB[t][i] 32 rows_scalars | E[t][w] 144 W ngroups (window sums, W windows of MID_C bits) | values 64 ngroups
// (E is laid out on every route; msm_run writes the caller's values itself)
struct IpagRegions {
  u32 W = 0;                                   // windows of MID_C bits
  uint64_t o_gsa = 0, o_gsb = 0, o_E = 0, o_vals = 0;
  uint64_t b_gsa = 0, b_gsb = 0, b_E = 0, b_vals = 0;
};
static inline uint64_t ipag_take(uint64_t &at, uint64_t bytes) { const uint64_t o = at; at += align_up(bytes, 256); return o; }
static inline void ipag_place(IpagRegions &r, uint64_t &at, uint64_t rows_scalars, u32 ngroups) {
  r.W = 255u / MID_C + 1u;
  r.b_gsa = r.b_gsb = 32 * rows_scalars;
  r.b_E = 4ull * XYZZ_WORDS * r.W * ngroups;
  r.b_vals = 64ull * ngroups;
  r.o_gsa = ipag_take(at, r.b_gsa); r.o_gsb = ipag_take(at, r.b_gsb); r.o_E = ipag_take(at, r.b_E); r.o_vals = ipag_take(at, r.b_vals);
}

struct IpagPlan : IpagRegions {
  int err = 0; const char *msg = nullptr;      // an argument error: nothing else is set
  IpapPlan packed;                             // the unchanged plan of the packed verifier (packed.rows: cut to the transposition budget)
  u32 group = 0, ngroups = 0;                  // proofs per group (at most the batch), groups
  u32 per = 0;                                 // extra pairs per proof
  uint64_t pairs = 0;                          // 2 n + group per: the pairs of a full group's MSM
  u32 route = 0;
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
  IpagShape s;
  if (n_proofs >= 1 && n_proofs <= IPAB_PROOFS_MAX) {          // (any other count is the packed plan's to refuse)
    s = ipag_shape(n_proofs, group, k, ipap_pairs(k, protocol));
    if (!ipag_rows_fit(s.ngroups * n)) return ipag_plan_error("too many groups: n_groups x 2 n must not exceed 2^26");
  }
  IpagPlan p;
  p.packed = ipa_packed_plan(opt, k, protocol, n_proofs, in, has_scale);
  if (p.packed.err) return ipag_plan_error(p.packed.msg);
  if (t_budget && t_budget < IPAP_T_BYTES_MAX) {
    uint64_t rows = t_budget / (8ull * p.packed.W) / 64 * 64;
    if (rows < 64) rows = 64;
    if (rows < p.packed.rows) p.packed.rows = (u32)rows;
  }
  p.group = s.group; p.ngroups = s.ngroups; p.per = p.packed.pairs; p.pairs = s.pairs; p.route = s.route;
  uint64_t at = p.packed.total_bytes;
  ipag_place(p, at, n * s.ngroups, s.ngroups);
  p.total_bytes = at;
  return p;
}
