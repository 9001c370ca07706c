// ipa_group_mixed_plan_host.hpp -- part of libbpmi; plain C++17 (no HIP, no bpmi_ctx), also compiled for the host by tests/csrc_host.
// The plan of bpmi_ipa_group_values_packed_mixed_dev: a list of classes of PACKED inner-product proofs of DIFFERENT lengths whose
// weighted combination is taken per GROUP of consecutive proofs of ONE class, so that one call says which groups hold an invalid
// proof.  It is the unchanged ipa_packed_mixed_plan (the uploads, the preparation's rounds, the mixed half tables; its plain SA / SB,
// units and partial sums are laid out and not used) followed by the groups' regions, and per class what ipa_group_plan decides for a
// batch of one length: both plans call ipag_shape, ipag_rows_fit and ipag_place of ipa_group_plan_host.hpp, which hold those rules
// once.  tests/test_ipa_group_mixed_plan_cpu.py checks it without a GPU; ipa_group_mixed_dev_host.hpp consumes it.
// Kernels: k_sc_svector_sum_groups_mixed (ipa_mixed_kernels.hpp), k_msm_ipa_group_mixed (msm_kernels.hpp).
//
// Groups.  Class c (n_c = 2^k_c elements, P_c proofs) is cut into groups of group_c = min(group[c], P_c) consecutive proofs, the last
// one possibly short; a group never straddles a class and an empty class has none.  Groups are numbered class-major, in the caller's
// order: class c owns the groups [first_group, first_group + ngroups).  Clamp, group count, pairs of a full group's MSM and its
// route are ipag_shape's, class by class.
//
// Proofs and tables.  ipa_mixed_plan sorts the class-major list of proofs by descending k, STABLE: a class's proofs have one k, so
// they stay contiguous and in their own order (two classes of one k follow each other in the caller's order).  Its descriptors give
// consecutive proofs of one (k, kl) consecutive tables of 2^kl + 2^(k - kl) records (ipa_mixed_plan_host.hpp: `off` advances by exactly
// that per sorted proof), so the block of the packed half-table array that starts at desc[first_sorted].tab_off has the layout
// svb_sum_element reads for a batch of one length: proof j of the class at tab_base + j tab_stride.  The extra pairs stay in the
// caller's class order: proof j of class c owns the pairs [extra_off + j per_c, extra_off + (j + 1) per_c).
//
// Rows.  Group t of class c has a row of n_c scalars of SA and one of SB.  A class's rows are contiguous from its row offset, and the
// row offset (in scalars) is rounded up to a multiple of 256, so that one 256-lane block of the sum kernel belongs to ONE class: block
// b of the launch belongs to the last class whose block start (row offset / 256) is <= b, and its lanes beyond the class's
// ngroups n_c scalars are pad lanes.
// Indexing: sum_c ngroups_c 2 n_c <= 2^26 (IPAG_ROWS_MAX, the cap of the single-class call) gives sum_c ngroups_c n_c <= 2^25; each of the
// at most 64 classes adds fewer than 256 pad scalars, so the padded rows stay below 2^25 + 2^14 < 2^32 and every scalar index fits 32
// bits (the word index 8 x scalar is formed in 64 bits).
//
// Regions behind packed.total_bytes, every one on a 256-byte line:
//   rows SA 32 rows_total | rows SB 32 rows_total      (rows_total: the last class's row offset + its ngroups n scalars)
//   E 144 W per group (window sums, W = 255 / MID_C + 1 windows) | values 64 per group
//   class table, IPAGM_CLASS_WORDS words per non-empty class, caller's order:
//       block start, row offset, k, kl, table base, table stride, proofs, group
//   group table, IPAGM_GROUP_WORDS words per group:  n_c, row offset of the group's row, first extra pair, extra pairs
//   the list of the LIGHT groups | the list of the MID groups       (block b of a launch is (list[b / W], window b % W))
// The four tables are uploaded as one piece.  For ONE class rows, E and values have the sizes of ipa_group_plan.
#pragma once
#include <string>
#include <vector>

#include "ipa_group_plan_host.hpp"
#include "ipa_packed_mixed_plan_host.hpp"

#define IPAGM_CLASS_WORDS 8u
#define IPAGM_GROUP_WORDS 4u
#define IPAGM_BLOCK 256u                       // lanes of one block of k_sc_svector_sum_groups_mixed

struct IpagmClass {
  u32 k = 0, kl = 0, per = 0;                  // n = 2^k; extra pairs per proof
  u32 count = 0;                               // proofs; 0: an empty class, nothing else is set
  u32 group = 0, ngroups = 0, first_group = 0;
  uint64_t pairs = 0;                          // 2 n + group per: the pairs of a full group's MSM
  u32 route = 0;                               // IPAG_ROUTE_*
  u32 tab_base = 0, tab_stride = 0;            // in records of the packed half-table array
  u32 row_off = 0, block_start = 0;            // in scalars (a multiple of 256); row_off / 256
  uint64_t rows = 0;                           // ngroups n scalars
  uint64_t extra_off = 0;                      // its first extra pair
};

struct IpagmPlan : IpagRegions {               // (rows SA / rows SB / E / values and W: ipag_place)
  int err = 0; std::string msg;                // an argument error: nothing else is set
  bool empty = false;                          // every class is empty: value_off is all zero, nothing to do
  IpapmPlan packed;                            // the unchanged plan of the mixed packed verifier
  std::vector<IpagmClass> cls;                 // n_classes, caller's order
  std::vector<uint64_t> value_off;             // n_classes + 1: class c owns the values [value_off[c], value_off[c + 1])
  u32 ngroups = 0;
  u32 n_blocks = 0;                            // of the sum kernel
  uint64_t rows_total = 0;
  std::vector<u32> class_tab, group_tab, light, mid;
  std::vector<u32> run;                        // the groups on the msm_run route
  uint64_t o_ctab = 0, o_gtab = 0, o_light = 0, o_mid = 0;
  uint64_t b_ctab = 0, b_gtab = 0, b_light = 0, b_mid = 0;
  uint64_t total_bytes = 0;
};

static inline IpagmPlan ipagm_plan_error(const std::string &msg) { IpagmPlan p; p.err = BPMI_E_ARG; p.msg = msg; return p; }

// K, protocol, classes, weights, seed, has_scale: as ipa_packed_mixed_plan.  group: one size per class (read for the non-empty ones).
// have_outputs: `values`, `value_off` and `status` are all there.  t_budget: bytes of the T regions of one round (0: IPAP_T_BYTES_MAX).
// Reads classes[c].tr_off[0 .. n_proofs] of the non-empty classes and nothing else of the arrays.
static inline IpagmPlan ipa_group_mixed_plan(const BpmiOptions &opt, u32 K, int protocol, u32 n_classes, const bpmi_ipa_packed_class *classes, const uint64_t *group,
                                             const uint8_t *weights, const uint8_t *seed, int has_scale, bool have_outputs, uint64_t t_budget) {
  if (!have_outputs) return ipagm_plan_error("null argument (values, value_off and status)");
  if (!group) return ipagm_plan_error("null argument (group)");
  IpagmPlan p;
  p.packed = ipa_packed_mixed_plan(opt, K, protocol, n_classes, classes, weights, seed, has_scale, t_budget ? t_budget : IPAP_T_BYTES_MAX);
  if (p.packed.err) return ipagm_plan_error(p.packed.msg);
  const IpapmPlan &mp = p.packed;
  p.cls.resize(n_classes);
  p.value_off.assign(n_classes + 1, 0);
  if (mp.empty) { p.empty = true; return p; }
  uint64_t row_scalars = 0;                                  // sum ngroups n, unpadded: the cap
  for (u32 c : mp.fin_cls) {
    if (group[c] < 1) return ipagm_plan_error("class " + std::to_string(c) + ": group must be at least 1");
    const IpapmClass &m = mp.cls[c];
    row_scalars += (uint64_t)ipag_shape(m.n_proofs, group[c], m.k, m.pairs).ngroups << m.k;
  }
  if (!ipag_rows_fit(row_scalars)) return ipagm_plan_error("too many groups: the sum over the classes of n_groups x 2 n must not exceed 2^26");
  u32 first_group = 0, block = 0;
  for (u32 c = 0; c < n_classes; c++) {
    p.value_off[c] = first_group;
    const IpapmClass &m = mp.cls[c];
    if (!m.n_proofs) continue;
    IpagmClass &q = p.cls[c];
    const u32 n = 1u << m.k;
    const IpagShape s = ipag_shape(m.n_proofs, group[c], m.k, m.pairs);
    q.k = m.k; q.kl = m.k / 2; q.per = m.pairs; q.count = (u32)m.n_proofs;
    q.group = s.group; q.ngroups = s.ngroups; q.pairs = s.pairs; q.route = s.route;
    q.first_group = first_group;
    q.tab_base = mp.base.desc[m.first_sorted].tab_off;
    q.tab_stride = (1u << q.kl) + (1u << (q.k - q.kl));
    q.block_start = block; q.row_off = block * IPAGM_BLOCK;
    q.rows = (uint64_t)q.ngroups * n;
    q.extra_off = m.extra_off;
    block += (u32)((q.rows + IPAGM_BLOCK - 1) / IPAGM_BLOCK);
    p.rows_total = q.row_off + q.rows;
    const u32 row[IPAGM_CLASS_WORDS] = {q.block_start, q.row_off, q.k, q.kl, q.tab_base, q.tab_stride, q.count, q.group};
    p.class_tab.insert(p.class_tab.end(), row, row + IPAGM_CLASS_WORDS);
    std::vector<u32> &list = q.route == IPAG_ROUTE_LIGHT ? p.light : (q.route == IPAG_ROUTE_MID ? p.mid : p.run);
    for (u32 t = 0; t < q.ngroups; t++) {
      const u32 g0 = t * q.group, cnt = q.count - g0 < q.group ? q.count - g0 : q.group;
      const u32 grow[IPAGM_GROUP_WORDS] = {n, q.row_off + t * n, (u32)(q.extra_off + (uint64_t)g0 * q.per), cnt * q.per};
      p.group_tab.insert(p.group_tab.end(), grow, grow + IPAGM_GROUP_WORDS);
      list.push_back(first_group + t);
    }
    first_group += q.ngroups;
  }
  p.value_off[n_classes] = first_group;
  p.ngroups = first_group; p.n_blocks = block;
  p.b_ctab = 4ull * p.class_tab.size(); p.b_gtab = 4ull * p.group_tab.size();
  p.b_light = 4ull * p.light.size(); p.b_mid = 4ull * p.mid.size();
  uint64_t at = mp.total_bytes;
  ipag_place(p, at, p.rows_total, p.ngroups);
  p.o_ctab = ipag_take(at, p.b_ctab); p.o_gtab = ipag_take(at, p.b_gtab); p.o_light = ipag_take(at, p.b_light); p.o_mid = ipag_take(at, p.b_mid);
  p.total_bytes = at;
  return p;
}
