// ipa_packed_mixed_plan_host.hpp -- part of libbpmi; plain C++17 (no HIP, no bpmi_ctx), also compiled for the host by tests/csrc_host.
// The plan of a batch of PACKED inner-product proofs of DIFFERENT lengths -- a list of classes, each what one call of
// bpmi_ipa_verify_batch_packed_dev takes -- on its way through bpmi_ipa_batch_prepare_mixed, bpmi_ipa_batch_prepare_mixed_dev and
// bpmi_ipa_verify_batch_packed_mixed_dev, as a pure function of the sizes over the unchanged ipa_mixed_plan and ipa_packed_plan: the
// argument errors with their messages, the embedded IpamPlan of the class-major list of k's, per class the place of its records,
// extra pairs and uploads, the rounds of the preparation with their role units, and the pair-offset table of the finish.
// tests/test_ipa_packed_mixed_plan_cpu.py checks it without a GPU; ipa_packed_mixed_dev_host.hpp consumes it.
//
// Numbering.  Proofs are numbered class-major (gbase[c] = proofs of the classes before c).  ipa_mixed_plan sorts that list by
// descending k, stable: a class's proofs have one k and follow each other, so they stay contiguous and class c's records are the
// block that starts at desc[first_sorted].rec_off.  The extra pairs stay in the caller's class order.
//
// Workspace behind base.total_bytes, every region on a 256-byte line:
//   per class, caller's order:  ab | xs | LR | transcripts (+ 8) | tr_off | start | u | P | c | head | weights | role verdicts
//   then once:                  status (one byte per proof, global index)
//   then per class:             T, the transposed transcripts of one round of that class (8 W_c rows_c bytes)
//   then once:                  the unit table (IPAPM_UNIT_STRIDE bytes per unit, round-major) | the class table of the finish
//                               (IPAPM_UNIT_STRIDE bytes per non-empty class) | the pair-offset table (non-empty classes + 1 words)
// For ONE class this is the layout of ipa_packed_plan followed by the three tables.
//
// Rounds.  The T regions of one round together take about `t_budget` bytes: the budget is split evenly over the non-empty classes,
// rows_c = as many multiples of 64 as fit the class's share, at least 64 (a share below 64 rows is exceeded: whole waves), at most
// P_c.  Rounds = max_c ceil(P_c / rows_c); a class that is exhausted takes no part in later rounds.  Round r runs ONE launch of
// k_ipap_roles_mixed over the units {class, rows [r rows_c, ..)} of the classes still running, in the caller's order; a unit owns
// IPAP_ROLES blocks per 64 rows, and the launch's dynamic LDS is that of the round's largest k.
#pragma once
#include <string>
#include <vector>

#include "ipa_mixed_plan_host.hpp"
#include "ipa_packed_plan_host.hpp"

#define IPAPM_CLASSES_MAX 64u
#define IPAPM_UNIT_STRIDE 256u                 // bytes of one slot of the unit table and of the class table (ipad::MixedUnit, ipa_packed_kernels.hpp)

struct IpapmClass : IpapRegions {              // its regions (the status is the call's, the T region follows the status)
  u32 k = 0, pairs = 0;
  uint64_t n_proofs = 0;                       // 0: skipped, nothing else is set
  uint64_t gbase = 0;                          // global index of its proof 0
  u32 first_sorted = 0, rec_off = 0;           // its first position in base.perm's order; the word offset of its records
  uint64_t extra_off = 0;                      // its first extra pair
  u32 W = 0, rows = 0, chunks = 0;             // 8-byte rows of T; proofs per round; rounds it takes part in
  uint64_t tr_bytes = 0;
};
struct IpapmUnit { u32 cls, chunk, first_block; };      // rows [chunk rows, min(P, (chunk + 1) rows)) of class cls
struct IpapmRound { u32 first_unit = 0, n_units = 0, blocks = 0, lds_bytes = 0, k_max = 0; };

struct IpapmPlan {
  int err = 0; std::string msg;                // an argument error: nothing else is set
  bool empty = false;                          // every class is empty: nothing to do
  int protocol = 0;
  u32 n_classes = 0;
  IpamPlan base;                               // over the class-major list of k's, n_extra = the extra pairs of all classes
  std::vector<IpapmClass> cls;
  std::vector<IpapmUnit> unit;                 // round-major: slot i of the unit table
  std::vector<IpapmRound> round;
  std::vector<u32> fin_cls;                    // the non-empty classes, caller's order: slot j of the finish's class table
  std::vector<u32> pair_off;                   // fin_cls.size() + 1: the extra pairs of fin_cls[j] are [pair_off[j], pair_off[j + 1])
  uint64_t tr_bytes = 0;
  uint64_t o_status = 0, b_status = 0, o_units = 0, b_units = 0, o_fin = 0, b_fin = 0, o_pairoff = 0, b_pairoff = 0;
  uint64_t total_bytes = 0;
};

static inline IpapmPlan ipapm_plan_error(const std::string &msg) { IpapmPlan p; p.err = BPMI_E_ARG; p.msg = msg; return p; }
// a class's arrays with the call's weights (the class's slice, or NULL) and seed
static inline IpaPackedIn ipapm_class_in(const bpmi_ipa_packed_class &c, const uint8_t *weights, const uint8_t *seed) {
  return ipap_in(c.ab, c.xs, c.LR, c.transcripts, c.tr_off, c.start, c.u, c.P, c.c, c.head, weights, seed);
}

// K: the capacity, n_gens = 2^K.  weights / seed: the call's (their addresses are never followed).  has_scale: as ipa_mixed_plan (0 for
// the preparation alone).  t_budget: bytes of the T regions of one round (the library: IPAP_T_BYTES_MAX, or the test hook's value).
// Reads classes[c].tr_off[0 .. n_proofs] of the non-empty classes and nothing else of the arrays.
static inline IpapmPlan ipa_packed_mixed_plan(const BpmiOptions &opt, u32 K, int protocol, u32 n_classes, const bpmi_ipa_packed_class *classes,
                                              const uint8_t *weights, const uint8_t *seed, int has_scale, uint64_t t_budget) {
  if (n_classes < 1 || n_classes > IPAPM_CLASSES_MAX || !classes) return ipapm_plan_error("between 1 and 64 classes, classes not NULL");
  if (protocol != 1 && protocol != 2) return ipapm_plan_error("protocol must be 1 or 2");
  if (K > IPAB_K_MAX) return ipapm_plan_error("n_gens must be 2^K, K <= 22");
  IpapmPlan p;
  p.protocol = protocol; p.n_classes = n_classes;
  p.cls.resize(n_classes);
  uint64_t total = 0, n_extra = 0, tr_bytes = 0;
  for (u32 c = 0; c < n_classes; c++) {
    const bpmi_ipa_packed_class &in = classes[c];
    if (!in.n_proofs) continue;
    const std::string who = "class " + std::to_string(c) + ": ";
    if (in.k > K) return ipapm_plan_error(who + "k must be at most K (proofs of 2^k elements over n_gens = 2^K generators)");
    const IpapPlan single = ipa_packed_plan(opt, in.k, protocol, in.n_proofs, ipapm_class_in(in, weights, seed), 0);      // the class's errors, W
    if (single.err) return ipapm_plan_error(who + single.msg);
    IpapmClass &m = p.cls[c];
    m.k = in.k; m.pairs = single.pairs; m.n_proofs = in.n_proofs; m.gbase = total; m.extra_off = n_extra; m.tr_bytes = single.tr_bytes; m.W = single.W;
    total += in.n_proofs; n_extra += in.n_proofs * m.pairs; tr_bytes += m.tr_bytes;
    p.fin_cls.push_back(c);
  }
  if (!total) { p.empty = true; return p; }
  if (total > IPAB_PROOFS_MAX) return ipapm_plan_error("between 1 and 2^16 proofs per call");
  if (n_extra > IPAB_EXTRA_MAX) return ipapm_plan_error("at most 2^22 extra points per call");
  if (tr_bytes > IPAP_TRANSCRIPTS_MAX) return ipapm_plan_error("at most 4 GiB of transcripts per call");
  std::vector<u32> ks;
  ks.reserve((size_t)total);
  for (u32 c = 0; c < n_classes; c++) ks.insert(ks.end(), (size_t)p.cls[c].n_proofs, p.cls[c].k);
  p.base = ipa_mixed_plan(opt, 1ull << K, total, ks.data(), n_extra, has_scale);
  if (p.base.err) return ipapm_plan_error(p.base.msg);
  p.tr_bytes = tr_bytes;
  std::vector<u32> where((size_t)total);                     // the caller's index -> sorted position
  for (u32 s = 0; s < (u32)total; s++) where[p.base.perm[s]] = s;
  // the uploads of every class, the status, the T regions, the tables
  uint64_t at = p.base.total_bytes;
  auto take = [&at](uint64_t bytes) { const uint64_t o = at; at += align_up(bytes, 256); return o; };
  const uint64_t n_live = p.fin_cls.size(), share = t_budget / n_live;
  u32 n_rounds = 0;
  for (u32 c : p.fin_cls) {
    IpapmClass &m = p.cls[c];
    m.first_sorted = where[(size_t)m.gbase];
    m.rec_off = p.base.desc[m.first_sorted].rec_off;
    uint64_t rows = share / (8ull * m.W) / 64 * 64;
    if (rows < 64) rows = 64;
    m.rows = (u32)(rows < m.n_proofs ? rows : m.n_proofs);
    m.chunks = (u32)((m.n_proofs + m.rows - 1) / m.rows);
    if (m.chunks > n_rounds) n_rounds = m.chunks;
    // (has_start / has_weights as ipapm_class_in gave them to the class's ipa_packed_plan above: for ONE class this is that plan's layout)
    ipap_region_sizes(m, m.k, protocol, m.n_proofs, classes[c].start != nullptr, weights != nullptr, m.tr_bytes);
    m.b_T = 8ull * m.W * m.rows;
    ipap_place_regions(m, take);
  }
  p.b_status = total; p.o_status = take(p.b_status);
  for (u32 c : p.fin_cls) p.cls[c].o_T = take(p.cls[c].b_T);
  for (u32 r = 0; r < n_rounds; r++) {
    IpapmRound rd;
    rd.first_unit = (u32)p.unit.size();
    for (u32 c : p.fin_cls) {
      const IpapmClass &m = p.cls[c];
      if (r >= m.chunks) continue;
      const uint64_t first = (uint64_t)r * m.rows, cnt = m.n_proofs - first < m.rows ? m.n_proofs - first : m.rows;
      p.unit.push_back(IpapmUnit{c, r, rd.blocks});
      rd.n_units++;
      rd.blocks += IPAP_ROLES * (u32)((cnt + 63) / 64);
      if (m.k > rd.k_max) rd.k_max = m.k;
    }
    rd.lds_bytes = rd.k_max * 9u * 64u * 4u;
    p.round.push_back(rd);
  }
  p.pair_off.push_back(0);
  for (u32 c : p.fin_cls) p.pair_off.push_back((u32)(p.cls[c].extra_off + p.cls[c].n_proofs * p.cls[c].pairs));
  p.b_units = (uint64_t)IPAPM_UNIT_STRIDE * p.unit.size(); p.o_units = take(p.b_units);
  p.b_fin = (uint64_t)IPAPM_UNIT_STRIDE * n_live; p.o_fin = take(p.b_fin);
  p.b_pairoff = 4ull * p.pair_off.size(); p.o_pairoff = take(p.b_pairoff);
  p.total_bytes = at;
  return p;
}
