// rp_group_mixed_plan_host.hpp -- part of libbpmi; plain C++17 (no HIP, no bpmi_ctx), also compiled for the host by tests/csrc_host.
// The plan of bpmi_rp_batch_group_values_mixed_dev: a MIXED batch of range proofs (classes of one (n_gens, values_per_proof) each over the
// prefixes of one generator list) whose weighted combination is taken per GROUP of consecutive proofs of ONE class, so that one call
// says which groups hold an invalid proof.  It is the unchanged rp_mixed_plan (the uploads, every class's preparation regions, the
// rounds; its merged scalars are laid out and not used, its one bad word is written and not read) followed by the groups' regions, and
// per class what rp_prepare_plan decides for a batch of one size in group mode: rp_group_shape and rp_group_route of
// rp_batch_plan_host.hpp hold those rules once.  One thing of the mixed plan is changed: under option rp_overlap = 0 the point decoding
// runs in FRONT of the rounds (RP_DECODE_FIRST in place of RP_DECODE_LAST), because the per-proof verdicts read the point flags.
// tests/test_rp_group_mixed_plan_cpu.py checks it without a GPU; rp_group_mixed_dev_host.hpp consumes it.
// Kernel: k_msm_group_mixed (msm_kernels.hpp).
//
// Groups.  Class c (n_c generators, m_c values and per_c = 6 + 2 k_c points per proof, P_c proofs) is cut into groups of
// group_c = min(group[c], P_c) consecutive proofs, the last one possibly short; a group never straddles a class.  Groups are numbered
// class-major: class c owns the groups [value_off[c], value_off[c + 1]).  A group's MSM runs over
// [g h u gs[:n_c] hs[:n_c] | its commitments | its proof points]; the pairs of a FULL group, 3 + 2 n_c + group_c (m_c + per_c), name the
// class's route.
//
// Generator copies.  A Segs has three segments, and a group needs shared generators, commitments and proof points; inside
// d_gens = g h u gs[0..N) hs[0..N) the shared part of a class with n_c < N is NOT contiguous (hs starts at 3 + N).  So every distinct
// n_c < N gets a contiguous copy [g h u gs[:n_c] hs[:n_c]] of (3 + 2 n_c) x 64 bytes, made by three device-to-device copies; a class
// with n_c = N reads d_gens itself.
//
// Regions behind mixed.need in ctx->rp_buf, every one on a 256-byte line:
//   per class gfin: ngroups x (3 + 2n) scalars of the groups' MSMs          (all classes' first: word offsets from gfin_base fit 32 bits,
//                                                                            sum ngroups (3 + 2n) <= 2^26 and 64 classes x 64 pad words)
//   per class gsum: ngroups x (5 + 2n) raw column sums | per class ptflag: one byte per proof
//   verdict: one byte per proof of the WHOLE call by global index (class c's slice starts at its first index: one copy serves `status`)
//   the generator copies | E 144 W per group (W = 255 / MID_C + 1 windows) | values 64 per group       (once for all groups: one tail)
//   group table, RPGM_GROUP_WORDS words per group:
//       points offset of its generator copy inside the copies (RPGM_GENS_DIRECT: d_gens), 3 + 2 n_c, word offset of its gfin row from
//       gfin_base, first commitment pair, commitment pairs, first proof-point pair, proof-point pairs, 0     (pairs of d_points / d_scalars)
//   the list of the LIGHT groups | the list of the MID groups        (block b of a launch is (list[b / W], window b % W))
// The table and the two lists are uploaded as one piece; the groups on the msm_run route are a host list (`run`).
#pragma once
#include <string>
#include <vector>

#include "rp_mixed_plan_host.hpp"

#define RPGM_GROUP_WORDS 8u
#define RPGM_GENS_DIRECT 0xFFFFFFFFu
#define RPGM_SCALARS_MAX (1ull << 26)          // sum over the classes of ngroups x (3 + 2 n): the cap of the single-class call

struct RpgmClass {
  u32 n = 0, m = 0, per = 0, count = 0;        // n_gens, values and points per proof, proofs
  u32 group = 0, ngroups = 0, first_group = 0;
  uint64_t pairs = 0;                          // of a full group's MSM
  RpGroupRoute route = RP_GROUPS_NONE;
  RpRegion gsum, gfin, ptflag;                 // in ctx->rp_buf
  size_t o_verdict = 0;                        // its slice of `verdict`
  u32 gens_off = 0;                            // points offset of its generator copy, or RPGM_GENS_DIRECT
  u32 gfin_word = 0;                           // word offset of its gfin region from gfin_base
};
struct RpgmCopy { u32 n = 0, pts_off = 0; RpRegion at; };      // [g h u gs[:n] hs[:n]] at `at`, pts_off points behind copies_base

struct RpgmPlan {
  int err = 0; std::string msg;                // an argument error: nothing else is set
  RpMixedPlan mixed;                           // rp_mixed_plan's, decode first under rp_overlap = 0
  std::vector<RpgmClass> cls;
  std::vector<uint64_t> value_off;             // n_classes + 1
  u32 ngroups = 0, W = 0;
  std::vector<RpgmCopy> copies;                // one per distinct n_c < N, in order of first use
  size_t gfin_base = 0, copies_base = 0;
  RpRegion verdict, E, vals, gtab, light_list, mid_list;
  std::vector<u32> group_tab, light, mid, run;
  size_t need = 0, pin_bytes = 0;
};

static inline RpgmPlan rpgm_plan_error(const std::string &msg) { RpgmPlan p; p.err = BPMI_E_ARG; p.msg = msg; return p; }

// classes .. others_present: as rp_mixed_plan (others_present: d_gens, d_points, d_scalars).  group: one size per class.
// have_outputs: `values`, `value_off` and `status` are all there.  Reads what rp_mixed_plan reads and group[0 .. n_classes).
static inline RpgmPlan rp_group_mixed_plan(const BpmiOptions &o, uint32_t n_classes, const bpmi_rp_class *classes, uint32_t n_gens_max, const uint64_t *group,
                                           bool has_weights, bool has_seed, bool others_present, bool have_outputs) {
  if (!have_outputs) return rpgm_plan_error("null argument (values, value_off and status)");
  if (!group) return rpgm_plan_error("null argument (group)");
  RpgmPlan p;
  p.mixed = rp_mixed_plan(o, n_classes, classes, n_gens_max, has_weights, has_seed, others_present);
  if (p.mixed.err) return rpgm_plan_error(p.mixed.msg);
  RpMixedPlan &mp = p.mixed;
  uint64_t scalars = 0;
  for (u32 c = 0; c < n_classes; c++) {
    if (group[c] < 1) return rpgm_plan_error("class " + std::to_string(c) + ": group must be at least 1");
    scalars += (uint64_t)rp_group_shape(group[c], mp.cls[c].pl.P).ngroups * (3 + 2 * (uint64_t)classes[c].n_gens);
  }
  if (scalars > RPGM_SCALARS_MAX) return rpgm_plan_error("too many groups: the sum over the classes of n_groups x (3 + 2 n_gens) must not exceed 2^26");
  p.W = 255u / MID_C + 1u;
  p.cls.resize(n_classes);
  p.value_off.assign(n_classes + 1, 0);
  u32 first_group = 0;
  for (u32 c = 0; c < n_classes; c++) {
    RpMixedClass &mc = mp.cls[c];
    if (mc.pl.decode == RP_DECODE_LAST) mc.pl.decode = RP_DECODE_FIRST;
    RpgmClass &q = p.cls[c];
    const RpGroupShape s = rp_group_shape(group[c], mc.pl.P);
    q.n = classes[c].n_gens; q.m = mc.pl.m; q.per = mc.pl.per; q.count = mc.pl.P;
    q.group = s.group; q.ngroups = s.ngroups; q.first_group = first_group;
    q.pairs = 3 + 2 * (uint64_t)q.n + (uint64_t)q.group * (q.m + q.per);
    q.route = rp_group_route(q.pairs);
    p.value_off[c] = first_group;
    first_group += q.ngroups;
  }
  p.value_off[n_classes] = first_group;
  p.ngroups = first_group;
  RpLayout buf;
  buf.end = mp.need;
  for (RpgmClass &q : p.cls) q.gfin = buf.add(32 * (3 + 2 * (size_t)q.n) * q.ngroups);
  p.gfin_base = p.cls[0].gfin.off;
  for (RpgmClass &q : p.cls) q.gfin_word = (u32)((q.gfin.off - p.gfin_base) / 4);
  for (RpgmClass &q : p.cls) q.gsum = buf.add(32 * (5 + 2 * (size_t)q.n) * q.ngroups);
  for (RpgmClass &q : p.cls) q.ptflag = buf.add(q.count);
  p.verdict = buf.add((size_t)mp.n_proofs);
  for (u32 c = 0; c < n_classes; c++) p.cls[c].o_verdict = p.verdict.off + (size_t)mp.cls[c].first;
  for (RpgmClass &q : p.cls) {
    q.gens_off = RPGM_GENS_DIRECT;
    if (q.n == n_gens_max) continue;
    for (const RpgmCopy &k : p.copies) if (k.n == q.n) q.gens_off = k.pts_off;
    if (q.gens_off != RPGM_GENS_DIRECT) continue;
    RpgmCopy k;
    k.n = q.n; k.at = buf.add(64 * (3 + 2 * (size_t)q.n));
    if (p.copies.empty()) p.copies_base = k.at.off;
    k.pts_off = (u32)((k.at.off - p.copies_base) / 64);
    q.gens_off = k.pts_off;
    p.copies.push_back(k);
  }
  p.E = buf.add(4ull * XYZZ_WORDS * p.W * p.ngroups);
  p.vals = buf.add(64 * (size_t)p.ngroups + 256);
  for (u32 c = 0; c < n_classes; c++) {
    const RpgmClass &q = p.cls[c];
    const RpMixedClass &mc = mp.cls[c];
    const u32 nshared = 3 + 2 * q.n;
    std::vector<u32> &list = q.route == RP_GROUPS_LIGHT ? p.light : (q.route == RP_GROUPS_MID ? p.mid : p.run);
    for (u32 t = 0; t < q.ngroups; t++) {
      const u32 g0 = t * q.group, cnt = q.count - g0 < q.group ? q.count - g0 : q.group;
      const u32 row[RPGM_GROUP_WORDS] = {q.gens_off, nshared, q.gfin_word + 8u * nshared * t, (u32)(mc.pair_off + (uint64_t)q.m * g0), cnt * q.m,
                                         (u32)(mc.pair_off + mc.nv + (uint64_t)q.per * g0), cnt * q.per, 0u};
      p.group_tab.insert(p.group_tab.end(), row, row + RPGM_GROUP_WORDS);
      list.push_back(q.first_group + t);
    }
  }
  p.gtab = buf.add(4 * p.group_tab.size());
  p.light_list = buf.add(4 * p.light.size());
  p.mid_list = buf.add(4 * p.mid.size());
  p.need = buf.end;
  p.pin_bytes = std::max<size_t>(mp.pin_bytes, 64 * (size_t)p.ngroups + (size_t)mp.n_proofs + 64);
  return p;
}
