// rp_prove_mixed_plan_host.hpp -- part of libbpmi; plain C++17 (no HIP, no bpmi_ctx), also compiled for the host by tests/csrc_host.
// The plan of ONE call of the batched range-proof prover over CLASSES of different sizes (bpmi_rp_prove_batch_mixed,
// rp_prove_mixed_host.hpp): a prover created for (nbits, M) over N = nbits M generators is a capacity, a class of m_c values per proof
// runs over the first n_c = nbits m_c of gs and of hs.  The tables are indexed by base, so the capacity enters in ONE place: the base
// lists (rpp_class_bases: hs_i at base 3 + N + i).  The plan is a pure function of the shapes: the argument errors and caps, per class
// the geometry of rpp_plan, its regions of every device array, its base lists and its slice of the output, and per step the launches
// with their tables of units {class, first block}: what tests/test_rp_prove_mixed_plan_cpu.py pins without a GPU.
#pragma once
#include <string>
#include <vector>

#include "rp_prove_plan_host.hpp"

#define RPPM_MAX_CLASSES 64u

// The lists of EVERY class of a capacity in one array, cached on the prover: class m = 2^e (nbits m >= 2) at entry
// rpp_capacity_bases_off(nbits, M, m); the whole array has rpp_capacity_bases_off(nbits, M, 2 M) entries (at most 53 000)
static inline size_t rpp_capacity_bases_off(u32 nbits, u32 M, u32 m) {
  size_t off = 0;
  for (u32 mm = 1; mm < m && mm <= M; mm <<= 1) if (nbits * mm >= 2) off += rpp_class_bases_len(nbits * mm);
  return off;
}

// one class of a call, as the caller states it
struct RppmClassIn { u32 m = 0; uint64_t count = 0, seed_total = 0, seed_max = 0; };      // values per proof, proofs, total and longest seed bytes

// what a launch runs; a launch's blocks are the concatenated blocks of its units
enum RppmKind : u32 { RPPM_BLIND, RPPM_COMMIT_A, RPPM_AFFINE, RPPM_MSM, RPPM_CHAL_YZ, RPPM_POLY, RPPM_FINAL_CHAL, RPPM_FINAL_WIDE, RPPM_ROUND_WIDE, RPPM_ROUND_CHAL, RPPM_EMIT };
static inline const char *rppm_kind_name(u32 kind) {
  static const char *const names[] = {"k_pv_blind_mixed", "k_pv_commit_A_mixed", "k_pv_affine_mixed", "k_pv_msm_mixed", "k_pv_chal_yz_mixed", "k_pv_poly_mixed",
                                      "k_pv_final_chal_mixed", "k_pv_final_wide_mixed", "k_pv_round_wide_mixed", "k_pv_round_chal_mixed", "k_pv_emit_mixed"};
  return names[kind];
}
struct RppmUnit { u32 cls, first; };             // blocks [first, the next unit's first) of the launch are class cls's blocks 0 ..
struct RppmLaunch {
  u32 kind = 0, step = 0;
  u32 threads = 0;                               // per block: 256, 64, or the NT of a wide kernel
  u32 gl = 0;                                    // RPPM_MSM: log2 of the lanes per job (1, 4 or 6)
  u32 per = 0, slot0 = 0, slot_step = 0, step_k = 0;   // RPPM_AFFINE: results per proof, first slot, slot step (step_k: the class's k_c)
  u32 round = 0, first = 0;                      // RPPM_ROUND_*: the round; RPPM_ROUND_WIDE first = 1: no fold
  u32 blocks = 0, first_unit = 0, n_units = 0;   // units[first_unit, first_unit + n_units)
};
// a class's jobs of a step's multi-scalar multiplication (rpp::MsmJobs without the pointers)
struct RppmJobs { u32 njobs = 0, ntypes = 0, T = 0, stride = 0, base_off = 0, from_slr = 0, from_tsc = 0; };

struct RppmClass : RppGeom, RppStrides, RppRegions {   // RppRegions: its arrays in the prover's device buffer
  uint64_t count = 0, first = 0;                 // proofs; the call-wide index of proof 0 (class-major in the caller's order)
  size_t bases_off = 0;                          // its lists in the capacity's array (entries)
  size_t seed_at = 0;                            // its seeds inside the call's seed bytes
  uint64_t out_at = 0, out_bytes = 0;            // its slice of the output
  uint64_t fixed_bytes = 0;                      // a proof without its seed
};

struct RppmPlan {
  int err = 0; std::string msg;                  // an argument error: nothing else is set
  u32 nb = 0, M = 0, N = 0, tw = 0, k_max = 0, nsteps = 0;
  std::vector<RppmClass> cls;
  uint64_t n_proofs = 0, total_out = 0, seed_bytes = 0;
  // device buffer: [the classes' inputs | seeds | seed offsets | output offsets | Batch array | MsmJobs array | unit table] uploaded in one copy,
  // then the classes' scratch, then the output bytes
  size_t o_seeds = 0, o_soff = 0, o_ooff = 0, o_batch = 0, o_jobs = 0, o_units = 0, in_bytes = 0, o_out = 0, need = 0;
  std::vector<RppmUnit> units;
  std::vector<RppmLaunch> launches;              // in launch order; launches of step s are contiguous
  std::vector<RppmJobs> jobs;                    // [step][class], steps 0 .. 2 + k_max (njobs = 0: the class has no multiplication in the step)
};
#define RPPM_BATCH_SLOT 512u                     // bytes of a class's rpp::Batch in the device array (static_assert in rp_prove_mixed_kernels.hpp)
#define RPPM_JOBS_SLOT 48u                       // bytes of an rpp::MsmJobs

static inline RppmPlan rppm_error(const std::string &msg) { RppmPlan p; p.err = BPMI_E_ARG; p.msg = msg; return p; }

// tw: the window bits of the prover's tables (recorded: one width for every class); wire_fmt: option "prover_wire_format"; job_lanes:
// option "prover_job_lanes"; ip_prefix_len: bytes of "&&" str(x_ip) "&", which start every Protocol-2 transcript (the prover's own; 81: the
// longest there is, x_ip of 78 digits)
// the argument errors and caps, from the shapes alone (nothing of a call beyond them is read or allocated): empty, or the text of the BPMI_E_ARG
static inline std::string rppm_args_error(uint32_t nbits, uint32_t M, uint32_t n_classes, const RppmClassIn *classes) {
  if (nbits < 1 || nbits > 128 || (nbits & (nbits - 1)) || M < 1 || (M & (M - 1)) || (uint64_t)nbits * M < 2 || (uint64_t)nbits * M > PROVER_ELEMS_MAX)
    return "the bit width (at most 128) and the number of values must be powers of two with 2 <= bits x values <= 1024";
  if (n_classes > RPPM_MAX_CLASSES) return "n_classes must be at most 64";
  if (n_classes && !classes) return "null argument";
  uint64_t proofs = 0, elems = 0;
  for (u32 c = 0; c < n_classes; c++) {
    const RppmClassIn &k = classes[c];
    const std::string who = "class " + std::to_string(c) + ": ";
    if (k.m < 1 || (k.m & (k.m - 1)) || k.m > M || (uint64_t)nbits * k.m < 2)
      return who + "the number of values must be a power of two, at most the prover's, with bits x values >= 2";
    if (k.count == 0) return who + "n_proofs must be at least 1";
    if (k.count > PROVER_PROOFS_MAX) return "at most 2^20 proofs per call";
    proofs += k.count;
    elems += k.count * nbits * k.m;
    if (proofs > PROVER_PROOFS_MAX) return "at most 2^20 proofs per call";
    if (elems > PROVER_BATCH_ELEMS_MAX) return "at most 2^27 elements (proofs x bits x values) per call";
  }
  return std::string();
}

static inline RppmPlan rpp_mixed_plan(uint32_t nbits, uint32_t M, u32 tw, uint32_t n_classes, const RppmClassIn *classes, int wire_fmt, int job_lanes, size_t ip_prefix_len = 81) {
  {
    const std::string bad = rppm_args_error(nbits, M, n_classes, classes);
    if (!bad.empty()) return rppm_error(bad);
  }
  uint64_t proofs = 0;
  for (u32 c = 0; c < n_classes; c++) {
    if (classes[c].seed_max > 0xFFFF) return rppm_error("class " + std::to_string(c) + ": a seed is longer than 65535 bytes");
    proofs += classes[c].count;
  }
  RppmPlan p;
  p.nb = nbits; p.M = M; p.N = nbits * M; p.tw = tw;
  p.cls.resize(n_classes);
  p.n_proofs = proofs;
  RppTake take;
  // ---- classes: geometry, inputs
  for (u32 c = 0; c < n_classes; c++) {
    const RppmClassIn &k = classes[c];
    RppmClass &q = p.cls[c];
    static_cast<RppGeom &>(q) = rpp_geom(nbits, k.m);
    q.count = k.count;
    q.first = c ? p.cls[c - 1].first + p.cls[c - 1].count : 0;
    static_cast<RppStrides &>(q) = rpp_strides(k.seed_max, q.k, ip_prefix_len);
    q.bases_off = rpp_capacity_bases_off(nbits, M, k.m);
    q.seed_at = p.seed_bytes;
    p.seed_bytes += k.seed_total;
    q.fixed_bytes = rpp_fixed_bytes(q.k, wire_fmt);
    q.out_at = p.total_out;
    q.out_bytes = q.count * q.fixed_bytes + k.seed_total;
    p.total_out += q.out_bytes;
    if (q.k > p.k_max) p.k_max = q.k;
    rpp_take_inputs(q, take, q, (size_t)q.count, q);
  }
  p.nsteps = n_classes ? 4 + p.k_max : 0;
  // ---- steps: the launches and their units
  auto add_launch = [&](RppmLaunch L, auto &&blocks_of) {      // blocks_of(class) = 0: the class is not in the launch
    L.first_unit = (u32)p.units.size();
    u32 at = 0;
    for (u32 c = 0; c < n_classes; c++) {
      const u32 b = blocks_of(c);
      if (!b) continue;
      p.units.push_back(RppmUnit{c, at});
      at += b;
    }
    L.blocks = at; L.n_units = (u32)p.units.size() - L.first_unit;
    if (L.n_units) p.launches.push_back(L);
  };
  auto ceil_div = [](uint64_t a, uint64_t b) { return (u32)((a + b - 1) / b); };
  auto simple = [&](u32 kind, u32 step, u32 threads, auto &&blocks_of, u32 round = 0, u32 first = 0) {
    RppmLaunch L; L.kind = kind; L.step = step; L.threads = threads; L.round = round; L.first = first;
    add_launch(L, blocks_of);
  };
  auto affine = [&](u32 step, u32 per, u32 slot0, u32 slot_step, u32 step_k, auto &&in_step) {
    RppmLaunch L; L.kind = RPPM_AFFINE; L.step = step; L.threads = 256; L.per = per; L.slot0 = slot0; L.slot_step = slot_step; L.step_k = step_k;
    add_launch(L, [&](u32 c) { return in_step(c) ? ceil_div(per * p.cls[c].count, 256) : 0u; });
  };
  auto wide = [&](u32 kind, u32 step, auto &&in_step, u32 round = 0, u32 first = 0) {
    for (u32 NT = 256; NT <= 1024; NT <<= 1)
      simple(kind, step, NT, [&](u32 c) { return in_step(c) && p.cls[c].NT == NT ? ceil_div(p.cls[c].count, p.cls[c].per_block) : 0u; }, round, first);
  };
  p.jobs.assign((size_t)(p.nsteps ? p.nsteps - 1 : 0) * n_classes, RppmJobs());
  // the multiplication of a step: J(c) fills the class's jobs (njobs = 0: none); one launch per lane width, a class's width by the jobs of
  // the whole step (rpp_job_lanes_log2); forced_gl: the two-term jobs of T1 / T2 run two lanes per job
  auto msm = [&](u32 step, auto &&J, int forced_gl) {
    uint64_t total = 0;
    for (u32 c = 0; c < n_classes; c++) { RppmJobs &j = p.jobs[(size_t)step * n_classes + c]; J(c, j); total += j.njobs; }
    const int widths[3] = {1, 4, 6};
    for (int gl : widths) {
      RppmLaunch L; L.kind = RPPM_MSM; L.step = step; L.threads = 256; L.gl = (u32)gl;
      add_launch(L, [&](u32 c) {
        const RppmJobs &j = p.jobs[(size_t)step * n_classes + c];
        if (!j.njobs) return 0u;
        const int mine = forced_gl ? forced_gl : rpp_job_lanes_log2(p.cls[c].n, total, job_lanes);
        return mine == gl ? ceil_div((uint64_t)j.njobs << gl, 256) : 0u;
      });
    }
  };
  auto all = [](u32) { return true; };
  auto chain = [&](u32 c) { return ceil_div(p.cls[c].count, 64); };
  if (n_classes) {
    // step 0: A, S
    simple(RPPM_BLIND, 0, 256, [&](u32 c) { return ceil_div(p.cls[c].count * (2 * p.cls[c].n + 2), 256); });
    simple(RPPM_COMMIT_A, 0, 256, [&](u32 c) { return ceil_div(p.cls[c].count * 16, 256); });
    affine(0, 1, 2 /* PV_PT_A */, 0, 0, all);
    msm(0, [&](u32 c, RppmJobs &j) { const RppmClass &q = p.cls[c]; j.njobs = (u32)q.count; j.ntypes = 1; j.T = 2 * q.n + 1; j.stride = 2 * q.n + 1; j.base_off = rpp_off_S(q.n); j.from_slr = 1; }, 0);
    affine(0, 1, 3 /* PV_PT_S */, 0, 0, all);
    // step 1: y, z, T1, T2
    simple(RPPM_CHAL_YZ, 1, 64, chain);
    wide(RPPM_POLY, 1, all);
    msm(1, [&](u32 c, RppmJobs &j) { const RppmClass &q = p.cls[c]; j.njobs = 2 * (u32)q.count; j.ntypes = 1; j.T = 2; j.stride = 2; j.base_off = rpp_off_T(q.n); j.from_tsc = 1; }, 1);
    affine(1, 2, 0 /* PV_PT_T1 */, 1, 0, all);
    // step 2: x, the vectors, P_new, the scalars of round 0
    simple(RPPM_FINAL_CHAL, 2, 64, chain);
    wide(RPPM_FINAL_WIDE, 2, all);
    msm(2, [&](u32 c, RppmJobs &j) { const RppmClass &q = p.cls[c]; j.njobs = (u32)q.count; j.ntypes = 1; j.T = 2 * q.n + 1; j.stride = 2 * q.n + 1; j.base_off = rpp_off_P(q.n); }, 0);
    affine(2, 1, 5 /* PV_PT_PNEW */, 0, 0, all);
    wide(RPPM_ROUND_WIDE, 2, all, 0, 1);
    // steps 3 .. 2 + k_max: round r for the classes with k_c > r
    for (u32 r = 0; r < p.k_max; r++) {
      auto in_round = [&](u32 c) { return p.cls[c].k > r; };
      msm(3 + r, [&](u32 c, RppmJobs &j) {
        const RppmClass &q = p.cls[c];
        if (q.k <= r) return;
        j.njobs = 2 * (u32)q.count; j.ntypes = 2; j.T = q.n + 1; j.stride = q.n + 1; j.base_off = rpp_off_round(q.n, r);
      }, 0);
      affine(3 + r, 2, 6 + r, 0, 1, in_round);
      simple(RPPM_ROUND_CHAL, 3 + r, 64, [&](u32 c) { return in_round(c) ? chain(c) : 0u; }, r, 0);
      wide(RPPM_ROUND_WIDE, 3 + r, in_round, r, 0);
    }
    // the last step: the wire bytes of every class
    simple(RPPM_EMIT, 3 + p.k_max, 64, chain);
  }
  // ---- the rest of the upload, the scratch, the output
  p.o_seeds = take(p.seed_bytes + 16);
  p.o_soff = take(8 * (size_t)(proofs + 1));
  p.o_ooff = take(8 * (size_t)(proofs + 1));
  p.o_batch = take((size_t)RPPM_BATCH_SLOT * n_classes);
  p.o_jobs = take((size_t)RPPM_JOBS_SLOT * p.jobs.size());
  p.o_units = take(sizeof(RppmUnit) * p.units.size());
  p.in_bytes = take.o;
  for (RppmClass &q : p.cls) rpp_take_scratch(q, take, q, (size_t)q.count, q);
  p.o_out = take((size_t)p.total_out + 16);
  p.need = take.o;
  return p;
}
