// ipa_prove_mixed_plan_host.hpp -- part of libbpmi; plain C++17 (no HIP, no bpmi_ctx), also compiled for the host by tests/csrc_host.
// The plan of ONE call of the batched inner-product prover over CLASSES of different lengths (bpmi_ipa_prove_batch_mixed and
// bpmi_ipa_batch_prover_commit_batch_mixed, ipa_prove_mixed_host.hpp): a prover created over N generators is a capacity, a class of
// n_c = 2^k_c <= N elements runs over g[:n_c], h[:n_c], the one u and h_scale[:n_c].  The tables are indexed by base and the rounds
// never fold a generator, so the capacity enters in ONE place: the base of h_j (ipp_class_bases: 1 + N + j).  The plan is a pure
// function of the shapes: the argument errors and caps, per class the geometry of ipp_plan, its regions of every array of ipp::Batch,
// its strides and its base lists, and per step the launches with their tables of units {class, first block}: what
// tests/test_ipa_prove_mixed_plan_cpu.py pins without a GPU.  The host runs the launches in order and nothing else.
#pragma once
#include <string>
#include <vector>

#include "ipa_prove_plan_host.hpp"
#include "rp_prove_mixed_plan_host.hpp"

#define IPPM_MAX_CLASSES 64u
#define IPPM_BATCH_SLOT 256u                     // bytes of a class's ipp::Batch in the device array (static_assert in ipa_prove_mixed_kernels.hpp)
#define IPPM_COMMIT_SLOT 64u                     // bytes of a class's ipp::Commit
#define IPPM_AFFINE_SLOT 32u                     // bytes of a class's ipp::AffineJob
#define IPPM_JOBS_SLOT RPPM_JOBS_SLOT            // bytes of an rpp::MsmJobs

// The lists of EVERY class of a capacity in one device array, made by a prover's first mixed call and kept: class n = 2^e at entry
// ipp_capacity_bases_off(N, n); the whole array has ipp_capacity_bases_off(N, 2 N) entries -- at most 36 989 (74 KB) at N = 1 024
static inline size_t ipp_capacity_bases_off(u32 N, u32 n) {
  size_t off = 0;
  for (u32 nn = 1; nn < n && nn <= N; nn <<= 1) off += ipp_class_bases_len(nn);
  return off;
}
// the statements' lists likewise: per class the three lists of ipp_commit_bases_all (4 n + 3 entries; ipp_commit_bases_offset inside);
// at most 8 221 entries at N = 1 024
static inline size_t ipp_capacity_commit_bases_off(u32 N, u32 n) {
  size_t off = 0;
  for (u32 nn = 1; nn < n && nn <= N; nn <<= 1) off += 4 * (size_t)nn + 3;
  return off;
}
static inline std::vector<unsigned short> ipp_capacity_bases(u32 N) {
  std::vector<unsigned short> all;
  for (u32 n = 1; n <= N; n <<= 1) { const std::vector<unsigned short> bl = ipp_class_bases(n, N); all.insert(all.end(), bl.begin(), bl.end()); }
  return all;
}
static inline std::vector<unsigned short> ipp_capacity_commit_bases(u32 N) {
  std::vector<unsigned short> all;
  for (u32 n = 1; n <= N; n <<= 1) { const std::vector<unsigned short> bl = ipp_commit_bases_all(n, N); all.insert(all.end(), bl.begin(), bl.end()); }
  return all;
}

// one class of a call, as the caller states it.  Proving: have_c (Protocol 1: c given).  Statements: have_a, have_b, have_t
struct IppmClassIn {
  u32 n = 0; uint64_t count = 0, seed_max = 0;
  bool have_c = false, have_a = true, have_b = true, have_t = false;
};

static inline bool ipp_is_class(u32 N, u32 n) { return n >= 1 && !(n & (n - 1)) && n <= N; }

// the argument errors and caps, from the shapes alone (nothing of a call beyond them is read or allocated): empty, or the text of the BPMI_E_ARG
static inline std::string ippm_args_error(uint32_t N, uint32_t n_classes, const IppmClassIn *classes) {
  if (N < 1 || N > PROVER_ELEMS_MAX || (N & (N - 1))) return "the vector length must be a power of two with 1 <= n <= 1024 (longer vectors: the single-proof prover)";
  if (n_classes > IPPM_MAX_CLASSES) return "n_classes must be at most 64";
  if (n_classes && !classes) return "null argument";
  uint64_t proofs = 0, elems = 0;
  for (u32 c = 0; c < n_classes; c++) {
    const IppmClassIn &k = classes[c];
    const std::string who = "class " + std::to_string(c) + ": ";
    if (!ipp_is_class(N, k.n)) return who + "the vector length must be a power of two, at most the prover's";
    if (k.count == 0) return who + "n_proofs must be at least 1";
    if (k.count > PROVER_PROOFS_MAX) return "at most 2^20 proofs per call";
    proofs += k.count;
    elems += k.count * k.n;
    if (proofs > PROVER_PROOFS_MAX) return "at most 2^20 proofs per call";
    if (elems > PROVER_BATCH_ELEMS_MAX) return "at most 2^27 elements (proofs x n) per call";
  }
  return std::string();
}

// what a launch runs; a launch's blocks are the concatenated blocks of its units
enum IppmKind : u32 { IPPM_BEGIN, IPPM_ROUND_WIDE, IPPM_MSM, IPPM_HEAD, IPPM_AFFINE, IPPM_ROUND_CHAL, IPPM_COMMIT_SCALARS };
static inline const char *ippm_kind_name(u32 kind) {
  static const char *const names[] = {"k_ip_begin_mixed", "k_ip_round_wide_mixed", "k_pv_msm_mixed", "k_ip_head_mixed", "k_ip_affine_mixed", "k_ip_round_chal_mixed",
                                      "k_ip_commit_scalars_mixed"};
  return names[kind];
}
struct IppmLaunch {
  u32 kind = 0, step = 0;
  u32 threads = 0;                               // per block: 64 (one lane per proof), 256, or the NT of a wide kernel
  u32 gl = 0;                                    // IPPM_MSM: log2 of the lanes per job (1, 4 or 6)
  u32 round = 0, first = 0;                      // IPPM_ROUND_*, IPPM_AFFINE: the round; IPPM_ROUND_WIDE first = 1: no fold
  u32 blocks = 0, first_unit = 0, n_units = 0;   // units[first_unit, first_unit + n_units)
};
// a class's jobs of a step's multi-scalar multiplication (rpp::MsmJobs without the pointers); from_hsc: the head's scalars, else jsc
struct IppmJobs { u32 njobs = 0, ntypes = 0, T = 0, stride = 0, base_off = 0, from_hsc = 0; };

struct IppRegions {
  size_t o_dig0 = 0, o_dlen = 0, o_ain = 0, o_bin = 0, o_cin = 0, o_Pin = 0;                                         // inputs (uploaded)
  size_t o_uc = 0, o_hsc = 0, o_xr = 0, o_a = 0, o_b = 0, o_cg = 0, o_hf = 0, o_jsc = 0, o_jout = 0;                 // scratch
  size_t o_ab = 0, o_xs = 0, o_lr = 0, o_head = 0, o_trlen = 0, o_tr = 0;                                            // outputs (come back)
};
// the transcript's start as the host stages it and the transcript's bound, both rounded up to 16 (ipa_prove_host.hpp states the same)
struct IppStrides { u32 dig0_stride = 0, tr_stride = 0; };
static inline IppStrides ipp_strides(u32 k, int protocol, uint64_t seed_max) {
  IppStrides s;
  s.dig0_stride = (u32)(((protocol == 1 ? ((seed_max + 2) / 3) * 4 + 1 : 1 + seed_max) + 15) & ~15ull);
  s.tr_stride = (u32)((ipp_transcript_bytes(k, protocol, seed_max) + 15) & ~15ull);
  return s;
}
static inline void ipp_take_inputs(IppRegions &r, RppTake &take, size_t P, size_t n, const IppStrides &s, bool have_c) {
  r.o_dig0 = take(P * s.dig0_stride); r.o_dlen = take(4 * P); r.o_ain = take(32 * P * n); r.o_bin = take(32 * P * n);
  r.o_cin = take(have_c ? 32 * P : 0);
}
static inline void ipp_take_scratch(IppRegions &r, RppTake &take, size_t P, size_t n) {
  r.o_uc = take(32 * P); r.o_hsc = take(64 * P); r.o_xr = take(64 * P);
  r.o_a = take(32 * P * n); r.o_b = take(32 * P * n); r.o_cg = take(32 * P * n); r.o_hf = take(32 * P * n);
  r.o_jsc = take(32 * 2 * P * (n + 1)); r.o_jout = take(144 * 2 * P);
}
static inline void ipp_take_outputs(IppRegions &r, RppTake &take, size_t P, size_t k, const IppStrides &s) {
  r.o_ab = take(64 * P); r.o_xs = take(32 * P * k); r.o_lr = take(128 * P * k); r.o_head = take(128 * P);
  r.o_trlen = take(4 * P); r.o_tr = take(P * s.tr_stride);
}

struct IppmClass : IppStrides, IppRegions {
  u32 n = 0, k = 0, NT = 0, per_block = 0;      // the geometry by ipp_plan's rules
  uint64_t count = 0, first = 0;                // proofs; the call-wide index of proof 0 (class-major in the caller's order)
  size_t bases_off = 0;                         // its lists in the capacity's array (entries)
  uint64_t tr_bytes = 0;                        // ipp_transcript_bytes of its longest seed: cap_c >= count x tr_bytes
};

struct IppmPlan {
  int err = 0; std::string msg;                  // an argument error: nothing else is set
  u32 N = 0, k_max = 0, nsteps = 0;
  int protocol = 0;
  std::vector<IppmClass> cls;
  uint64_t n_proofs = 0;
  // device buffer: [the classes' inputs | Batch array | AffineJob array | MsmJobs array | unit table] uploaded in one copy, then the classes'
  // scratch, then the classes' outputs (contiguous: [o_out, need) comes down in one copy)
  size_t o_P = 0, o_P_end = 0, o_batch = 0, o_affine = 0, o_jobs = 0, o_units = 0, in_bytes = 0, o_out = 0, need = 0;
  std::vector<RppmUnit> units;
  std::vector<IppmLaunch> launches;              // in launch order; launches of step s are contiguous
  std::vector<IppmJobs> jobs;                    // [step][class], steps 0 .. k_max (njobs = 0: the class has no multiplication in the step)
};
static inline IppmPlan ippm_error(const std::string &msg) { IppmPlan p; p.err = BPMI_E_ARG; p.msg = msg; return p; }

// units and launches of either plan: blocks_of(class) = 0 leaves the class out of the launch; an empty launch is dropped
template <class Plan, class F> static inline void ippm_add_launch(Plan &p, u32 n_classes, IppmLaunch L, F &&blocks_of) {
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
}
static inline u32 ippm_ceil_div(uint64_t a, uint64_t b) { return (u32)((a + b - 1) / b); }

// protocol: 1 or 2 (checked by the caller's ipp_call_error); job_lanes: option "prover_job_lanes"
static inline IppmPlan ipp_mixed_plan(uint32_t N, int protocol, uint32_t n_classes, const IppmClassIn *classes, int job_lanes) {
  {
    const std::string bad = ippm_args_error(N, n_classes, classes);
    if (!bad.empty()) return ippm_error(bad);
  }
  for (u32 c = 0; c < n_classes; c++)
    if (classes[c].seed_max > IPP_SEED_MAX) return ippm_error("class " + std::to_string(c) + ": a seed is longer than 65535 bytes");
  IppmPlan p;
  p.N = N; p.protocol = protocol;
  p.cls.resize(n_classes);
  RppTake take;
  for (u32 c = 0; c < n_classes; c++) {
    const IppmClassIn &k = classes[c];
    IppmClass &q = p.cls[c];
    q.n = k.n;
    while ((1u << q.k) < q.n) q.k++;
    q.NT = q.n <= 256u ? 256u : q.n;
    q.per_block = q.NT / q.n;
    q.count = k.count;
    q.first = c ? p.cls[c - 1].first + p.cls[c - 1].count : 0;
    static_cast<IppStrides &>(q) = ipp_strides(q.k, protocol, k.seed_max);
    q.bases_off = ipp_capacity_bases_off(N, q.n);
    q.tr_bytes = ipp_transcript_bytes(q.k, protocol, k.seed_max);
    p.n_proofs += q.count;
    if (q.k > p.k_max) p.k_max = q.k;
    ipp_take_inputs(q, take, (size_t)q.count, q.n, q, protocol == 1 && k.have_c);
  }
  // the statement points of every class back to back (a region's padding stays zero, and 64 zero bytes are the identity): ONE on-curve
  // check covers [o_P, o_P_end), a bad point's class is found from its offset
  p.o_P = take.o;
  for (IppmClass &q : p.cls) q.o_Pin = take(protocol == 1 ? 64 * (size_t)q.count : 0);
  p.o_P_end = take.o;
  p.nsteps = n_classes ? 1 + p.k_max : 0;
  p.jobs.assign((size_t)p.nsteps * n_classes, IppmJobs());
  auto simple = [&](u32 kind, u32 step, u32 threads, auto &&blocks_of, u32 round = 0, u32 first = 0) {
    IppmLaunch L; L.kind = kind; L.step = step; L.threads = threads; L.round = round; L.first = first;
    ippm_add_launch(p, n_classes, L, blocks_of);
  };
  auto wide = [&](u32 step, auto &&in_step, u32 round, u32 first) {
    for (u32 NT = 256; NT <= 1024; NT <<= 1)
      simple(IPPM_ROUND_WIDE, step, NT, [&](u32 c) { return in_step(c) && p.cls[c].NT == NT ? ippm_ceil_div(p.cls[c].count, p.cls[c].per_block) : 0u; }, round, first);
  };
  // the multiplication of a step: one launch per lane width, a class's width by the jobs of the whole step (ipp_job_lanes_log2);
  // forced_gl: the head's one-term jobs run two lanes per job, as in bpmi_ipa_prove_batch
  auto msm = [&](u32 step, auto &&J, int forced_gl) {
    uint64_t total = 0;
    for (u32 c = 0; c < n_classes; c++) { IppmJobs &j = p.jobs[(size_t)step * n_classes + c]; J(c, j); total += j.njobs; }
    const int widths[3] = {1, 4, 6};
    for (int gl : widths) {
      IppmLaunch L; L.kind = IPPM_MSM; L.step = step; L.threads = 256; L.gl = (u32)gl;
      ippm_add_launch(p, n_classes, L, [&](u32 c) {
        const IppmJobs &j = p.jobs[(size_t)step * n_classes + c];
        if (!j.njobs) return 0u;
        const int mine = forced_gl ? forced_gl : ipp_job_lanes_log2(p.cls[c].n, total, job_lanes);
        return mine == gl ? ippm_ceil_div((uint64_t)j.njobs << gl, 256) : 0u;
      });
    }
  };
  auto all = [](u32) { return true; };
  auto chain = [&](u32 c) { return ippm_ceil_div(p.cls[c].count, 64); };
  auto pairs = [&](u32 c) { return ippm_ceil_div(2 * p.cls[c].count, 256); };
  if (n_classes) {
    // step 0: the transcripts' start, the state and the scalars of round 0; under Protocol 1 the head
    simple(IPPM_BEGIN, 0, 64, chain);
    wide(0, all, 0, 1);
    if (protocol == 1) {
      msm(0, [&](u32 c, IppmJobs &j) { j.njobs = 2 * (u32)p.cls[c].count; j.ntypes = 1; j.T = 1; j.stride = 1; j.base_off = 0; j.from_hsc = 1; }, 1);
      simple(IPPM_HEAD, 0, 256, pairs);
    }
    // steps 1 .. k_max: round r for the classes with k_c > r
    for (u32 r = 0; r < p.k_max; r++) {
      auto in_round = [&](u32 c) { return p.cls[c].k > r; };
      msm(1 + r, [&](u32 c, IppmJobs &j) {
        const IppmClass &q = p.cls[c];
        if (q.k <= r) return;
        j.njobs = 2 * (u32)q.count; j.ntypes = 2; j.T = q.n + 1; j.stride = q.n + 1; j.base_off = 1 + r * 2 * (q.n + 1);
      }, 0);
      simple(IPPM_AFFINE, 1 + r, 256, [&](u32 c) { return in_round(c) ? pairs(c) : 0u; }, r, 0);
      simple(IPPM_ROUND_CHAL, 1 + r, 64, [&](u32 c) { return in_round(c) ? chain(c) : 0u; }, r, 0);
      wide(1 + r, in_round, r, 0);
    }
  }
  p.o_batch = take((size_t)IPPM_BATCH_SLOT * n_classes);
  p.o_affine = take((size_t)IPPM_AFFINE_SLOT * n_classes);
  p.o_jobs = take((size_t)IPPM_JOBS_SLOT * p.jobs.size());
  p.o_units = take(sizeof(RppmUnit) * p.units.size());
  p.in_bytes = take.o;
  for (IppmClass &q : p.cls) ipp_take_scratch(q, take, (size_t)q.count, q.n);
  p.o_out = take.o;
  for (IppmClass &q : p.cls) ipp_take_outputs(q, take, (size_t)q.count, q.k, q);
  p.need = take.o;
  return p;
}

// ---- the statements of such a block (bpmi_ipa_batch_prover_commit_batch_mixed) ---------------------------------------------------------
struct IppmCommitClass {
  u32 n = 0, NT = 0, per_block = 0, T = 0;      // T: terms of a job, n per given half and one under a u_mode
  uint64_t count = 0;
  size_t bases_off = 0;                         // its list in the capacity's statement array (entries)
  size_t o_ain = 0, o_bin = 0, o_tin = 0;       // inputs (uploaded)
  size_t o_jsc = 0, o_jout = 0;                 // scratch
  size_t o_pts = 0;                             // output
};
struct IppmCommitPlan {
  int err = 0; std::string msg;
  u32 N = 0;
  std::vector<IppmCommitClass> cls;
  uint64_t count = 0;
  // [the classes' inputs | Commit array | AffineJob array | MsmJobs array | unit table] uploaded in one copy, the scratch, the points (contiguous)
  size_t o_commit = 0, o_affine = 0, o_jobs = 0, o_units = 0, in_bytes = 0, o_out = 0, need = 0;
  std::vector<RppmUnit> units;
  std::vector<IppmLaunch> launches;
  std::vector<IppmJobs> jobs;                    // [class]
};
// u_mode and the NULL rules per class are the caller's (ipp_commit_error)
static inline IppmCommitPlan ipp_mixed_commit_plan(uint32_t N, int u_mode, uint32_t n_classes, const IppmClassIn *classes, int job_lanes) {
  IppmCommitPlan p;
  {
    const std::string bad = ippm_args_error(N, n_classes, classes);
    if (!bad.empty()) { p.err = BPMI_E_ARG; p.msg = bad; return p; }
  }
  p.N = N;
  p.cls.resize(n_classes);
  p.jobs.assign(n_classes, IppmJobs());
  RppTake take;
  uint64_t total = 0;
  for (u32 c = 0; c < n_classes; c++) {
    const IppmClassIn &k = classes[c];
    IppmCommitClass &q = p.cls[c];
    q.n = k.n; q.NT = q.n <= 256u ? 256u : q.n; q.per_block = q.NT / q.n; q.count = k.count;
    q.T = (k.have_a ? q.n : 0u) + (k.have_b ? q.n : 0u) + (u_mode ? 1u : 0u);
    q.bases_off = ipp_capacity_commit_bases_off(N, q.n) + ipp_commit_bases_offset(q.n, k.have_a, k.have_b);
    const size_t C = (size_t)q.count;
    q.o_ain = take(k.have_a ? 32 * C * q.n : 0); q.o_bin = take(k.have_b ? 32 * C * q.n : 0); q.o_tin = take(k.have_t ? 32 * C : 0);
    IppmJobs &j = p.jobs[c];
    j.njobs = (u32)q.count; j.ntypes = 1; j.T = q.T; j.stride = q.T; j.base_off = 0;
    p.count += q.count;
    total += q.count;
  }
  if (n_classes) {
    for (u32 NT = 256; NT <= 1024; NT <<= 1) {
      IppmLaunch L; L.kind = IPPM_COMMIT_SCALARS; L.threads = NT;
      ippm_add_launch(p, n_classes, L, [&](u32 c) { return p.cls[c].NT == NT ? ippm_ceil_div(p.cls[c].count, p.cls[c].per_block) : 0u; });
    }
    const int widths[3] = {1, 4, 6};
    for (int gl : widths) {
      IppmLaunch L; L.kind = IPPM_MSM; L.threads = 256; L.gl = (u32)gl;
      ippm_add_launch(p, n_classes, L, [&](u32 c) {
        return ipp_job_lanes_log2(p.cls[c].n, total, job_lanes) == gl ? ippm_ceil_div((uint64_t)p.jobs[c].njobs << gl, 256) : 0u;
      });
    }
    IppmLaunch L; L.kind = IPPM_AFFINE; L.threads = 256;
    ippm_add_launch(p, n_classes, L, [&](u32 c) { return ippm_ceil_div(p.cls[c].count, 256); });
  }
  p.o_commit = take((size_t)IPPM_COMMIT_SLOT * n_classes);
  p.o_affine = take((size_t)IPPM_AFFINE_SLOT * n_classes);
  p.o_jobs = take((size_t)IPPM_JOBS_SLOT * n_classes);
  p.o_units = take(sizeof(RppmUnit) * p.units.size());
  p.in_bytes = take.o;
  for (IppmCommitClass &q : p.cls) { q.o_jsc = take(32 * (size_t)q.count * q.T); q.o_jout = take(144 * (size_t)q.count); }
  p.o_out = take.o;
  for (IppmCommitClass &q : p.cls) { q.o_pts = take.o; take.o += 64 * (size_t)q.count; }      // the points of all classes back to back: one copy, class-major
  p.need = (take.o + 255) & ~(size_t)255;
  return p;
}
