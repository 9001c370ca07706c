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

// The shape of a proof of m values of nbits bits: what rpp_plan, a class of a mixed call and the proof-size calls derive from (nbits, m)
struct RppGeom {
  u32 m = 0, n = 0, k = 0;                     // values per proof, n = nbits m elements, k = log2 n rounds
  u32 NT = 0, per_block = 0;                   // threads of a block of the n-lanes-per-proof kernels, proofs it holds
  u32 npt = 0;                                 // points of a proof: 6 + 2k
};
static inline RppGeom rpp_geom(u32 nbits, u32 m) {
  RppGeom g;
  g.m = m; g.n = nbits * m;
  while ((1u << g.k) < g.n) g.k++;
  g.NT = g.n <= 256u ? 256u : g.n;                               // 256, 512 or 1 024: a proof never straddles blocks
  g.per_block = g.NT / g.n;
  g.npt = 6 + 2 * g.k;
  return g;
}
// bytes of a proof without its seed; wire_fmt: option "prover_wire_format" (3: with the points' y coordinates)
static inline uint64_t rpp_fixed_bytes(u32 k, int wire_fmt) { return 6 + 32 * (5 + (uint64_t)k) + 33 * (6 + 2 * (uint64_t)k) + 128 + 2 + 2 + (wire_fmt == 3 ? 32 * (6 + 2 * (uint64_t)k) : 0); }

struct RppPlan : RppGeom {
  int err = 0; const char *msg = nullptr;      // an argument error: nothing else is set
  u32 nb = 0;                                  // bits per value
  u32 nbases = 0;                              // 3 + 2n: g, h, u, gs, hs
  u32 tw = 0, wt = 0, bt = 0;                  // table windows: tw bits, wt = ceil(256 / tw) per scalar, bt = 2^(tw-1) entries each
  uint64_t table_bytes = 0;
  uint64_t max_proofs = 0;                     // per call: min(2^20, 2^27 / n)
  u32 off_S = 0, off_T = 0, off_P = 0, off_round = 0;          // rpp_off_*: where the lists of `bases` start
  std::vector<unsigned short> bases;           // rpp_class_bases(n, n)
};

// The base lists of a proof of n elements, in entries: S and P_new 2n + 1 (gs_0.., hs_0.., then h / u), T 2 (g, h), round r: L then R,
// n + 1 each (rp_prove_kernels.hpp k_pv_round_wide).  Functions of n alone: a class of a mixed call has the offsets of its own n
static inline u32 rpp_off_S(u32) { return 0; }
static inline u32 rpp_off_T(u32 n) { return 2 * n + 1; }
static inline u32 rpp_off_P(u32 n) { return 2 * n + 3; }
static inline u32 rpp_off_round(u32 n, u32 r) { return 4 * n + 4 + r * 2 * (n + 1); }
static inline size_t rpp_class_bases_len(u32 n) {
  u32 k = 0;
  while ((1u << k) < n) k++;
  return rpp_off_round(n, k);
}
// The lists over the first n of N generators (n <= N: a class of a mixed call under a capacity of N; n == N: the prover's own): gs_i at
// base 3 + i, hs_i at base 3 + N + i
static inline std::vector<unsigned short> rpp_class_bases(u32 n, u32 N) {
  std::vector<unsigned short> bl;
  bl.reserve(rpp_class_bases_len(n));
  for (int pass = 0; pass < 2; pass++) {                   // S: .., h;  T: g, h;  P_new: .., u
    for (u32 i = 0; i < n; i++) bl.push_back((unsigned short)(3 + i));
    for (u32 i = 0; i < n; i++) bl.push_back((unsigned short)(3 + N + i));
    bl.push_back(pass == 0 ? 1 : 2);
    if (pass == 0) { bl.push_back(0); bl.push_back(1); }
  }
  for (u32 len = n; len > 1; len >>= 1) {                  // round r: len = n >> r
    const u32 half = len >> 1;
    for (int side = 0; side < 2; side++) {                 // 0: L, 1: R
      for (u32 j = 0; j < n; j++) if (((j & (len - 1)) >= half) == (side == 0)) bl.push_back((unsigned short)(3 + j));
      for (u32 j = 0; j < n; j++) if (((j & (len - 1)) < half) == (side == 0)) bl.push_back((unsigned short)(3 + N + j));
      bl.push_back(2);
    }
  }
  return bl;
}

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
  static_cast<RppGeom &>(p) = rpp_geom(nbits, m);
  p.nb = nbits;
  const u32 n = p.n;
  p.nbases = 3 + 2 * n;
  p.tw = opt_tw ? (u32)opt_tw : rpp_default_table_bits(n);
  p.wt = (256u + p.tw - 1u) / p.tw; p.bt = 1u << (p.tw - 1u);
  p.table_bytes = rpp_table_bytes(n, p.tw);
  p.max_proofs = PROVER_BATCH_ELEMS_MAX / n < PROVER_PROOFS_MAX ? PROVER_BATCH_ELEMS_MAX / n : PROVER_PROOFS_MAX;
  p.off_S = rpp_off_S(n); p.off_T = rpp_off_T(n); p.off_P = rpp_off_P(n); p.off_round = rpp_off_round(n, 0);
  p.bases = rpp_class_bases(n, n);
  return p;
}

// the per-call caps of bpmi_rp_prove_batch (max_proofs: the plan's): nullptr, or the text of the BPMI_E_ARG (checked before anything is allocated)
static inline const char *rpp_batch_error(uint64_t max_proofs, uint64_t n_proofs) {
  if (n_proofs > PROVER_PROOFS_MAX) return "at most 2^20 proofs per call";
  if (n_proofs > max_proofs) return "at most 2^27 elements (proofs x bits x values) per call";
  return nullptr;
}

// Bytes per proof of the transcript's start (base64 of the longest seed, '&') and of the transcript buffer: the longer of the range
// proof's (start, 4 points, 3 scalars) and the inner product's (ip_prefix_len: bytes of "&&" str(x_ip) "&", then k rounds), then a hash block
struct RppStrides { u32 dig0_stride = 0, tr_stride = 0; };
static inline RppStrides rpp_strides(uint64_t seed_max, u32 k, size_t ip_prefix_len) {
  RppStrides s;
  s.dig0_stride = (u32)((((seed_max + 2) / 3) * 4 + 1 + 15) & ~15ull);
  const uint64_t tr_a = (uint64_t)s.dig0_stride + 4 * 45 + 3 * 80, tr_b = ip_prefix_len + (uint64_t)k * (90 + 80);
  s.tr_stride = (u32)(((tr_a > tr_b ? tr_a : tr_b) + 64 + 15) & ~15ull);
  return s;
}

// The device arrays of P proofs of one shape (every array of rpp::Batch), in bytes from the start of the prover's device buffer, each
// rounded up to 256 by the RppTake that lays a call out.  Inputs (uploaded): dig0, dlen, val, gam.  Scratch: the rest.
struct RppTake {
  size_t o = 0;
  size_t operator()(size_t bytes) { const size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; }
};
struct RppRegions {
  size_t o_dig0 = 0, o_dlen = 0, o_val = 0, o_gam = 0;
  size_t o_tr = 0, o_trlen = 0, o_slr = 0, o_alpha = 0, o_chal = 0, o_tau = 0, o_tsc = 0, o_res = 0, o_xs = 0, o_xr = 0, o_a = 0, o_b = 0, o_cg = 0, o_hf = 0, o_jsc = 0, o_jout = 0, o_pts = 0;
};
static inline void rpp_take_inputs(RppRegions &r, RppTake &take, const RppGeom &g, size_t P, const RppStrides &s) {
  r.o_dig0 = take(P * s.dig0_stride); r.o_dlen = take(4 * P); r.o_val = take(32 * P * g.m); r.o_gam = take(32 * P * g.m);
}
static inline void rpp_take_scratch(RppRegions &r, RppTake &take, const RppGeom &g, size_t P, const RppStrides &s) {
  const size_t n = g.n;
  r.o_tr = take(P * s.tr_stride); r.o_trlen = take(4 * P);
  r.o_slr = take(32 * P * (2 * n + 1)); r.o_alpha = take(32 * P); r.o_chal = take(128 * P); r.o_tau = take(64 * P); r.o_tsc = take(128 * P);
  r.o_res = take(160 * P); r.o_xs = take(32 * P * g.k); r.o_xr = take(64 * P);
  r.o_a = take(32 * P * n); r.o_b = take(32 * P * n); r.o_cg = take(32 * P * n); r.o_hf = take(32 * P * n);
  r.o_jsc = take(32 * P * (2 * n + 2)); r.o_jout = take(144 * 2 * P); r.o_pts = take(64 * P * g.npt);
}
// The whole device buffer of bpmi_rp_prove_batch: [inputs | seeds | seed offsets | output offsets] uploaded in one copy, then the scratch,
// then the output bytes -- a one-class mixed plan (rp_prove_mixed_plan_host.hpp) without its three device tables
struct RppLayout : RppStrides, RppRegions {
  size_t o_seeds = 0, o_soff = 0, o_ooff = 0, in_bytes = 0, o_out = 0, need = 0;
};
static inline RppLayout rpp_layout(const RppGeom &g, size_t P, size_t seed_bytes, uint64_t seed_max, uint64_t total_out, size_t ip_prefix_len) {
  RppLayout L;
  static_cast<RppStrides &>(L) = rpp_strides(seed_max, g.k, ip_prefix_len);
  RppTake take;
  rpp_take_inputs(L, take, g, P, L);
  L.o_seeds = take(seed_bytes + 16); L.o_soff = take(8 * (P + 1)); L.o_ooff = take(8 * (P + 1));
  L.in_bytes = take.o;
  rpp_take_scratch(L, take, g, P, L);
  L.o_out = take((size_t)total_out + 16);
  L.need = take.o;
  return L;
}

// log2 of the lanes k_pv_msm gives a job: 4, or 6 (a wave).  opt: option "prover_job_lanes" (0 automatic, 16, 64).  Automatic: 16 for
// proofs of up to 128 elements whatever the batch; above, a wave while the launch has at most PROVER_WAVE_JOBS_MAX jobs
static inline int rpp_job_lanes_log2(u32 elems, uint64_t njobs, int opt) {
  if (opt == 16) return 4;
  if (opt == 64) return 6;
  return elems > PROVER_ELEMS_SMALL && njobs <= PROVER_WAVE_JOBS_MAX ? 6 : 4;
}
