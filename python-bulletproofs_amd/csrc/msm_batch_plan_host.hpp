// msm_batch_plan_host.hpp -- part of libbpmi; plain C++17 (no HIP, no bpmi_ctx), also compiled for the host by tests/csrc_host.
// The plan of a batched MSM -- n_vec scalar vectors over ONE shared point set of up to three segments, n_vec results
// (bpmi_msm_batch, bpmi_msm_batch_dev, bpmi_msm_batch_dev_enqueue) -- as a pure function of the sizes and the options: the argument
// errors, the route, the launch geometry, the row ranges of a batch whose window sums do not fit one launch, and the layout of the
// workspace.  tests/test_msm_batch_plan_cpu.py checks it without a GPU; msm_batch_host.hpp consumes it.  Kernels: k_msm_batch and
// k_msm_batch_tail (msm_kernels.hpp) over the body of the one-block-per-window kernel, msm_mid_block.
#pragma once
#include "shared_defs.hpp"

#define MSMB_VECS_MAX (1ull << 20)             // vectors per call
#define MSMB_WORK_MAX (1ull << 30)             // vectors x pairs per call
#define MSMB_PARTS_MAX 4u                      // blocks per window ("mid_parts" runs the body with 1 .. 4)
#define MSMB_E_BYTES_MAX (256ull << 20)        // window sums of one launch
#define MSMB_LIGHT_THREADS GROUP_LIGHT_THREADS // the two shapes of msm_mid_block that exist (msm_kernels.hpp: k_msm_group runs both)
#define MSMB_MID_THREADS 512u
#define MSMB_ROUTE_NONE 0u                     // no pair at all: n_vec identities, nothing is launched
#define MSMB_ROUTE_LIGHT 1u                    // total <= GROUP_LIGHT_NMAX: 256 threads, 52 KB of LDS, three blocks per CU
#define MSMB_ROUTE_MID 2u                      // total <= 4 MID_NMAX: 512 threads, 139 KB of LDS, ceil(total / MID_NMAX) blocks per window (automatic: up to 3)
#define MSMB_ROUTE_LOOP 3u                     // one msm_run per vector on the row's segments: the same 64 bytes
// The AUTOMATIC route's bounds, measured against the faster of a loop of bpmi_msm_dev and the three-slot rotation of bpmi_msm_dev_enqueue
// (profiles/r10_msm_batch.txt).  Every vector's Horner chain over the windows (36 x 7 doublings, an addition per
// window and part, one inversion) is ONE lane of the tail kernel -- 0.9 ms whatever the batch size -- where the single MSMs combine their
// windows on the host: a batch of fewer than min_vecs vectors runs as the loop.  With one or two blocks per window the batch passes the
// rotation between 24 and 32 vectors (129, 512, 513, 8 193, 16 896 pairs), with three between 32 and 64 (25 344 pairs); with four it
// stays behind it at 16, 64 and 128 vectors (33 792 pairs: 1.85x, 1.17x, 1.08x), where the bucket pipeline's wider windows do less work
// per pair than 7-bit windows in LDS: the automatic route takes at most three parts.  A forced route ("msm_batch_route") ignores both.
#define MSMB_AUTO_PARTS_MAX 3u
static inline u32 msmb_min_vecs(u32 parts) { return parts >= 3u ? 64u : 32u; }

struct MsmBatchPlan {
  int err = 0; const char *msg = nullptr;      // an argument error: nothing else is set
  u32 route = MSMB_ROUTE_NONE;
  uint64_t total = 0, n_vec = 0;               // pairs per vector (the sum of the segments); vectors
  u32 threads = 0, nmax = 0;                   // block shape of k_msm_batch: <threads, nmax> (0 on the LOOP route)
  u32 parts = 0;                               // blocks per window (gridDim.z)
  u32 W = 0;                                   // windows of MID_C bits (gridDim.x = vecs x W)
  u32 vecs = 0, launches = 0;                  // vectors per launch; launch k runs rows [k vecs, min((k + 1) vecs, n_vec))
  // the workspace: byte offsets into lane 0's workspace, every region on a 256-byte line
  //   window sums 144 W parts vecs (one launch's; the next launch reuses them: same stream) | results 64 n_vec (only the host-out forms)
  uint64_t o_E = 0, b_E = 0, o_out = 0, b_out = 0, total_bytes = 0;
};

static inline MsmBatchPlan msmb_plan_error(const char *msg) { MsmBatchPlan p; p.err = BPMI_E_ARG; p.msg = msg; return p; }
// rows of launch k
static inline void msmb_range(const MsmBatchPlan &p, u32 k, uint64_t &v0, u32 &cnt) {
  v0 = (uint64_t)k * p.vecs;
  cnt = (u32)(p.n_vec - v0 < p.vecs ? p.n_vec - v0 : p.vecs);
}

// n: nseg pair counts (an empty segment is allowed).  host_out: the results are copied to host memory, so they need a device region.
// Options: opt_msm_batch_route (0 automatic, 1 / 2 / 3 forces LIGHT / MID / LOOP), opt_msm_batch_vecs (0 automatic, else vectors per launch).
static inline MsmBatchPlan msm_batch_plan(const BpmiOptions &o, u32 nseg, const uint64_t *n, uint64_t n_vec, bool host_out) {
  if (nseg < 1 || nseg > 3) return msmb_plan_error("nseg must be 1 .. 3");
  if (!n) return msmb_plan_error("null argument");
  uint64_t total = 0;
  for (u32 s = 0; s < nseg; s++) {
    if (n[s] > BPMI_MAX_N) return msmb_plan_error("the pairs of a vector (all segments) exceed BPMI_MAX_N");
    total += n[s];
  }
  if (total > BPMI_MAX_N) return msmb_plan_error("the pairs of a vector (all segments) exceed BPMI_MAX_N");
  if (n_vec > MSMB_VECS_MAX) return msmb_plan_error("at most 2^20 vectors per call");
  if (n_vec * total > MSMB_WORK_MAX) return msmb_plan_error("at most 2^30 pairs (n_vec x pairs of a vector) per call");
  MsmBatchPlan p;
  p.total = total; p.n_vec = n_vec;
  if (total == 0 || n_vec == 0) return p;
  const uint64_t mid_max = (uint64_t)MSMB_PARTS_MAX * MID_NMAX;
  const int forced = o.opt_msm_batch_route;
  if (forced == (int)MSMB_ROUTE_LIGHT && total > GROUP_LIGHT_NMAX) return msmb_plan_error("msm_batch_route = 1 (LIGHT) takes at most 512 pairs per vector");
  if (forced == (int)MSMB_ROUTE_MID && total > mid_max) return msmb_plan_error("msm_batch_route = 2 (MID) takes at most 33792 pairs per vector");
  if (forced >= 1 && forced <= 3) p.route = (u32)forced;
  else if (total > (uint64_t)MSMB_AUTO_PARTS_MAX * MID_NMAX || n_vec < msmb_min_vecs((u32)((total + MID_NMAX - 1) / MID_NMAX))) p.route = MSMB_ROUTE_LOOP;
  else p.route = total <= GROUP_LIGHT_NMAX ? MSMB_ROUTE_LIGHT : MSMB_ROUTE_MID;
  if (p.route == MSMB_ROUTE_LOOP) return p;
  p.W = 255u / MID_C + 1u;
  if (p.route == MSMB_ROUTE_LIGHT) { p.threads = MSMB_LIGHT_THREADS; p.nmax = GROUP_LIGHT_NMAX; p.parts = 1; }
  else { p.threads = MSMB_MID_THREADS; p.nmax = MID_NMAX; p.parts = (u32)((total + MID_NMAX - 1) / MID_NMAX); }
  const uint64_t per_vec = 4ull * XYZZ_WORDS * p.W * p.parts;                  // 144 B per (window, part)
  uint64_t vecs = MSMB_E_BYTES_MAX / per_vec;
  if (o.opt_msm_batch_vecs > 0 && (uint64_t)o.opt_msm_batch_vecs < vecs) vecs = (uint64_t)o.opt_msm_batch_vecs;
  if (vecs > n_vec) vecs = n_vec;
  p.vecs = (u32)vecs;
  p.launches = (u32)((n_vec + vecs - 1) / vecs);
  p.b_E = per_vec * vecs;
  p.b_out = host_out ? 64 * n_vec : 0;
  uint64_t at = 0;
  auto take = [&at](uint64_t bytes) { const uint64_t off = at; at += align_up(bytes, 256); return off; };
  p.o_E = take(p.b_E); p.o_out = take(p.b_out);
  p.total_bytes = at;
  return p;
}
