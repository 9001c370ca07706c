// The MSM planner (csrc/msm_plan_host.hpp) behind flat arrays, for tests only: host_shim.cpp exports these to
// tests/test_msm_plan_cpu.py, host_native_fuzz.cpp runs them under the sanitizers on heap blocks of exactly these sizes.
#pragma once
#include <stdint.h>
#include <stddef.h>

#include "msm_plan_host.hpp"
#include "options_flat.hpp"        // kv: (row of the option's name, value) pairs
static inline MsmMode plan_mode(uint32_t bits) {          // 1 chained, 2 free_run, 4 beside
  MsmMode m;
  m.chained = bits & 1u; m.free_run = bits & 2u; m.beside = bits & 4u;
  return m;
}

#define PLAN_GEOM_WORDS 16       // n c W w0 B G L nv prio fuse top2 inblock | mid small glv mid_parts
#define PLAN_LAYOUT_WORDS 30     // the 24 regions' offsets in msm_layout's order | total (placed) total (sizing pass) P nscan_blocks rec0_max nchunks
#define PLAN_JOB_WORDS 12        // in_off in_stride N s type glanes gpw nsums out_off out_stride blk0 cnt
#define PLAN_JOBS_WORDS (2 + 4 * PLAN_JOB_WORDS)      // njobs prio | 4 jobs
#define PLAN_REDUCE_WORDS (3 * PLAN_JOBS_WORDS + 12)  // j1 j2 j2top | grid1 top_w | to: nv off[4] top top_off[4]

static inline void plan_flat_jobs(uint32_t *out, const DigitJobs &J) {
  out[0] = J.njobs; out[1] = J.prio;
  for (int k = 0; k < 4; k++) {
    const DigitJob &j = J.j[k];
    const uint32_t f[PLAN_JOB_WORDS] = {j.in_off, j.in_stride, j.N, j.s, j.type, j.glanes, j.gpw, j.nsums, j.out_off, j.out_stride, j.blk0, j.cnt};
    for (int i = 0; i < PLAN_JOB_WORDS; i++) out[2 + PLAN_JOB_WORDS * k + i] = f[i];
  }
}
// geometry, layout and reduction of one MSM; returns the window bits pick_window_bits gives for n (what msm_run_split forms its groups from)
static inline uint32_t plan_flat(const int32_t *kv, int nkv, uint64_t n, uint32_t w0, uint32_t wcount, uint32_t mode_bits,
                                 uint32_t geom[PLAN_GEOM_WORDS], uint64_t layout[PLAN_LAYOUT_WORDS], uint32_t reduce[PLAN_REDUCE_WORDS]) {
  const BpmiOptions o = plan_options(kv, nkv);
  const MsmPlan pl = msm_pick_geometry(o, plan_mode(mode_bits), n, w0, wcount);
  const MsmGeom &g = pl.g;
  const uint32_t gw[PLAN_GEOM_WORDS] = {g.n, g.c, g.W, g.w0, g.B, g.G, g.L, g.nv, g.prio, g.fuse, g.top2, g.inblock, pl.mid, pl.small, pl.glv, mid_parts(o, n)};
  for (int i = 0; i < PLAN_GEOM_WORDS; i++) geom[i] = gw[i];
  MsmWs sized, w;
  msm_layout(g, sized, nullptr, pl.glv);
  char *const base = (char *)(uintptr_t)(1ull << 40);       // never dereferenced: only the offsets are read back
  msm_layout(g, w, base, pl.glv);
  const void *const region[24] = {w.glv_sub, w.glv_bx, w.glv_neg, w.hist, w.off, w.cursor, w.bsum, w.coarse_hist, w.coarse_off, w.coarse_cursor, w.dig, w.sidx,
                                  w.dig16, w.negs, w.chunk_key, w.buckets, w.rec_key[0], w.rec_pt[0], w.rec_key[1], w.rec_pt[1], w.D, w.E, w.F, w.out};
  for (int i = 0; i < 24; i++) layout[i] = (uint64_t)((const char *)region[i] - base);
  layout[24] = w.total; layout[25] = sized.total; layout[26] = w.P; layout[27] = w.nscan_blocks; layout[28] = w.rec0_max; layout[29] = w.nchunks;
  const MsmReducePlan r = msm_reduce_plan(g, o);
  plan_flat_jobs(reduce, r.j1);
  plan_flat_jobs(reduce + PLAN_JOBS_WORDS, r.j2);
  plan_flat_jobs(reduce + 2 * PLAN_JOBS_WORDS, r.j2top);
  uint32_t *t = reduce + 3 * PLAN_JOBS_WORDS;
  t[0] = r.grid1; t[1] = r.top_w; t[2] = r.to.nv; t[7] = r.to.top;
  for (int k = 0; k < 4; k++) { t[3 + k] = r.to.off[k]; t[8 + k] = r.to.top_off[k]; }
  return pick_window_bits(o, n);
}
// The slices of a dense input of up to three segments of nseg[i] pairs whose arrays start at pts[i] / sc[i] (addresses, never
// dereferenced): returns K = msm_slice_count; for k < min(K, cap) out[10 k ..] = total n[3] pts[3] sc[3] of segs_slice(msm_slice(k)).
#define PLAN_SLICE_WORDS 10
static inline uint64_t plan_flat_slices(const int32_t *kv, int nkv, const uint32_t nseg[3], const uint64_t pts[3], const uint64_t sc[3], uint64_t cap, uint64_t *out) {
  const BpmiOptions o = plan_options(kv, nkv);
  Segs s = segs_init();
  for (int i = 0; i < 3; i++) { s.n[i] = nseg[i]; s.pts[i] = (const u32 *)(uintptr_t)pts[i]; s.sc[i] = (const u32 *)(uintptr_t)sc[i]; s.total += nseg[i]; }
  const uint64_t K = msm_slice_count(o, s), per = (s.total + K - 1) / K;
  for (uint64_t k = 0; k < K && k < cap; k++) {
    const MsmSlice sl = msm_slice(s.total, per, k);
    const Segs r = segs_slice(s, sl.lo, sl.cnt);
    uint64_t *q = out + PLAN_SLICE_WORDS * k;
    q[0] = r.total;
    for (int i = 0; i < 3; i++) { q[1 + i] = r.n[i]; q[4 + i] = (uint64_t)(uintptr_t)r.pts[i]; q[7 + i] = (uint64_t)(uintptr_t)r.sc[i]; }
  }
  return K;
}
