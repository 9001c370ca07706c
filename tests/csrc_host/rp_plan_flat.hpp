// The batch verifier's planner (csrc/rp_batch_plan_host.hpp) behind flat arrays, for tests only: host_shim.cpp exports these to
// tests/test_rp_plan_cpu.py, host_native_fuzz.cpp runs them under the sanitizers on heap blocks of exactly these sizes.
#pragma once
#include <stdint.h>
#include <stddef.h>

#include "rp_batch_plan_host.hpp"
#include "options_flat.hpp"        // kv: (row of the option's name, value) pairs

#define RP_PLAN_NREGIONS 11      // contrib ctx shared T lens | gsum gfin verdict ptflag E vals
// err | P m k per ncols nslots fmt0 v2 rp_prio maxlen W | o_off o_w o_st stage_bytes | 11 x (off, bytes) | o_bad o_fin need | cell_row out_row rows
// lanes el_log ranges lds_bytes pin_bytes | nsl 4 x (g0 g1 b0 b1) decode | group ngroups msm_windows route
#define RP_PLAN_WORDS (1 + 11 + 4 + 2 * RP_PLAN_NREGIONS + 3 + 8 + 1 + 4 * RP_UPLOAD_SLICES + 1 + 4)

// the plan of one call as RP_PLAN_WORDS words; returns the error code (then only out[0] is set and msg holds the text, cut to msg_cap - 1 characters)
static inline int rp_plan_flat(const int32_t *kv, int nkv, uint32_t n_gens, uint32_t m, uint64_t n_proofs, const uint8_t *blobs, uint64_t blobs_len,
                               const uint64_t *blob_off, int has_weights, uint64_t group, uint64_t *out, char *msg, size_t msg_cap) {
  const BpmiOptions o = plan_options(kv, nkv);
  const RpPlan p = rp_prepare_plan(o, n_gens, m, n_proofs, blobs, blobs_len, blob_off, has_weights != 0, group);
  for (int i = 0; i < RP_PLAN_WORDS; i++) out[i] = 0;
  if (msg_cap) msg[0] = 0;
  out[0] = (uint64_t)(int64_t)p.err;
  if (p.err) {
    for (size_t i = 0; i + 1 < msg_cap && p.msg[i]; i++) { msg[i] = p.msg[i]; msg[i + 1] = 0; }
    return p.err;
  }
  uint64_t *w = out + 1;
  const uint64_t shape[] = {p.P, p.m, p.k, p.per, p.ncols, p.nslots, p.fmt0, p.v2, p.rp_prio, p.maxlen, p.W, p.o_off, p.o_w, p.o_st, p.stage_bytes};
  for (uint64_t v : shape) *w++ = v;
  const RpRegion *const region[RP_PLAN_NREGIONS] = {&p.contrib, &p.ctx, &p.shared, &p.T, &p.lens, &p.gsum, &p.gfin, &p.verdict, &p.ptflag, &p.E, &p.vals};
  for (const RpRegion *r : region) { *w++ = r->off; *w++ = r->bytes; }
  const uint64_t rest[] = {p.o_bad, p.o_fin, p.need, p.cell_row, p.out_row, p.rows, p.lanes, p.el_log, p.ranges, p.lds_bytes, p.pin_bytes, p.nsl};
  for (uint64_t v : rest) *w++ = v;
  for (uint32_t c = 0; c < RP_UPLOAD_SLICES; c++) {
    const bool live = c < p.nsl;
    *w++ = live ? p.sl[c].g0 : 0; *w++ = live ? p.sl[c].g1 : 0; *w++ = live ? p.sl[c].b0 : 0; *w++ = live ? p.sl[c].b1 : 0;
  }
  *w++ = p.decode; *w++ = p.group; *w++ = p.ngroups; *w++ = p.msm_windows; *w++ = p.route;
  return 0;
}
// t0 nt lpg gpb nblk of k_rp_group_colsum over the proofs [base, base + cnt)
static inline void rp_group_chunk_flat(uint32_t group, uint32_t base, uint32_t cnt, uint32_t out[5]) {
  const RpGroupChunk c = rp_group_chunk(group, base, cnt);
  out[0] = c.t0; out[1] = c.nt; out[2] = c.lpg; out[3] = c.gpb; out[4] = c.nblk;
}
