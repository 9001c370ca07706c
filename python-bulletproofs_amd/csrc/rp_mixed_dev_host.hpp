// rp_mixed_dev_host.hpp -- part of libbpmi (included by bpmi.hip; one translation unit).  HOST code.
// bpmi_rp_batch_verify_mixed_dev: range proofs of DIFFERENT sizes -- classes of one (n_gens, values_per_proof) each, over the prefixes of one
// generator list -- verified by ONE MSM.  Everything the call decides is rp_mixed_plan's (rp_mixed_plan_host.hpp); this file queues it on
// the ctx's two lanes with no host wait between classes: per class the stages of rp_batch_dev_host.hpp in the class's own regions
// (uploads, word-major proofs, point decoding on the second lane, column sums, shared scalars), per ROUND one launch of each of the two
// chain kernels over every class's row chunk (k_rp_roles_mixed, k_rp_elements_mixed), then k_rp_shared_merge and one msm_run.
// rp_mixed_enqueue also has a GROUP mode -- verdict bytes and per-group sums in place of the column sums, nothing merged -- for
// bpmi_rp_batch_group_values_mixed_dev (rp_group_mixed_dev_host.hpp).
#pragma once

// the unit table of the whole call: slot i = plan.unit[i]; host copy in `table` (RP_MIXED_UNIT_STRIDE bytes per slot)
static void rp_mixed_units(bpmi_ctx *ctx, const RpMixedPlan &mp, const std::vector<RpRun> &runs, const bpmi_rp_class *classes, std::vector<uint8_t> &table) {
  table.assign((size_t)RP_MIXED_UNIT_STRIDE * mp.unit.size(), 0);
  std::vector<rpd::Params> base;
  for (u32 c = 0; c < mp.n_classes; c++) base.push_back(rp_params(ctx, runs[c], classes[c].n_gens));
  for (const RpMixedRound &rd : mp.round) {
    u32 roles = 0, elems = 0;
    for (u32 i = rd.first_unit; i < rd.first_unit + rd.n_units; i++) {
      const RpMixedUnit &u = mp.unit[i];
      const RpPlan &pl = mp.cls[u.cls].pl;
      const u32 first = u.chunk * pl.rows, cnt = std::min(pl.rows, pl.P - first);
      rpd::MixedUnit mu;
      memset(&mu, 0, sizeof(mu));
      mu.q = base[u.cls];
      rp_params_rows(mu.q, runs[u.cls], first, cnt);
      mu.eg.el_log = pl.el_log; mu.eg.ranges = pl.ranges;
      mu.first_roles = roles; mu.first_elems = elems;
      roles += RP_ROLES * ((cnt + pl.lanes - 1) / pl.lanes);
      elems += 2 * pl.ranges * ((cnt + 63) / 64);
      memcpy(table.data() + (size_t)RP_MIXED_UNIT_STRIDE * i, &mu, sizeof(mu));
    }
  }
}
// blocks of the two launches of a round
static void rp_mixed_round_blocks(const RpMixedPlan &mp, const RpMixedRound &rd, u32 &roles, u32 &elems) {
  roles = elems = 0;
  for (u32 i = rd.first_unit; i < rd.first_unit + rd.n_units; i++) {
    const RpPlan &pl = mp.cls[mp.unit[i].cls].pl;
    const u32 first = mp.unit[i].chunk * pl.rows, cnt = std::min(pl.rows, pl.P - first);
    roles += RP_ROLES * ((cnt + pl.lanes - 1) / pl.lanes);
    elems += 2 * pl.ranges * ((cnt + 63) / 64);
  }
}

// everything up to the merged scalars, queued; `table` must live until the lanes have been waited for.
// gm: group mode (bpmi_rp_batch_group_values_mixed_dev, rp_group_mixed_dev_host.hpp; mp is then gm->mixed) -- the two buffers hold the
// groups' regions behind the mixed plan's, every class's cells are summed per group behind a per-proof verdict (rp_queue_group_rows in
// place of k_rp_colsum) and folded into the scalars of the groups' MSMs (k_rp_group_scalars), nothing is merged, and under
// rp_overlap = 0 the plan asks for the decoding in front of the rounds (RP_DECODE_FIRST).  groups: one RpGroups per class, filled here
// (d_E / d_vals / route / W stay unset: the call has one E and one tail); it must live as long as `table`.  nullptr: the batch as one.
static int rp_mixed_enqueue(bpmi_ctx *ctx, const RpMixedPlan &mp, const bpmi_rp_class *classes, const uint8_t *weights, const uint8_t *seed, void *d_points,
                            void *d_scalars, PointCheck &pc, const void *d_gens, std::vector<uint8_t> &table, u32 *&d_merged, unsigned long long *&d_bad,
                            const RpgmPlan *gm = nullptr, std::vector<RpGroups> *groups = nullptr) {
  int rc = rp_ensure_sizes(ctx, mp.stage_bytes, gm ? gm->pin_bytes : mp.pin_bytes, gm ? gm->need : mp.need);
  if (rc) return rc;
  char *din = (char *)ctx->stage_in, *buf = (char *)ctx->rp_buf;
  d_merged = (u32 *)(buf + mp.merged.off);
  d_bad = (unsigned long long *)(buf + mp.bad.off);
  uint8_t *d_units = (uint8_t *)(buf + mp.units.off);
  // the commitments: staged back to back for ONE on-curve check (the index of a refused one counts commitments class-major), then copied
  // to the head of each class's block
  char *d_vstage = din + mp.o_vstage;
  for (u32 c = 0; c < mp.n_classes; c++) HIPCHK(ctx, h2d(ctx, d_vstage + 64 * mp.cls[c].v_off, classes[c].v_points, 64 * mp.cls[c].nv, ctx->stream));
  pc.queue(d_vstage, mp.n_v, "v_points");
  if (ctx->opt_validate >= 2) pc.queue(d_gens, 3 + 2 * (uint64_t)mp.N, "d_gens");
  rc = pc.fetch();
  if (rc) return rc;
  for (u32 c = 0; c < mp.n_classes; c++)
    HIPCHK(ctx, hipMemcpyAsync((char *)d_points + 64 * mp.cls[c].pair_off, d_vstage + 64 * mp.cls[c].v_off, 64 * mp.cls[c].nv, hipMemcpyDeviceToDevice, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(d_bad, 0xFF, 8, ctx->stream));
  if (gm) {
    groups->assign(mp.n_classes, RpGroups{});
    for (u32 c = 0; c < mp.n_classes; c++) {
      const RpgmClass &q = gm->cls[c];
      RpGroups &G = (*groups)[c];
      G.group = q.group; G.ngroups = q.ngroups;
      G.d_gsum = (u32 *)(buf + q.gsum.off); G.d_gfin = (u32 *)(buf + q.gfin.off); G.d_verdict = (uint8_t *)(buf + q.o_verdict); G.d_ptflag = (uint8_t *)(buf + q.ptflag.off);
    }
  }
  std::vector<RpRun> runs;
  runs.reserve(mp.n_classes);
  for (u32 c = 0; c < mp.n_classes; c++) {
    const RpMixedClass &m = mp.cls[c];
    const bpmi_rp_class &k = classes[c];
    char *sc = (char *)d_scalars + 32 * m.pair_off;
    runs.push_back(RpRun{m.pl, k.blobs, weights ? weights + 128 * m.first : nullptr, seed, k.blob_off, sc, sc + 32 * m.nv, (char *)d_points + 64 * (m.pair_off + m.nv),
                         gm ? &(*groups)[c] : nullptr, din + m.in_base, buf + m.buf_base, d_bad, m.first});
  }
  rp_mixed_units(ctx, mp, runs, classes, table);
  if (!table.empty()) HIPCHK(ctx, h2d(ctx, d_units, table.data(), table.size(), ctx->stream));
  // per class: uploads (the second lane decodes the points of a slice behind it) and the word-major proofs
  for (u32 c = 0; c < mp.n_classes; c++) {
    rc = rp_queue_uploads(ctx, runs[c]);
    if (rc) return rc;
    rc = rp_queue_words(ctx, runs[c]);
    if (rc) return rc;
  }
  // group mode under rp_overlap = 0: the verdicts of the first round read every point flag
  for (u32 c = 0; c < mp.n_classes; c++)
    if (mp.cls[c].pl.decode == RP_DECODE_FIRST) rp_queue_decode(ctx, runs[c], ctx->stream, 0, mp.cls[c].pl.P);
  // The second lane's last record is behind every class's decoding: one wait in front of the first group rows (rp_queue_group_rows waits
  // again at every class's first chunk -- for the same, by then reached, record)
  if (gm) HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
  // per round: the two chain kernels over every class's row chunk in one launch each, then the classes' column sums
  for (const RpMixedRound &rd : mp.round) {
    u32 roles, elems;
    rp_mixed_round_blocks(mp, rd, roles, elems);
    const uint8_t *tab = d_units + (size_t)RP_MIXED_UNIT_STRIDE * rd.first_unit;
    {
      StageTimer t(ctx, ST_RPPREP);
      hipLaunchKernelGGL(rpd::k_rp_roles_mixed, dim3(roles), dim3(64), rd.lds_bytes, ctx->stream, tab, rd.n_units);
    }
    {
      StageTimer t(ctx, ST_RPELEM);
      hipLaunchKernelGGL(rpd::k_rp_elements_mixed, dim3(elems), dim3(64), 0, ctx->stream, tab, rd.n_units);
      for (u32 i = rd.first_unit; i < rd.first_unit + rd.n_units; i++) {
        if (gm) break;
        const RpMixedUnit &u = mp.unit[i];
        const RpPlan &pl = mp.cls[u.cls].pl;
        const u32 cnt = std::min(pl.rows, pl.P - u.chunk * pl.rows);
        hipLaunchKernelGGL(rpd::k_rp_colsum, dim3(pl.ncols), dim3(256), 0, ctx->stream, (const u32 *)runs[u.cls].d_contrib(), cnt, runs[u.cls].d_shared());
      }
    }
    if (!gm) continue;
    // group mode: per unit the verdict bytes and the per-group column sums of that class's chunk (its own timed section)
    for (u32 i = rd.first_unit; i < rd.first_unit + rd.n_units; i++) {
      const RpMixedUnit &u = mp.unit[i];
      const RpPlan &pl = mp.cls[u.cls].pl;
      const u32 first = u.chunk * pl.rows;
      rc = rp_queue_group_rows(ctx, runs[u.cls], first, std::min(pl.rows, pl.P - first));
      if (rc) return rc;
    }
  }
  for (u32 c = 0; c < mp.n_classes; c++)
    if (mp.cls[c].pl.decode == RP_DECODE_LAST) rp_queue_decode(ctx, runs[c], ctx->stream, 0, mp.cls[c].pl.P);      // option rp_overlap = 0: behind the preparation
  if (gm) {
    // every group's constants folded into its own row of scalars, class by class
    StageTimer t(ctx, ST_RPELEM);
    for (u32 c = 0; c < mp.n_classes; c++) {
      const u32 n = classes[c].n_gens;
      const RpGroups &G = (*groups)[c];
      hipLaunchKernelGGL(rpd::k_rp_group_scalars, dim3((u32)(((uint64_t)G.ngroups * (3 + 2 * n) + 255) / 256)), dim3(256), 0, ctx->stream, (const u32 *)G.d_gsum, n, G.ngroups,
                         G.d_gfin);
    }
  } else {
    // every class's constants folded into its own prefix, then the prefixes summed into the scalars of g, h, u, gs[0..N), hs[0..N)
    StageTimer t(ctx, ST_RPELEM);
    rpd::MergeArgs ma;
    memset(&ma, 0, sizeof(ma));
    ma.n_classes = mp.n_classes; ma.N = mp.N;
    for (u32 c = 0; c < mp.n_classes; c++) {
      const u32 n = classes[c].n_gens;
      u32 *fin = (u32 *)(runs[c].buf + mp.cls[c].pl.o_fin);
      hipLaunchKernelGGL(rpd::k_rp_shared_scalars, dim3((3 + 2 * n + 255) / 256), dim3(256), 0, ctx->stream, (const u32 *)runs[c].d_shared(), n, fin);
      ma.fin[c] = fin; ma.n[c] = n;
    }
    hipLaunchKernelGGL(rpd::k_rp_shared_merge, dim3((3 + 2 * mp.N + 255) / 256), dim3(256), 0, ctx->stream, ma, d_merged);
  }
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));      // the second lane's last record: behind every class's decoding
  return BPMI_OK;
}

extern "C" {

int bpmi_rp_batch_verify_mixed_dev(bpmi_ctx *ctx, uint32_t n_classes, const bpmi_rp_class *classes, uint32_t n_gens_max, const uint8_t *weights, const uint8_t *seed,
                                   const void *d_gens, void *d_points, void *d_scalars, uint8_t out[64], int64_t *first_bad) {
  if (!ctx) return BPMI_E_ARG;
  const RpMixedPlan mp = rp_mixed_plan(*ctx, n_classes, classes, n_gens_max, weights != nullptr, seed != nullptr, d_gens && d_points && d_scalars && out && first_bad);
  if (mp.err) return fail(ctx, mp.err, mp.msg);
  *first_bad = -1;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  PointCheck pc(ctx, "bpmi_rp_batch_verify_mixed_dev", ctx->stream, ctx->opt_validate >= 1);
  std::vector<uint8_t> table;
  u32 *d_merged = nullptr;
  unsigned long long *d_bad = nullptr;
  int rc = rp_mixed_enqueue(ctx, mp, classes, weights, seed, d_points, d_scalars, pc, d_gens, table, d_merged, d_bad);
  if (!rc && hipMemcpyAsync(ctx->pin, d_bad, 8, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = fail(ctx, BPMI_E_HIP, "copy of the verdict failed");
  // an error in the middle must not return while the second lane is still writing into the caller's point array
  if (rc) { memset(out, 0xFF, 64); return rp_wait_lanes(ctx, rc); }
  Segs s = segs_init();
  s.pts[0] = (const u32 *)d_gens; s.sc[0] = d_merged; s.n[0] = 3 + 2 * mp.N;
  s.pts[1] = (const u32 *)d_points; s.sc[1] = (const u32 *)d_scalars; s.n[1] = (u32)mp.n_pairs;
  s.total = s.n[0] + s.n[1];
  rc = msm_run(ctx, s, out);                      // waits for the MSM (ctx stream: behind everything queued above)
  rc = rp_wait_lanes(ctx, rc);
  if (!rc) rc = pc.verdict();
  if (rc) { memset(out, 0xFF, 64); return rc; }                    // (never the identity)
  *first_bad = rp_first_bad_at(ctx->pin);
  if (*first_bad >= 0) {
    // a well-formed proof of another wire format at the flagged index is a sender's mix-up, not a verdict: the argument error names the class
    u32 c = 0;
    while (c + 1 < mp.n_classes && mp.cls[c + 1].first <= (uint64_t)*first_bad) c++;
    rc = rp_mixed_formats(ctx, classes[c].blobs, classes[c].blobs_len, classes[c].blob_off, *first_bad - (int64_t)mp.cls[c].first, (int)c);
  }
  if (!rc && ctx->opt_rp_only_role >= 0) *first_bad = 0;             // a profiling run that checked part of every proof never reads as "all valid"
  if (rc) memset(out, 0xFF, 64);
  return rc;
}

}  // extern "C"
