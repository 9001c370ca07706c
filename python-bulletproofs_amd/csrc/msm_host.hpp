// msm_host.hpp -- part of libbpmi (included by bpmi.hip; one translation unit).
// Host orchestration of one MSM: the stages that queue what msm_plan_host.hpp planned, enqueue / finish on a lane, pairs, slices.
#pragma once

// ---- replay of an MSM's launch sequence as a HIP graph (option "graphs") -------------------------------------------------------
// An MSM is a dozen to 17 launches; the host pays ~9 us for each, and for every MSM below ~2^18 pairs the GPU finishes the sort's
// short kernels faster than the host can queue the next one (round 4, profiles/r04_C3_kernel_timeline_mid_round.txt: 160 us between
// the first kernels of the two lanes of one inner-product round).  Callers repeat the SAME sequence -- same input arrays, same
// size, same workspace: the rounds of an inner-product argument, a verifier's batches, a benchmark loop -- so the sequence is
// captured once per (lane, slot, inputs, geometry, options) and launched as one graph afterwards.  Only launches are captured: the
// slot's completion event is recorded behind the graph, allocation happens before the capture, a reallocation of the workspace or
// of the slot's pinned buffer drops the cache.  Not used with stage timers, debug syncs or the chained asynchronous pipeline.
struct MsmGraphKey {
  int lane, slot, glv, small, opt_quad, opt_tail, opt_epl, opt_hist_threads, opt_hist_blocks;
  u32 w0, wcount;
  Segs segs;
  MsmGeom g;
  const void *ws, *pin;
};
struct MsmGraphEntry {
  MsmGraphKey key;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  u32 W = 0, nv = 0, c = 0; int tail = 2; TailOffs to;
};
struct MsmGraphCache { std::vector<MsmGraphEntry> entries; };
static void msm_graphs_clear(bpmi_ctx *ctx) {
  if (!ctx->graphs || ctx->graphs->entries.empty()) return;
  // a replayed graph may still be running on any lane: nothing is destroyed under it
  (void)sync_lanes(ctx);
  for (auto &e : ctx->graphs->entries) { if (e.exec) (void)hipGraphExecDestroy(e.exec); if (e.graph) (void)hipGraphDestroy(e.graph); }
  ctx->graphs->entries.clear();
}
// what a captured sequence depends on (compared byte by byte: zeroed first)
static void msm_graph_key(MsmGraphKey &key, const bpmi_ctx *ctx, const MsmPlan &pl, int lane, int slot, const Segs &segs_in, u32 w0, u32 wcount) {
  memset(&key, 0, sizeof(key));
  key.lane = lane; key.slot = slot; key.glv = pl.glv; key.small = pl.small ? 1 : (pl.mid ? 2 : 0); key.opt_quad = ctx->opt_quad; key.opt_tail = ctx->opt_tail; key.opt_epl = ctx->opt_epl;
  key.opt_hist_threads = ctx->opt_hist_threads; key.opt_hist_blocks = ctx->opt_hist_blocks; key.w0 = w0; key.wcount = wcount;
  memcpy(&key.segs, &segs_in, sizeof(Segs)); memcpy(&key.g, &pl.g, sizeof(MsmGeom));
  key.ws = ctx->lane[lane].ws; key.pin = ctx->pend[slot].pin;
}
// One MSM's way into its pending slot: begin() replays the graph cached under `key` or opens a capture of the launches that follow,
// commit() closes and caches the capture and queues what stands behind the graph or behind the launches -- the completion event, the
// slot's bookkeeping.  Without begin() it is commit() alone; a capture that an error path leaves open ends with the object.
struct MsmCapture {
  bpmi_ctx *ctx; hipStream_t st; bpmi_ctx::PendingMsm &pd;
  MsmGraphKey key; bool open = false;
  MsmCapture(bpmi_ctx *c, hipStream_t s, bpmi_ctx::PendingMsm &p) : ctx(c), st(s), pd(p) {}
  ~MsmCapture() { if (open) { hipGraph_t g = nullptr; (void)hipStreamEndCapture(st, &g); if (g) (void)hipGraphDestroy(g); (void)hipGetLastError(); } }
  int begin(bool &replayed) {
    replayed = false;
    if (ctx->graphs)
      for (auto &e : ctx->graphs->entries)
        if (!memcmp(&e.key, &key, sizeof(key))) {
          HIPCHK(ctx, hipGraphLaunch(e.exec, st));
          replayed = true;
          return commit(e.W, e.nv, e.c, e.tail, e.to);
        }
    HIPCHK(ctx, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    open = true;
    return BPMI_OK;
  }
  int commit(u32 W_, u32 nv_, u32 c_, int tail_, const TailOffs &to_) {
    if (open) {
      MsmGraphEntry e;
      memcpy(&e.key, &key, sizeof(key)); e.W = W_; e.nv = nv_; e.c = c_; e.tail = tail_; e.to = to_;
      open = false;
      HIPCHK(ctx, hipStreamEndCapture(st, &e.graph));
      hipError_t ie = hipGraphInstantiate(&e.exec, e.graph, nullptr, nullptr, 0);
      if (ie != hipSuccess) { (void)hipGraphDestroy(e.graph); return fail(ctx, BPMI_E_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ie)); }
      if (!ctx->graphs) ctx->graphs = new MsmGraphCache();
      if (ctx->graphs->entries.size() >= 48) msm_graphs_clear(ctx);
      ctx->graphs->entries.push_back(e);
      HIPCHK(ctx, hipGraphLaunch(e.exec, st));
    }
    HIPCHK(ctx, hipEventRecord(pd.done, st));
    pd.active = true; pd.W = W_; pd.nv = nv_; pd.c = c_; pd.tail = tail_; pd.to = to_;
    HIPCHK(ctx, hipGetLastError());
    return BPMI_OK;
  }
};

// ---- the stages of msm_enqueue: each queues its launches on `st` and returns; E_dst is where the MSM's last device-side values go -------
// the one-block-per-window kernel, g.nv parts per window (every part of a window at bit offset 0: the host tail adds them)
static int msm_queue_mid(bpmi_ctx *ctx, hipStream_t st, const bpmi_ctx::PendingMsm &pd, const Segs &segs, const MsmGeom &g, const MsmWs &w, u32 *E_dst) {
  {
    StageTimer t(ctx, ST_ACCUM, st);
    MidPair mp;
    memset(&mp, 0, sizeof(mp));
    mp.segs[0] = segs; mp.g[0] = g; mp.E[0] = E_dst;
    hipLaunchKernelGGL(k_msm_mid, dim3(g.W, 1, g.nv), dim3(MID_THREADS), 0, st, mp);
  }
  debug_sync(ctx, "k_msm_mid", st);
  if (!ctx->opt_direct) HIPCHK(ctx, hipMemcpyAsync(pd.pin, w.E, 4ull * XYZZ_WORDS * g.W * g.nv, hipMemcpyDeviceToHost, st));
  return BPMI_OK;
}
// the one-launch kernel (and its combine from 257 pairs)
static int msm_queue_small(bpmi_ctx *ctx, hipStream_t st, const bpmi_ctx::PendingMsm &pd, const Segs &segs, const MsmGeom &g, const MsmWs &w, u32 *E_dst) {
  const uint64_t n = segs.total;
  {
    StageTimer t(ctx, ST_ACCUM, st);
    const u32 threads = (u32)std::min<uint64_t>(256, (n + 63) / 64 * 64);
    const u32 S = (u32)std::min<uint64_t>(64, (n + 255) / 256);
    hipLaunchKernelGGL(k_msm_small, dim3(g.W, S), dim3(threads), 0, st, segs, g, S > 1 ? w.buckets : E_dst);
    if (S > 1) hipLaunchKernelGGL(k_small_combine, dim3(g.W), dim3(64), 0, st, w.buckets, S, E_dst);
  }
  debug_sync(ctx, "k_msm_small", st);
  if (!ctx->opt_direct) HIPCHK(ctx, hipMemcpyAsync(pd.pin, w.E, 4ull * XYZZ_WORDS * g.W, hipMemcpyDeviceToHost, st));
  return BPMI_OK;
}
// sort path 2: the two-level LDS partition sort.  `rec` (the fixed-base MSM, msm_fixed_kernels.hpp): the recoding is k_fixed_recode with
// rec's arguments -- the real scalars into the codes of the virtual geometry g -- and the scan of the counts always its own launch
static void msm_queue_sort_lds(bpmi_ctx *ctx, hipStream_t st, const Segs &segs, const MsmGeom &g, const MsmWs &w, const MsmRecode *rec = nullptr) {
  {
    StageTimer t(ctx, ST_DIGITS, st);
    // few blocks (every block ends with a flush of its 2048-bin LDS histogram), many threads: a thread recodes its scalars one after
    // the other and every one starts with a load, so the waves per SIMD are what hides that latency (512 blocks of 256 threads: 38 us at
    // n = 2^20, 256 blocks of 1024: 28.5; options "hist_threads" / "hist_blocks", tools/hist_sweep.py)
    const u32 ht = ctx->opt_hist_threads > 0 ? (u32)ctx->opt_hist_threads : 1024u;
    const u32 hb = (u32)std::min<uint64_t>(((uint64_t)(rec ? rec->real.n : g.n) + ht - 1) / ht, ctx->opt_hist_blocks > 0 ? (u32)ctx->opt_hist_blocks : 256u);
    // (round 5: the last block to flush runs the scan of the partition counts itself; ticket word behind the any_heavy flag and the
    // segmented scan's ticket, zeroed by the memset of msm_queue_sort)
    CoarseScanOut so = {nullptr, nullptr, nullptr, nullptr};
    if (ctx->opt_histscan && !rec) { so.coarse_off = w.coarse_off; so.coarse_cursor = w.coarse_cursor; so.offG = w.off + g.G; so.ticket = w.coarse_hist + PART_MAX + 2; }
    if (rec) hipLaunchKernelGGL(k_fixed_recode, dim3(hb), dim3(ht), 0, st, rec->sc, rec->real, rec->n_scalars, rec->R, rec->Wv, g, w.P, w.coarse_hist, w.dig16, w.negs);
    else hipLaunchKernelGGL(k_coarse_hist, dim3(hb), dim3(ht), 0, st, segs, g, w.P, w.coarse_hist, w.dig16, w.negs, so);
  }
  debug_sync(ctx, "ST_DIGITS", st);
  if (!ctx->opt_histscan || rec) {
    StageTimer t(ctx, ST_SCAN, st);
    // exclusive scan of <= 2048 partition counts; total -> coarse_off[P] and off[G]
    hipLaunchKernelGGL(k_coarse_scan, dim3(1), dim3(1024), 0, st, w.coarse_hist, w.P, w.coarse_off, w.coarse_cursor, w.off + g.G);
  }
  debug_sync(ctx, "ST_SCAN", st);
  {
    StageTimer t(ctx, ST_SCATTER, st);
    const u32 TS = g.n >= (1u << 19) ? PT_MAX : 4096u;          // scalars per level-A tile: long runs once there are enough tiles
    hipLaunchKernelGGL(k_partition, dim3((g.n + TS - 1) / TS, g.W), dim3(PT_THREADS), 0, st, g, w.P, TS, w.coarse_off, w.coarse_cursor, w.dig16, w.negs, w.dig,
                       w.hist, w.coarse_hist + PART_MAX);
    // level B: one block per partition; writes off[0..G), the chunk keys and the sorted entries
    // (heavy partitions: counted and scattered by the tile kernels, which return at once when there are none)
    const u32 nft = (u32)(((size_t)g.n * g.W + FINE_TILE - 1) / FINE_TILE);
    const u32 *any_heavy = w.coarse_hist + PART_MAX;
    if (!g.inblock) hipLaunchKernelGGL(k_fine_hist_heavy, dim3(nft), dim3(256), 0, st, g, w.P, w.coarse_off, w.dig, w.coarse_off + w.P, any_heavy, w.hist);
    hipLaunchKernelGGL(k_fine_sort_part, dim3(w.P), dim3(FINE_THREADS), 0, st, g, w.coarse_off, w.dig, w.hist, w.off, w.cursor, w.chunk_key, w.sidx, w.buckets);
    if (!g.inblock) hipLaunchKernelGGL(k_fine_scatter_heavy, dim3(nft), dim3(256), 0, st, g, w.P, w.coarse_off, w.dig, w.coarse_off + w.P, any_heavy, w.cursor, w.sidx);
    if (g.runs) {
      // the run table of k_accum_runs: the non-empty buckets by run length, in two regions the sort no longer needs; raises the flag that
      // hands the MSM to k_accum_l0 when a run is longer than the cap
      const u32 cap = msm_runs_cap(*ctx, g), nblk = msm_runs_blocks(g);
      const RunTable rt = {w.run_order, w.run_counts, w.run_flags, msm_runs_bins(cap), cap};
      hipLaunchKernelGGL(k_runs_hist, dim3(nblk), dim3(256), 0, st, g, w.off, rt);
      hipLaunchKernelGGL(k_runs_scatter, dim3(nblk), dim3(256), 0, st, g, w.off, rt);
    }
  }
  debug_sync(ctx, "ST_SCATTER", st);
}
// sort path 1: counting sort with global atomics
static void msm_queue_sort_atomic(bpmi_ctx *ctx, hipStream_t st, const Segs &segs, const MsmGeom &g, const MsmWs &w) {
  const u32 nblk_n = (u32)std::min<uint64_t>(((uint64_t)g.n + 255) / 256, 8192);
  {
    StageTimer t(ctx, ST_DIGITS, st);
    hipLaunchKernelGGL(k_digits_hist, dim3(nblk_n), dim3(256), 0, st, segs, g, w.dig, w.hist);
  }
  debug_sync(ctx, "ST_DIGITS", st);
  {
    StageTimer t(ctx, ST_SCAN, st);
    hipLaunchKernelGGL(k_scan_partials, dim3(w.nscan_blocks), dim3(256), 0, st, w.hist, g.G, w.bsum);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(1024), 0, st, w.bsum, w.nscan_blocks, w.off, g.G);
    hipLaunchKernelGGL(k_scan_final, dim3(w.nscan_blocks), dim3(256), 0, st, w.hist, g.G, w.bsum, w.off, w.cursor);
  }
  debug_sync(ctx, "ST_SCAN", st);
  {
    StageTimer t(ctx, ST_SCATTER, st);
    hipLaunchKernelGGL(k_scatter, dim3(nblk_n), dim3(256), 0, st, g, w.dig, w.cursor, w.sidx);
    hipLaunchKernelGGL(k_chunk_keys, dim3((g.G + 255) / 256), dim3(256), 0, st, g, w.off, w.chunk_key);
  }
  debug_sync(ctx, "ST_SCATTER", st);
}
// recoding .. sorted entries, the buckets cleared: everything of the bucket pipeline before the accumulation
static int msm_queue_sort(bpmi_ctx *ctx, hipStream_t st, const Segs &segs, const MsmGeom &g, const MsmWs &w, const MsmRecode *rec = nullptr) {
  {
    StageTimer t(ctx, ST_MISC, st);
    if (w.P) HIPCHK(ctx, hipMemsetAsync(w.coarse_hist, 0, 4ull * COARSE_HIST_WORDS, st));      // (a multiple of 256 bytes: ONE fill kernel, not an aligned part and a tail)
    else {
      HIPCHK(ctx, hipMemsetAsync(w.hist, 0, 4ull * g.G, st));
      HIPCHK(ctx, hipMemsetAsync(w.buckets, 0, 4ull * XYZZ_WORDS * g.G, st));      // path 2: k_fine_sort_part clears the empty buckets
    }
  }
  debug_sync(ctx, "ST_MISC", st);
  if (w.P) msm_queue_sort_lds(ctx, st, segs, g, w, rec);
  else msm_queue_sort_atomic(ctx, st, segs, g, w);
  return BPMI_OK;
}
// k_accum_l0 and, on the chained pipeline, the events that order it behind the accumulation queued before it
static int msm_queue_accumulate(bpmi_ctx *ctx, const MsmMode &mode, int lane, hipStream_t st, const Segs &segs, const MsmGeom &g, const MsmWs &w, bool glv) {
  // Round 6 experiment (option "accum_stream"): on the chained pipeline every accumulation runs on ONE stream of its own, created with the
  // LOWEST queue priority, between two events of its lane -- the accumulations are in order by construction, and the lanes' sort and
  // reduction kernels sit on queues the dispatcher prefers whenever a wave slot frees up (with "chunk" below the one-round length the
  // accumulation's slots turn over while it runs).  profiles/r06_accum_stream_and_chunk_ab.txt
  const bool own_acc = mode.chained && ctx->opt_accum_stream && ctx->stream_acc;
  hipStream_t st_acc = own_acc ? ctx->stream_acc : st;
  Lane &l = ctx->lane[lane];
  if (own_acc) {
    HIPCHK(ctx, hipEventRecord(l.ev_sorted, st));
    HIPCHK(ctx, hipStreamWaitEvent(st_acc, l.ev_sorted, 0));
  } else if (mode.chained && !mode.free_run && ctx->accum_chain_lane >= 0 && ctx->accum_chain_lane != lane)
    HIPCHK(ctx, hipStreamWaitEvent(st, ctx->lane[ctx->accum_chain_lane].ev_accum, 0));
  {
    StageTimer t(ctx, ST_ACCUM, st_acc);
    auto kern = glv ? (g.fuse ? k_accum_l0<true, true> : k_accum_l0<true, false>) : (g.fuse ? k_accum_l0<false, true> : k_accum_l0<false, false>);
    // the accumulation by runs first (at most G runs; returns at once when the table kernels found a run over the cap), the chunked one behind it
    // (returns at once otherwise): the flag on the device chooses, nothing waits for the host
    const u32 *long_run = g.runs ? w.run_flags + RUN_FLAG_WORD : nullptr;
    if (g.runs) {
      auto runs = (!glv && segs_one_dense(segs)) ? k_accum_runs<true> : k_accum_runs<false>;      // one dense array: the point of an entry without the segment walk
      hipLaunchKernelGGL(runs, dim3((g.G + 255) / 256), dim3(256), 0, st_acc, segs, g, w.off, w.sidx, w.run_order, w.run_flags, w.buckets);
    }
    hipLaunchKernelGGL(kern, dim3((w.nchunks + 255) / 256), dim3(256), 0, st_acc, segs, g, w.off, w.chunk_key, w.sidx, w.buckets, w.rec_key[0], w.rec_pt[0], long_run);
  }
  if (own_acc) {
    HIPCHK(ctx, hipEventRecord(l.ev_accum, st_acc));
    HIPCHK(ctx, hipStreamWaitEvent(st, l.ev_accum, 0));
  } else if (mode.chained) { HIPCHK(ctx, hipEventRecord(l.ev_accum, st)); ctx->accum_chain_lane = lane; }
  debug_sync(ctx, "ST_ACCUM", st);
  return BPMI_OK;
}
// the partial records folded into their buckets: 256 -> 2 per block, level after level, until one block is left
static void msm_queue_segscan(bpmi_ctx *ctx, hipStream_t st, const MsmGeom &g, const MsmWs &w) {
  {
    StageTimer t(ctx, ST_SEGSCAN, st);
    u32 R = w.rec0_max;
    int level = 1, src = 0;
    // the ticket word of the last-block-done fusion (zeroed by the sort's memset; sort path 2 only, first level only)
    u32 *ticket = (w.P && ctx->opt_segfuse) ? w.coarse_hist + PART_MAX + 1 : nullptr;
    const u32 *long_run = g.runs ? w.run_flags + RUN_FLAG_WORD : nullptr;       // (every level returns at once when k_accum_runs took the MSM)
    for (;;) {
      const u32 nb = (R + 255) / 256;
      if (nb > 128u || nb <= 1u) ticket = nullptr;      // (the kernel's own block count is at most this one: fewer entries than the bound)
      hipLaunchKernelGGL(k_segscan, dim3(nb), dim3(256), 0, st, g, w.off, level, w.rec_key[src], w.rec_pt[src],
                         w.rec_key[src ^ 1], w.rec_pt[src ^ 1], w.buckets, ticket, long_run);
      if (g_debug_sync) { fprintf(stderr, "[bpmi] segscan level %d nb %u R %u\n", level, nb, R); debug_sync(ctx, "segscan level", st); }
      if (nb <= 1 || ticket) break;
      R = 2 * nb;
      // ping-pong: level 1 reads buffer 0 (large) and writes buffer 1; later levels are
      // small enough for either buffer (rec1_max >= every later level)
      src ^= 1;
      level++;
    }
  }
  debug_sync(ctx, "ST_SEGSCAN", st);
}
// sum_b b B[w][b] per window into E_red; returns the digits' bit offsets for the tail.  The jobs are msm_reduce_plan's: this only
// chooses and launches the finish variant.
static TailOffs msm_queue_reduce(bpmi_ctx *ctx, hipStream_t st, const MsmGeom &g, const MsmWs &w, u32 *E_red) {
  const MsmReducePlan r = msm_reduce_plan(g, *ctx);
  {
    StageTimer t(ctx, ST_BREDUCE, st);
    if (g.B <= 256u) {
      if (ctx->opt_quad) hipLaunchKernelGGL(k_window_weighted_small_quad, dim3(g.W), dim3(g.B < 16u ? 64u : 4u * g.B), 0, st, g, w.buckets, E_red);
      else hipLaunchKernelGGL(k_window_weighted_small, dim3(g.W), dim3(g.B < 64u ? 64u : g.B), 0, st, g, w.buckets, E_red);
    } else {
      hipLaunchKernelGGL(k_digit_sums, dim3(r.grid1), dim3(256), 0, st, w.buckets, w.D, r.j1);
      // (the tickets of the spread finish live behind the sort's partition counts: zeroed by this MSM's memset when the LDS sort runs)
      if (ctx->opt_quad && ctx->opt_final_spread == 1 && w.P)
        hipLaunchKernelGGL(k_digit_final_spread<0>, dim3(g.W * 64u), dim3(64), 0, st, w.D, w.F, w.coarse_hist + PART_MAX + 8, E_red, r.j2, r.j2top, r.top_w);
      else if (ctx->opt_quad && ctx->opt_final_spread >= 2) {
        if (ctx->opt_final_spread == 2) hipLaunchKernelGGL(k_digit_final_spread<1>, dim3(g.W * 64u), dim3(64), 0, st, w.D, w.F, nullptr, E_red, r.j2, r.j2top, r.top_w);
        else hipLaunchKernelGGL(k_digit_final_spread<1>, dim3(g.W * 16u), dim3(256), 0, st, w.D, w.F, nullptr, E_red, r.j2, r.j2top, r.top_w);
        hipLaunchKernelGGL(k_digit_final_spread<2>, dim3(g.W * 4u), dim3(64), 0, st, w.D, w.F, nullptr, E_red, r.j2, r.j2top, r.top_w);
      }
      else if (ctx->opt_quad) hipLaunchKernelGGL(k_digit_final_quad, dim3(g.W * 4u), dim3(1024), 0, st, w.D, E_red, r.j2, r.j2top, r.top_w);
      else hipLaunchKernelGGL(k_digit_final, dim3(g.W * 4u), dim3(256), 0, st, w.D, E_red, r.j2, r.j2top, r.top_w);
    }
  }
  debug_sync(ctx, "ST_BREDUCE", st);
  return r.to;
}
// tail 1: the device tail (k_tail) and its 64 bytes; tail 2: the window sums for the host tail
static int msm_queue_tail(bpmi_ctx *ctx, hipStream_t st, const bpmi_ctx::PendingMsm &pd, const MsmGeom &g, const MsmWs &w, int tail, const TailOffs &to) {
  StageTimer t(ctx, ST_TAIL, st);
  if (tail == 1) {
    hipLaunchKernelGGL(k_tail, dim3(1), dim3(64), 0, st, w.E, g.W, g.c, to, ctx->opt_direct ? (u32 *)pd.pin : w.out);
    if (!ctx->opt_direct) HIPCHK(ctx, hipMemcpyAsync(pd.pin, w.out, 64, hipMemcpyDeviceToHost, st));
  } else if (!ctx->opt_direct)
    HIPCHK(ctx, hipMemcpyAsync(pd.pin, w.E, 4ull * XYZZ_WORDS * g.W * g.nv, hipMemcpyDeviceToHost, st));
  return BPMI_OK;
}

// Enqueue every GPU stage of one MSM on `lane` (0 = the ctx stream, 1 / 2 = the other lanes: stream +
// workspace), including the device->pinned-host copy the tail needs, into pending slot `slot`
// (pinned buffer + completion event); returns without synchronising.
//   mode: what the caller's pipeline does around this MSM (MsmMode, msm_plan_host.hpp)
//   [w0, w0 + wcount): the windows this call handles (wcount = 0: all of them)
//   phase: 0 = everything; 1 = the sort stage only, nothing becomes pending; 2 = the rest of an MSM whose sort a phase-1 call with
//   the SAME arguments queued on this lane (the plan is a function of the arguments: it is simply computed again).  A synchronous
//   pair queues both sorts before either accumulation (msm_run_pair).  MSMs on the one-launch kernels or on GLV scalars have no
//   sort to queue ahead: phase 1 does nothing for them and phase 2 everything.
//   rec: the fixed-base MSM (msm_fixed_host.hpp) -- segs_in are the table's virtual pairs, the plan is rec's virtual geometry and the recoding
//   rec's kernel; whole MSMs in one phase, never replayed as a graph (the key of a captured sequence does not cover rec's arguments)
static int msm_enqueue(bpmi_ctx *ctx, const MsmMode &mode, int lane, int slot, const Segs &segs_in, u32 w0 = 0, u32 wcount = 0, int phase = 0,
                       const MsmRecode *rec = nullptr) {
  Segs segs = segs_in;
  const uint64_t n = segs.total;
  bpmi_ctx::PendingMsm &pd = ctx->pend[slot];
  if (pd.active) return fail(ctx, BPMI_E_STATE, "an MSM is still pending in this slot (bpmi_msm_finish it first)");
  if (n == 0) return BPMI_OK;
  if (n > BPMI_MAX_N) return fail(ctx, BPMI_E_ARG, "n exceeds BPMI_MAX_N");
  const MsmPlan pl = rec ? rec->plan : msm_pick_geometry(*ctx, mode, n, w0, wcount);
  MsmGeom g = pl.g;
  MsmWs w;
  msm_layout(g, w, nullptr, pl.glv);
  int rc = ensure_lane(ctx, lane);
  if (rc) return rc;
  rc = ensure_ws(ctx, w.total, lane);
  if (rc) return rc;
  msm_layout(g, w, (char *)ctx->lane[lane].ws, pl.glv);
  hipStream_t st = ctx->lane[lane].stream;
  // the slot's pinned buffer before anything is queued (a capture must not allocate)
  rc = ensure_pin_slot(ctx, slot, std::max<size_t>(4096, 4ull * XYZZ_WORDS * g.W * 4));
  if (rc) return rc;
  const bool sort_ahead = !pl.mid && !pl.small && !pl.glv;       // the phases exist for this MSM
  if (phase == 1) {
    if (!sort_ahead) return BPMI_OK;
    if ((rc = msm_queue_sort(ctx, st, segs, g, w))) return rc;
    HIPCHK(ctx, hipGetLastError());
    return BPMI_OK;
  }
  MsmCapture cap(ctx, st, pd);
  if (phase == 0 && ctx->opt_graph && !ctx->prof && !g_debug_sync && !mode.chained && !rec) {
    msm_graph_key(cap.key, ctx, pl, lane, slot, segs_in, w0, wcount);
    bool replayed;
    rc = cap.begin(replayed);
    if (rc || replayed) return rc;
  }
  // Round 4: the kernels that produce an MSM's last device-side values (the window sums, or the point of the device tail) write
  // them straight into the slot's page-locked host buffer -- it is mapped into the device's address space -- instead of into the
  // workspace with a copy behind: one kernel boundary less on a path where every boundary is ~8 us (option "direct_result" = 0: the copy)
  u32 *const E_dst = ctx->opt_direct ? (u32 *)pd.pin : w.E;
  if (pl.glv) {
    StageTimer t(ctx, ST_DIGITS, st);
    hipLaunchKernelGGL(k_glv_prepare, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, segs, (u32)n, w.glv_sub, w.glv_neg, w.glv_bx);
    segs.glv_sub = w.glv_sub; segs.glv_neg = w.glv_neg; segs.glv_bx = w.glv_bx;
  }
  TailOffs to;
  memset(&to, 0, sizeof(to));
  to.nv = 1;
  int tail = 2;
  if (pl.mid) {
    g.nv = to.nv = mid_parts(*ctx, n);
    if ((rc = msm_queue_mid(ctx, st, pd, segs, g, w, E_dst))) return rc;
  } else if (pl.small) {
    if ((rc = msm_queue_small(ctx, st, pd, segs, g, w, E_dst))) return rc;
  } else {
    ctx->lane[lane].run_planned = g.runs; ctx->lane[lane].run_flags = w.P ? w.run_flags : nullptr;
    if (!(phase == 2 && sort_ahead) && (rc = msm_queue_sort(ctx, st, segs, g, w, rec))) return rc;
    if ((rc = msm_queue_accumulate(ctx, mode, lane, st, segs, g, w, pl.glv))) return rc;
    msm_queue_segscan(ctx, st, g, w);
    tail = wcount ? 2 : (ctx->opt_tail ? ctx->opt_tail : 2);      // window groups are combined on the host
    to = msm_queue_reduce(ctx, st, g, w, tail == 1 ? w.E : E_dst);      // (the device tail reads the window sums where they are)
    if ((rc = msm_queue_tail(ctx, st, pd, g, w, tail, to))) return rc;
  }
  return cap.commit(g.W, g.nv, g.c, tail, to);
}
// error path of a caller that has MSMs of ITS OWN queued in pending slots (bit s of `mine` = slot s was enqueued by this call):
// wait for both lanes, release those slots and no others -- a slot that holds a caller's asynchronous MSM (bpmi_msm_dev_enqueue)
// keeps it, so a later bpmi_msm_finish still returns that MSM's result and never the identity of an emptied slot
static void msm_abandon_pending(bpmi_ctx *ctx, unsigned mine) {
  (void)sync_lanes(ctx);
  for (int s = 0; s < BPMI_LANES; s++) if ((mine >> s) & 1u) ctx->pend[s].active = false;
}
// Wait for the slot's MSM (its completion event: work enqueued behind it keeps running) and run the
// host part of the tail; out = the MSM result.
static int msm_finish(bpmi_ctx *ctx, int slot, uint8_t out[64]) {
  bpmi_ctx::PendingMsm &pd = ctx->pend[slot];
  if (!pd.active) { memset(out, 0, 64); return BPMI_OK; }      // n == 0
  pd.active = false;
  HIPCHK(ctx, wait_event(ctx, pd.done));
  const void *pin = pd.pin;
  if (pd.tail == 1) {
    memcpy(out, pin, 64);
  } else {
    bpmi_host::tail_combine(out, (const u32 *)pin, pd.W, pd.c, pd.to);     // host_tail.hpp
  }
  return BPMI_OK;
}
// One MSM as two window groups, one per lane (option "split").  Measured on MI355X
// (tools/try_split.py): the lanes' kernels barely overlap -- every stage is bound by the
// same ALUs or by LDS atomics in blocks that cannot co-reside with the accumulation's --
// so the gain is the kernels' tails only (+5 % at n = 2^20, -8 % at 2^19); off by default.
static int msm_run_split(bpmi_ctx *ctx, const Segs &segs, uint8_t out[64]) {
  const u32 c = pick_window_bits(*ctx, segs.total), W = 255u / c + 1u, Wa = W / 2;
  int rc = ensure_lane(ctx, 1);
  if (rc) return rc;
  HIPCHK(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
  HIPCHK(ctx, hipStreamWaitEvent(ctx->lane[1].stream, ctx->ev_fork, 0));
  rc = msm_enqueue(ctx, MsmMode{}, 0, 0, segs, 0, Wa);
  if (rc) return rc;
  rc = msm_enqueue(ctx, MsmMode{}, 1, 1, segs, Wa, W - Wa);
  if (rc) { msm_abandon_pending(ctx, 1u); return rc; }
  bpmi_ctx::PendingMsm &p0 = ctx->pend[0], &p1 = ctx->pend[1];
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->lane[1].stream));
  const size_t b0 = 4ull * XYZZ_WORDS * p0.W * p0.nv, b1 = 4ull * XYZZ_WORDS * p1.W * p1.nv;
  std::vector<u32> E((b0 + b1) / 4);
  memcpy(E.data(), p0.pin, b0);
  memcpy((char *)E.data() + b0, p1.pin, b1);
  bpmi_host::tail_combine(out, E.data(), W, c, p0.to);
  p0.active = p1.active = false;
  return BPMI_OK;
}
// ---- large inputs as slices (msm_slice_count, msm_plan_host.hpp), two in flight on lanes 0 / 1 ----------------------------------------
static int msm_finish_pair(bpmi_ctx *ctx, uint8_t out0[64], uint8_t out1[64]);
static int msm_run_sliced(bpmi_ctx *ctx, const Segs &segs, uint64_t K, uint8_t out[64]) {
  for (int s = 0; s < 2; s++) if (ctx->pend[s].active || ctx->pend[s].async) return fail(ctx, BPMI_E_STATE, "an MSM is still pending in this slot (bpmi_msm_finish it first)");
  int rc = ensure_lane(ctx, 1);
  if (rc) return rc;
  HIPCHK(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
  HIPCHK(ctx, hipStreamWaitEvent(ctx->lane[1].stream, ctx->ev_fork, 0));
  const uint64_t total = segs.total, per = (total + K - 1) / K;
  bpmi_host::pt acc;
  bpmi_host::pt_set_inf(acc);
  // an error in the middle leaves the OTHER lane's slice queued: drain both lanes and release the slots of THIS call, or every later
  // MSM on this ctx would fail with "still pending"
  unsigned mine = 0;
  MsmMode mode;
  mode.chained = per >= (1u << 19);                  // (the accumulations chained as in bpmi_msm_dev_enqueue: each has the chip)
  auto leave = [&](int code) { ctx->accum_chain_lane = -1; if (code) msm_abandon_pending(ctx, mine); return code; };
  auto take = [&](int slot) -> int {
    uint8_t part[64];
    mine &= ~(1u << slot);
    const int r = msm_finish(ctx, slot, part);
    if (r) return r;
    bpmi_host::pt p;
    bpmi_host::pt_from_affine(p, part);
    bpmi_host::pt_add(acc, acc, p);
    return BPMI_OK;
  };
  ctx->accum_chain_lane = -1;
  for (uint64_t k = 0; k < K; k++) {
    const int lane = (int)(k & 1);
    if (k >= 2) { rc = take(lane); if (rc) return leave(rc); }
    const MsmSlice sl = msm_slice(total, per, k);
    rc = msm_enqueue(ctx, mode, lane, lane, segs_slice(segs, sl.lo, sl.cnt));
    if (rc) return leave(rc);
    mine |= 1u << lane;
  }
  {
    // the last two slices: their host tails side by side (the second on the ctx's helper thread, msm_finish_pair), oldest first in the sum
    uint8_t part[2][64];
    mine = 0;
    rc = msm_finish_pair(ctx, part[0], part[1]);
    if (rc) return leave(rc);
    for (uint64_t k = K - 2; k < K; k++) {
      bpmi_host::pt p;
      bpmi_host::pt_from_affine(p, part[k & 1]);
      bpmi_host::pt_add(acc, acc, p);
    }
  }
  bpmi_host::pt_to_affine(out, acc);
  return leave(BPMI_OK);
}
static int msm_run(bpmi_ctx *ctx, const Segs &segs, uint8_t out[64]) {
  if (segs.total > BPMI_MAX_N) return fail(ctx, BPMI_E_ARG, "n exceeds BPMI_MAX_N");
  {
    const uint64_t K = msm_slice_count(*ctx, segs);
    if (K > 1) return msm_run_sliced(ctx, segs, K, out);
  }
  if (ctx->opt_split == 1 && segs.total >= 2) return msm_run_split(ctx, segs, out);
  int rc = msm_enqueue(ctx, MsmMode{}, 0, 0, segs);
  if (rc) return rc;
  return msm_finish(ctx, 0, out);
}
// finish both slots of a synchronous pair; the second tail on the helper thread (it waits for its own event there)
static int msm_finish_pair(bpmi_ctx *ctx, uint8_t out0[64], uint8_t out1[64]) {
  if (!ctx->opt_tail_thread || !ctx->pend[0].active || !ctx->pend[1].active) {
    const int rc = msm_finish(ctx, 0, out0), rc1 = msm_finish(ctx, 1, out1);
    return rc ? rc : rc1;
  }
  if (!ctx->helper) ctx->helper = new HostHelper();
  bpmi_ctx::PendingMsm &pd = ctx->pend[1];
  hipError_t e1 = hipSuccess;
  const int dev = ctx->device;
  ctx->helper->submit([&pd, &e1, out1, dev, ctx] {           // (no ctx->err from this thread: the code travels back in e1)
    (void)hipSetDevice(dev);
    e1 = wait_event(ctx, pd.done);
    if (e1 != hipSuccess) return;
    if (pd.tail == 1) memcpy(out1, pd.pin, 64);
    else bpmi_host::tail_combine(out1, (const u32 *)pd.pin, pd.W, pd.c, pd.to);
  });
  const int rc = msm_finish(ctx, 0, out0);
  ctx->helper->wait();
  pd.active = false;
  if (rc) return rc;
  HIPCHK(ctx, e1);
  return BPMI_OK;
}
// Two SMALL MSMs (both on the one-launch kernel's path) as one launch sequence on the ctx stream: one k_msm_small_pair, one
// combine, the two copies; pending slots 0 and 1 as for a pair on two lanes.  (Two lanes cost a fork event, a second queue's
// doorbell and a second wait: ~40 us of a 0.3 ms round of the inner-product argument.)
static int msm_enqueue_small_pair(bpmi_ctx *ctx, const Segs &s0, const Segs &s1, bool mid) {
  bpmi_ctx::PendingMsm &p0 = ctx->pend[0], &p1 = ctx->pend[1];
  if (p0.active || p1.active) return fail(ctx, BPMI_E_STATE, "an MSM is still pending in this slot (bpmi_msm_finish it first)");
  SmallPair sp;
  CombinePair cp;
  MidPair mp;
  memset(&mp, 0, sizeof(mp));
  const Segs *ss[2] = {&s0, &s1};
  size_t off[2], total = 0;
  MsmWs w[2];
  MsmGeom gg[2];
  const u32 c = mid ? MID_C : SMALL_C;
  for (int j = 0; j < 2; j++) {
    MsmGeom &g = gg[j];
    memset(&g, 0, sizeof(g));
    g.n = ss[j]->total; g.c = c; g.W = 255u / g.c + 1u; g.w0 = 0; g.B = 1u << (g.c - 1); g.G = g.W * g.B; g.L = 8; g.nv = 1;
    msm_layout(g, w[j], nullptr);
    off[j] = total;
    total += align_up(w[j].total, 256);
  }
  int rc = ensure_ws(ctx, total);
  if (rc) return rc;
  const u32 parts = mid ? mid_parts(*ctx, std::max(s0.total, s1.total)) : 1u;
  const size_t eb = 4ull * XYZZ_WORDS * gg[0].W * parts;
  for (int j = 0; j < 2; j++) { rc = ensure_pin_slot(ctx, j, eb); if (rc) return rc; }
  u32 Smax = 1, threads = 64;
  for (int j = 0; j < 2; j++) {
    msm_layout(gg[j], w[j], (char *)ctx->lane[0].ws + off[j]);
    const uint64_t n = ss[j]->total;
    const u32 S = (u32)std::min<uint64_t>(64, (n + 255) / 256);
    u32 *const E_dst = ctx->opt_direct ? (u32 *)ctx->pend[j].pin : w[j].E;        // (see msm_enqueue: straight into the slot's host buffer)
    sp.segs[j] = *ss[j]; sp.g[j] = gg[j]; sp.S[j] = S; sp.out[j] = S > 1 ? w[j].buckets : E_dst;
    cp.part[j] = w[j].buckets; cp.S[j] = S; cp.E[j] = E_dst;
    mp.segs[j] = *ss[j]; mp.g[j] = gg[j]; mp.E[j] = E_dst;
    Smax = std::max(Smax, S);
    threads = std::max(threads, (u32)std::min<uint64_t>(256, (n + 63) / 64 * 64));
  }
  hipStream_t st = ctx->stream;
  {
    StageTimer t(ctx, ST_ACCUM, st);
    if (mid) hipLaunchKernelGGL(k_msm_mid, dim3(gg[0].W, 2, parts), dim3(MID_THREADS), 0, st, mp);
    else {
      hipLaunchKernelGGL(k_msm_small_pair, dim3(gg[0].W, Smax, 2), dim3(threads), 0, st, sp);
      if (Smax > 1) hipLaunchKernelGGL(k_small_combine_pair, dim3(gg[0].W, 2), dim3(64), 0, st, cp);
    }
  }
  debug_sync(ctx, "k_msm_small_pair / k_msm_mid", st);
  TailOffs to;
  memset(&to, 0, sizeof(to));
  to.nv = parts;
  // a failure from here on leaves none of THIS call's slots pending (both were free on entry: nobody else's is touched)
  unsigned mine = 0;
  auto queue_results = [&]() -> int {
    for (int j = 0; j < 2; j++) {
      bpmi_ctx::PendingMsm &pd = ctx->pend[j];
      if (!ctx->opt_direct) HIPCHK(ctx, hipMemcpyAsync(pd.pin, w[j].E, eb, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipEventRecord(pd.done, st));
      pd.active = true; pd.W = gg[j].W; pd.nv = parts; pd.c = c; pd.tail = 2; pd.to = to;
      mine |= 1u << j;
    }
    HIPCHK(ctx, hipGetLastError());
    return BPMI_OK;
  };
  rc = queue_results();
  if (rc && mine) msm_abandon_pending(ctx, mine);
  return rc;
}
// two independent MSMs, overlapped on the two lanes; everything already enqueued on the
// ctx stream (the producers of the scalars) is ordered before both
static int msm_run_pair(bpmi_ctx *ctx, const Segs &s0, uint8_t out0[64], const Segs &s1, uint8_t out1[64]) {
  if (s0.total > BPMI_MAX_N || s1.total > BPMI_MAX_N) return fail(ctx, BPMI_E_ARG, "n exceeds BPMI_MAX_N");
  {
    const uint64_t small_max = ctx->opt_small < 0 ? 0 : (ctx->opt_small ? (uint64_t)ctx->opt_small : SMALL_N_DEFAULT);
    const uint64_t mid_min = ctx->opt_mid_min > 0 ? (uint64_t)ctx->opt_mid_min : MID_MIN_DEFAULT;
    const uint64_t big = std::max<uint64_t>(s0.total, s1.total);
    const bool mid = ctx->opt_mid_min >= 0 && big >= mid_min && big <= MID_NMAX && ctx->opt_glv <= 0;
    if (ctx->opt_pair1 && ctx->opt_c == 0 && s0.total && s1.total && (mid || big <= small_max)) {
      int rc = msm_enqueue_small_pair(ctx, s0, s1, mid);           // (cleans up after itself)
      if (rc) return rc;
      return msm_finish_pair(ctx, out0, out1);
    }
  }
  int rc = ensure_lane(ctx, 1);
  if (rc) return rc;
  HIPCHK(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
  HIPCHK(ctx, hipStreamWaitEvent(ctx->lane[1].stream, ctx->ev_fork, 0));
  // (chaining the pair's accumulate kernels with the event of the asynchronous pipeline was measured on the IPA's 2^20-sized
  // rounds: 2.43 ms per round against 2.35 -- with only two MSMs there is no steady state to pipeline)
  const bool big = s0.total >= (1u << 19) && s1.total >= (1u << 19);
  // Round 6 experiment (option "pair_sched", off): a pair of LARGE MSMs as  sort 0 | sort 1 -> accumulation 0 -> accumulation 1 (reduction 0
  // beside it) -> reduction 1.  Queued one whole MSM after the other, the second MSM's sort meets the first one's accumulation and crawls
  // beside it (k_partition -- 1 024-thread blocks with 67 KB of LDS -- 1 025 us instead of 60, the accumulation beside it 1 126 instead of
  // 780: profiles/r06_C3_big_round_timeline.txt); with the schedule every kernel runs at its own speed (same file, second half) and the
  // round takes exactly as long: 2.41-2.57 ms either way, 23.9 / 25.6 against 24.4 / 24.6 ms per proof (profiles/r06_C3_pair_sched_ab.txt).
  // A pair has no steady state: two sorts (0.3 ms) + two accumulations (0.78 + 0.95 with the first reduction beside the second) + the last
  // reduction + the host tail IS the round, however it is interleaved -- what round 4 found for "pair_phases" and round 3 for "pair_chain".
  const bool sched = ctx->opt_pair_sched && big && !ctx->opt_graph;
  const bool chain = sched || (ctx->opt_pair_chain && big);
  MsmMode mode;
  mode.chained = chain;
  mode.beside = ctx->opt_pair_rounds != 1 && big;      // (msm_pick_geometry: multi-round chunks; the same geometry in both phases)
  if (chain) ctx->accum_chain_lane = -1;
  auto leave = [&](int code) { if (chain) ctx->accum_chain_lane = -1; return code; };
  // Round 4 experiment (option "pair_phases", off): both sorts first, then both accumulations, nothing else ordered.  Measured: NO difference
  // (2.336 / 2.330 against 2.343 / 2.319 ms for a round of the 2^20-element prover, profiles/r04_C3_pair_phases_ab.txt)
  const bool phases = sched || (ctx->opt_pair_phases && !chain && !ctx->opt_graph && s0.total >= (1u << 15) && s1.total >= (1u << 15));
  if (phases) {
    rc = msm_enqueue(ctx, mode, 0, 0, s0, 0, 0, 1);
    if (rc == BPMI_OK) rc = msm_enqueue(ctx, mode, 1, 1, s1, 0, 0, 1);
    if (rc) { msm_abandon_pending(ctx, 0u); return leave(rc); }        // (nothing pending yet: only drains the lanes)
    if (sched) {                                         // lane 0's accumulation behind lane 1's sort as well
      hipError_t e = hipEventRecord(ctx->ev_join, ctx->lane[1].stream);
      if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0);
      if (e != hipSuccess) { msm_abandon_pending(ctx, 0u); return leave(fail(ctx, BPMI_E_HIP, std::string("msm_run_pair: ") + hipGetErrorString(e))); }
    }
  }
  rc = msm_enqueue(ctx, mode, 0, 0, s0, 0, 0, phases ? 2 : 0);
  if (rc == BPMI_OK) {
    rc = msm_enqueue(ctx, mode, 1, 1, s1, 0, 0, phases ? 2 : 0);
    if (rc) msm_abandon_pending(ctx, 1u);
  }
  leave(0);
  if (rc) return rc;
  return msm_finish_pair(ctx, out0, out1);
}
