// context.hpp -- part of libbpmi (included by bpmi.hip; one translation unit).
// Engine context: lanes (stream + workspace), error reporting, per-stage HIP-event timers.
#pragma once

// ------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------
enum Stage {
  ST_DIGITS = 0, ST_SCAN, ST_SCATTER, ST_ACCUM, ST_SEGSCAN, ST_BREDUCE, ST_TAIL,
  ST_MULBATCH, ST_LINCOMB2, ST_SCDOT, ST_SCFOLD, ST_MISC, ST_RPPREP, ST_DECOMP, ST_RPELEM
};
static const char *STAGE_NAMES[BPMI_NSTAGES] = {
  "msm_digits_hist", "msm_scan", "msm_scatter", "msm_accumulate", "msm_segscan", "msm_bucket_reduce",
  "msm_tail", "ec_mul_batch", "ec_lincomb2", "sc_dot", "sc_fold", "misc", "rp_prepare", "ec_decompress", "rp_elements"
};

struct EvPair { int stage; hipEvent_t a, b; };
#define BPMI_LANES 3          // streams / workspaces / pending-MSM slots of a ctx

struct HostHelper;
struct MsmGraphCache;
// One MSM lane: a stream and a workspace of its own, so that independent MSMs overlap -- the latency-bound stages of one hide under
// the throughput-bound stages of the other.  Lane 0's stream is the ctx stream; lane 1 carries the second MSM of a pair (the L and R
// of an IPA round); only the asynchronous MSM pipeline uses lane 2 (slot 2 of bpmi_msm_dev_enqueue with option async_lanes): with
// three MSMs in flight the sort of MSM k + 1 is on the GPU while MSM k accumulates and MSM k - 1 is being reduced.
struct Lane {
  hipStream_t stream = nullptr;
  void *ws = nullptr; size_t ws_bytes = 0;       // workspace (grown on demand, never shrunk)
  // software pipeline of the asynchronous MSM pair on two lanes: the accumulate kernel of an MSM waits for the
  // accumulate kernel of the MSM enqueued before it (on the other lane), so the throughput-bound stage always has the
  // whole GPU while the other lane's latency-bound tail (segmented scan, bucket reduction) and next sort run beside it
  hipEvent_t ev_accum = nullptr;
  hipEvent_t ev_sorted = nullptr;                // option accum_stream: this lane's sort is in
  // the last bucket-pipeline MSM queued on this lane: was the accumulation by runs planned, and where its flag words are (bpmi_debug_msm_runs)
  const u32 *run_flags = nullptr; u32 run_planned = 0;
};
struct bpmi_ctx : BpmiOptions {
  int device = 0;
  Lane lane[BPMI_LANES];
  hipStream_t &stream = lane[0].stream;          // the ctx stream IS lane 0's (the caller's when own_stream is false)
  bool own_stream = false;
  std::string err;
  void *pin = nullptr; size_t pin_bytes = 0;       // pinned host staging
  hipEvent_t ev_slice[4] = {nullptr, nullptr, nullptr, nullptr};      // batch preparation: upload slice c has arrived
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;      // fork: lane 1 may start; join: lane 1's work is in (batch preparation)
  int accum_chain_lane = -1;     // lane whose ev_accum is the newest, -1: none pending
  void *up_ring = nullptr;       // page-locked staging ring of h2d()
  size_t up_cursor = 0;
  hipEvent_t up_ev = nullptr;
  bool up_pending = false;
  // One in-flight MSM: its own pinned host buffer (what the tail reads) and its own completion event, so
  // that finishing it never waits for work enqueued behind it (bpmi_msm_dev_enqueue / bpmi_msm_finish
  // keep two MSMs in flight on ONE stream: the host tail of MSM k overlaps the kernels of MSM k + 1).
  struct PendingMsm {
    bool active = false; u32 W = 0, nv = 0, c = 0; int tail = 2; TailOffs to;
    void *pin = nullptr; size_t pin_bytes = 0; hipEvent_t done = nullptr; bool async = false, async_empty = false;
  } pend[BPMI_LANES];
  void *stage_in = nullptr; size_t stage_in_bytes = 0;  // device staging for host-pointer entry points
  // (the options: struct BpmiOptions, shared_defs.hpp)
  void *rp_buf = nullptr; size_t rp_buf_bytes = 0;   // batch preparation: per-proof contributions to the shared generators
  uint64_t ipap_t_budget = 0;                        // bpmi_debug_ipap_t_budget: bytes of one round's transposed transcripts of the mixed packed calls and of the grouped one (0: IPAP_T_BYTES_MAX)
  bool async_lanes_ordered = false;                  // option async_lanes: this burst's extra lanes are ordered behind the ctx stream
  void *fold_tab = nullptr; size_t fold_tab_bytes = 0;     // tables + scratch of the width-4 NAF generator fold, allocated at the first fold, kept
  const void *fold_key_g = nullptr, *fold_key_h = nullptr; uint64_t fold_key_n = 0;     // whose tables fold_tab holds (nullptr: nobody's)
  // profiling
  bool prof = false;
  int prof_only = -1;      // >= 0: time only this stage (every event record costs a ~10 us bubble between kernels)
  std::vector<EvPair> evs;
  std::vector<hipEvent_t> ev_pool;      // recycled timing events (creating one costs more than recording it)
  HostHelper *helper = nullptr;
  MsmGraphCache *graphs = nullptr;      // captured launch sequences of repeated MSMs (msm_host.hpp)
  u32 *vflag = nullptr, *vflag_dev = nullptr;      // the points' on-curve check's verdict (smallest bad index, ~0 = none): device word, and the page-locked word it is copied to
  hipStream_t stream_acc = nullptr;     // option accum_stream: the accumulations' own stream
  double prof_ms[BPMI_NSTAGES] = {0};
  uint64_t prof_calls[BPMI_NSTAGES] = {0};
};
// every lane that exists has run dry; the first error
static hipError_t sync_lanes(bpmi_ctx *ctx) {
  hipError_t first = hipSuccess;
  for (Lane &l : ctx->lane)
    if (l.stream) { const hipError_t e = hipStreamSynchronize(l.stream); if (first == hipSuccess) first = e; }
  return first;
}

// One helper thread per ctx (started at first use) for host work that can run beside the calling thread's: the host tail of the
// second MSM of a synchronous pair (40 us of field arithmetic per MSM; 20 rounds of an inner-product argument pay it twice each).
struct HostHelper {
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  std::function<void()> job;
  bool has_job = false, done = true, quit = false;
  void start() {
    if (th.joinable()) return;
    th = std::thread([this] {
      std::unique_lock<std::mutex> lk(mu);
      for (;;) {
        cv.wait(lk, [this] { return has_job || quit; });
        if (quit) return;
        std::function<void()> j = std::move(job);
        has_job = false;
        lk.unlock();
        j();
        lk.lock();
        done = true;
        cv.notify_all();
      }
    });
  }
  void submit(std::function<void()> j) {
    start();
    std::lock_guard<std::mutex> lk(mu);
    job = std::move(j); has_job = true; done = false;
    cv.notify_all();
  }
  void wait() {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [this] { return done; });
  }
  ~HostHelper() {
    if (!th.joinable()) return;
    { std::lock_guard<std::mutex> lk(mu); quit = true; cv.notify_all(); }
    th.join();
  }
};

static std::string g_create_err;
static std::mutex g_mu;

static int fail(bpmi_ctx *ctx, int code, const std::string &msg) {
  if (ctx) ctx->err = msg;
  else { std::lock_guard<std::mutex> lk(g_mu); g_create_err = msg; }
  return code;
}
#define HIPCHK(ctx, call)                                                                   \
  do {                                                                                      \
    hipError_t e_ = (call);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return fail(ctx, e_ == hipErrorOutOfMemory ? BPMI_E_NOMEM : BPMI_E_HIP,               \
                  std::string(#call) + ": " + hipGetErrorString(e_));                       \
  } while (0)

static bool g_debug_sync = getenv("BPMI_DEBUG_SYNC") != nullptr;
static void debug_sync(bpmi_ctx *ctx, const char *what, hipStream_t stream = nullptr) {
  if (!g_debug_sync) return;
  fprintf(stderr, "[bpmi] sync after %s ... ", what); fflush(stderr);
  hipError_t e = hipStreamSynchronize(stream ? stream : ctx->stream);
  fprintf(stderr, "%s\n", hipGetErrorString(e)); fflush(stderr);
}
struct StageTimer {
  bpmi_ctx *ctx; int stage; hipStream_t stream; hipEvent_t a = nullptr, b = nullptr;
  StageTimer(bpmi_ctx *c, int s, hipStream_t st = nullptr) : ctx(c), stage(s), stream(st ? st : c->stream) {
    if (ctx->prof && (ctx->prof_only < 0 || ctx->prof_only == stage)) {
      a = take(); b = take();
      if (!a || !b) { a = b = nullptr; return; }
      (void)hipEventRecord(a, stream);
    }
  }
  hipEvent_t take() {
    if (!ctx->ev_pool.empty()) { hipEvent_t e = ctx->ev_pool.back(); ctx->ev_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    return hipEventCreate(&e) == hipSuccess ? e : nullptr;
  }
  ~StageTimer() {
    if (ctx->prof && a) { (void)hipEventRecord(b, stream); ctx->evs.push_back({stage, a, b}); }
  }
};

// Host -> device copies of 4 KB .. 8 MB from PAGEABLE memory go through a page-locked ring of the ctx.  Left to the runtime such
// a copy pins the caller's pages on the fly, and on a busy host that took 9 ms for the 1.5 MB of a bpmi_msm2 call (0.1 ms on a
// quiet one: config C4's prover 31-39 ms instead of 10.5 on one box in four).  Sources that are already page-locked
// (bpmi_host_alloc: the batch verifier's receive buffers) and very large or tiny copies go straight to the runtime.
#define UP_RING_BYTES (32u << 20)
static hipError_t h2d(bpmi_ctx *ctx, void *dst, const void *src, size_t bytes, hipStream_t st) {
  if (bytes < 4096 || bytes > (8u << 20)) return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, src) == hipSuccess && attr.type == hipMemoryTypeHost) return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
  (void)hipGetLastError();                                  // an ordinary host pointer is "invalid value" to the query
  if (!ctx->up_ring) {
    if (hipHostMalloc(&ctx->up_ring, UP_RING_BYTES, hipHostMallocDefault) != hipSuccess) { ctx->up_ring = nullptr; (void)hipGetLastError(); return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st); }
    if (hipEventCreateWithFlags(&ctx->up_ev, hipEventDisableTiming) != hipSuccess) {       // no ring without its event: the runtime's own copy
      (void)hipGetLastError();
      (void)hipHostFree(ctx->up_ring);
      ctx->up_ring = nullptr; ctx->up_ev = nullptr;
      return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
    }
  }
  const size_t need = (bytes + 255) & ~(size_t)255;
  if (ctx->up_cursor + need > UP_RING_BYTES) {              // wrap: everything queued from the ring so far must have left it
    if (ctx->up_pending) {                                  // (the event covers the stream of the last copy; the ctx's streams are few)
      hipError_t e = hipEventSynchronize(ctx->up_ev);
      if (e == hipSuccess) e = sync_lanes(ctx);
      if (e != hipSuccess) return e;
    }
    ctx->up_cursor = 0;
  }
  char *stage = (char *)ctx->up_ring + ctx->up_cursor;
  ctx->up_cursor += need;
  memcpy(stage, src, bytes);
  hipError_t e = hipMemcpyAsync(dst, stage, bytes, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) { e = hipEventRecord(ctx->up_ev, st); ctx->up_pending = true; }
  return e;
}
// Waits of the latency-critical paths.  Polling the event before sleeping in the runtime (option "spin_wait" = number of polls) was
// tried against the slow boxes of the pool and is OFF: the slowness was the pageable uploads (h2d above), the polls change nothing
// for one caller (C2 0.36 ms, C4 10.3 ms either way) and cost the batch verifier's eight threads 4.5 % of their throughput
// (profiles/r03_spin_wait_ab.txt).
static hipError_t wait_event(const bpmi_ctx *ctx, hipEvent_t ev) {
  for (int spin = 0; spin < ctx->opt_spin_wait; spin++) {           // some tens of milliseconds at most (option "spin_wait", per ctx)
    const hipError_t e = hipEventQuery(ev);
    if (e != hipErrorNotReady) return e;
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
  }
  return hipEventSynchronize(ev);
}
static hipError_t wait_stream(const bpmi_ctx *ctx, hipStream_t st) {
  for (int spin = 0; spin < ctx->opt_spin_wait; spin++) {
    const hipError_t e = hipStreamQuery(st);
    if (e != hipErrorNotReady) return e;
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
  }
  return hipStreamSynchronize(st);
}
static void msm_graphs_clear(bpmi_ctx *ctx);
static int ensure_ws(bpmi_ctx *ctx, size_t bytes, int lane = 0) {
  Lane &l = ctx->lane[lane];
  if (bytes <= l.ws_bytes) return BPMI_OK;
  msm_graphs_clear(ctx);                 // captured sequences hold pointers into the workspace
  if (l.ws) { HIPCHK(ctx, hipStreamSynchronize(l.stream)); HIPCHK(ctx, hipFree(l.ws)); l.ws = nullptr; l.ws_bytes = 0; }
  const size_t want = bytes + bytes / 8;
  HIPCHK(ctx, hipMalloc(&l.ws, want));
  l.ws_bytes = want;
  return BPMI_OK;
}
static int ensure_lane(bpmi_ctx *ctx, int lane) {
  if (lane == 0) return BPMI_OK;
  if (!ctx->lane[1].stream) {
    HIPCHK(ctx, hipStreamCreateWithPriority(&ctx->lane[1].stream, hipStreamNonBlocking, ctx->opt_lane_prio));
    HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
    HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
    for (Lane &l : ctx->lane) HIPCHK(ctx, hipEventCreateWithFlags(&l.ev_accum, hipEventDisableTiming));
  }
  if (lane == 2 && !ctx->lane[2].stream) HIPCHK(ctx, hipStreamCreateWithPriority(&ctx->lane[2].stream, hipStreamNonBlocking, ctx->opt_lane_prio));
  if (ctx->opt_accum_stream && !ctx->stream_acc) {
    int least = 0, greatest = 0;
    HIPCHK(ctx, hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIPCHK(ctx, hipStreamCreateWithPriority(&ctx->stream_acc, hipStreamNonBlocking, ctx->opt_accum_stream == 2 ? 0 : least));
    for (Lane &l : ctx->lane) HIPCHK(ctx, hipEventCreateWithFlags(&l.ev_sorted, hipEventDisableTiming));
  }
  return BPMI_OK;
}
static int ensure_pin_slot(bpmi_ctx *ctx, int slot, size_t bytes);
static int ensure_stage_in(bpmi_ctx *ctx, size_t bytes) {
  if (bytes <= ctx->stage_in_bytes) return BPMI_OK;
  if (ctx->stage_in) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHK(ctx, hipFree(ctx->stage_in)); ctx->stage_in = nullptr; ctx->stage_in_bytes = 0; }
  HIPCHK(ctx, hipMalloc(&ctx->stage_in, bytes));
  ctx->stage_in_bytes = bytes;
  return BPMI_OK;
}
static int ensure_pin(bpmi_ctx *ctx, size_t bytes) {
  if (bytes <= ctx->pin_bytes) return BPMI_OK;
  if (ctx->pin) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHK(ctx, hipHostFree(ctx->pin)); ctx->pin = nullptr; ctx->pin_bytes = 0; }
  HIPCHK(ctx, hipHostMalloc(&ctx->pin, bytes, hipHostMallocDefault));
  ctx->pin_bytes = bytes;
  return BPMI_OK;
}

// pinned buffer + completion event of pending-MSM slot `slot`
static int ensure_pin_slot(bpmi_ctx *ctx, int slot, size_t bytes) {
  bpmi_ctx::PendingMsm &pd = ctx->pend[slot];
  if (!pd.done) HIPCHK(ctx, hipEventCreateWithFlags(&pd.done, hipEventDisableTiming));
  if (bytes <= pd.pin_bytes) return BPMI_OK;
  msm_graphs_clear(ctx);
  if (bytes < 16384) bytes = 16384;
  if (pd.pin) { HIPCHK(ctx, hipEventSynchronize(pd.done)); HIPCHK(ctx, hipHostFree(pd.pin)); pd.pin = nullptr; pd.pin_bytes = 0; }
  HIPCHK(ctx, hipHostMalloc(&pd.pin, bytes, hipHostMallocDefault));
  pd.pin_bytes = bytes;
  return BPMI_OK;
}
