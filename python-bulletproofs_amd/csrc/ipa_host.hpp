// ipa_host.hpp -- part of libbpmi (included by bpmi.hip; one translation unit).  HOST code.
// The inner-product prover (/root/reference/src/innerproduct/inner_product_prover.py:94-110): the state object bpmi_ipa with its deferred
// generator folding, and the bpmi_ipa_* entry points -- create, round_LR, fold, prove_rounds, finish, export, destroy.  bpmi_ipa_fold is a
// dispatcher over one function per algorithm; the digit tables its generator folds send down are built in fold_ops_host.hpp.
// Kernels: point_kernels.hpp, scalar_kernels.hpp.  The verifier (bpmi_ipa_verify_dev) is in bpmi.hip.
#pragma once

// ---- IPA prover state ---------------------------------------------------------------------------
struct bpmi_ipa {
  bpmi_ctx *ctx;
  uint64_t n0, n;       // initial and current LOGICAL length m
  uint64_t M;           // length of the (unfolded) base arrays g, h;  M = n << d
  u32 d;                // deferred folds
  uint64_t big_m;       // materialisation threshold (ctx option ipa_big_m)
  u32 *g, *h;           // device bases (M points each)
  u32 *g2, *h2;         // device, materialisation targets (M/16 points each)
  u32 *a, *b;           // device, folded in place every round
  u32 *eg, *eh, *eg2, *eh2;   // device, expanded scalars for the deferred L and R MSMs (M each)
  u32 *cg[2], *ch[2];   // device coefficient tables (ping-pong), 2^d entries in cg[cur]
  int cur;
  u32 *u;               // device, 64 B point
  u32 *cl, *cr;         // device, 32 B scalars (stay on device between dot and MSM)
  u32 *partial;         // device scratch for dots
  NafK *nafk[2];        // device, NAF tables for the multifold kernel
  u32 *hscale_buf;      // device, room for n0 scalars
  u32 *hscale;          // device, optional per-base scale of the h generators (n0 scalars) or nullptr
  uint64_t small_m;     // logical length at which bases below big_m are folded through products (0: never)
  void *block;          // one allocation
  std::vector<sc> hcg, hch;   // host copies of the coefficient tables while 2^d <= 16
  bool lr_done;
  bool prep_ready;      // the scalars of the next L / R and c_L, c_R are on the device already (k_ipa_small_step did the next round's preparation)
  const void *src_g = nullptr, *src_h = nullptr;      // bpmi_ipa_create_dev: the caller's generator arrays (the key of the kept fold tables, option ipa_fixed_generators)
};

// deferral policy: bases of 2^18 points or more are folded 16-way at once (an MSM over the
// unfolded bases costs ~2.6 ms per L/R at 2^20 against ~50 ms for the pairwise ladder fold,
// while a K-term ladder stays throughput-bound only for many outputs); smaller bases are
// never folded -- the prover needs L and R, not the folded generators, and a ladder launch
// is ~2 ms of pure latency.
#define IPA_BIG_M_DEFAULT (1u << 18)
#define IPA_BIG_D 4
// Round 4: bases BELOW that threshold (the 2^16 points per side a 2^20-element proof is left with after its 16-way fold; the 2^14
// generators of an aggregated 128 x 64-bit range proof) are folded ONCE more, when the logical length reaches 4 096, through
// per-term products (k_ipa_fold_scalars, bpmi_ec_mul_batch, k_ec_sum_strided: point_kernels.hpp) -- from there on L and R are MSMs
// over <= 4 097 pairs on the one-launch small-MSM kernel, both in one launch.  Option "ipa_small_m": 0 default, 1 never, else the length.
#define IPA_SMALL_M_DEFAULT 4096u

extern "C" {

static void ipa_free(bpmi_ipa *st) { (void)hipFree(st->block); delete st; }
static void host_sc_from(sc &r, const uint8_t b[32]) { memcpy(r.v, b, 32); }
static u32 ipa_log2(uint64_t n) { u32 k; (void)log2_exact(n, k); return k; }          // smallest k with 2^k >= n
// the host copies of the coefficient tables := [1]
static void ipa_host_coef_one(bpmi_ipa *st) {
  sc o; memset(&o, 0, sizeof(o)); o.v[0] = 1;
  st->hcg.assign(1, o); st->hch.assign(1, o);
}

static int ipa_alloc(bpmi_ctx *ctx, uint64_t n, bpmi_ipa **out) {
  bpmi_ipa *st = new bpmi_ipa();
  st->ctx = ctx; st->n0 = st->n = st->M = n; st->d = 0; st->cur = 0; st->lr_done = false; st->prep_ready = false;
  st->big_m = ctx->opt_ipa_big > 0 ? (uint64_t)ctx->opt_ipa_big : IPA_BIG_M_DEFAULT;
  if (st->big_m < 32) st->big_m = 32;
  st->small_m = ctx->opt_ipa_small == 1 ? 0 : (ctx->opt_ipa_small > 1 ? (uint64_t)ctx->opt_ipa_small : IPA_SMALL_M_DEFAULT);
  const size_t pts = align_up(64 * n, 256), scs = align_up(32 * n, 256);
  // the targets of a fold: n / 16 points (the ladder's 16-way fold) or small_m points (the product fold of bases that were never folded)
  const size_t pts2 = align_up(64 * std::max<uint64_t>(n / 16 + 1, std::min<uint64_t>(n, st->small_m)), 256), coef = align_up(32 * n, 256);
  const size_t bytes = pts * 2 + pts2 * 2 + scs * 7 + coef * 4 + 256 * 3 + 2 * 32 * SC_DOT_MAX_BLOCKS + 2 * align_up(sizeof(NafK), 256);
  hipError_t e = hipMalloc(&st->block, bytes);
  if (e != hipSuccess) { delete st; return fail(ctx, BPMI_E_NOMEM, std::string("hipMalloc(ipa state): ") + hipGetErrorString(e)); }
  char *p = (char *)st->block;
  auto take = [&p](size_t b) { u32 *r = (u32 *)p; p += b; return r; };
  st->g = take(pts); st->h = take(pts); st->g2 = take(pts2); st->h2 = take(pts2);
  st->a = take(scs); st->b = take(scs);
  st->eg = take(scs); st->eh = take(scs); st->eg2 = take(scs); st->eh2 = take(scs);
  st->hscale = nullptr;
  st->hscale_buf = take(scs);
  for (int k = 0; k < 2; k++) { st->cg[k] = take(coef); st->ch[k] = take(coef); }
  st->u = take(256); st->cl = take(256); st->cr = take(256);
  st->partial = take(2 * 32 * SC_DOT_MAX_BLOCKS);
  for (int k = 0; k < 2; k++) st->nafk[k] = (NafK *)take(align_up(sizeof(NafK), 256));
  // coefficient tables start as [1]
  uint8_t one[32] = {1};
  e = h2d(ctx, st->cg[0], one, 32, ctx->stream);
  if (e == hipSuccess) e = h2d(ctx, st->ch[0], one, 32, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) { ipa_free(st); return fail(ctx, BPMI_E_HIP, std::string("ipa_alloc: ") + hipGetErrorString(e)); }
  ipa_host_coef_one(st);
  *out = st;
  return BPMI_OK;
}
static bool is_pow2(uint64_t n) { return n && !(n & (n - 1)); }

// the two constructors: the generators and vectors come from device memory (no validation; the arrays' addresses are remembered for
// option ipa_fixed_generators) or from the host
static int ipa_create_from(bpmi_ctx *ctx, bool on_device, const void *g, const void *h, const void *a, const void *b, uint64_t n,
                           const uint8_t u[64], bpmi_ipa **out) {
  if (!ctx || !g || !h || !a || !b || !u || !out) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  if (!is_pow2(n) || n > BPMI_MAX_N) return fail(ctx, BPMI_E_ARG, "n must be a power of two <= BPMI_MAX_N");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  bpmi_ipa *st = nullptr;
  int rc = ipa_alloc(ctx, n, &st);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  PointCheck pc(ctx, "bpmi_ipa_create", s, !on_device && ctx->opt_validate >= 1);
  rc = pc.host(u, 1, "u");
  if (rc) { ipa_free(st); return rc; }
  auto copy = [&](void *dst, const void *src, size_t bytes) {
    return on_device ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s) : h2d(ctx, dst, src, bytes, s);
  };
  hipError_t e = copy(st->g, g, 64 * n);
  if (e == hipSuccess) e = copy(st->h, h, 64 * n);
  if (e == hipSuccess) e = copy(st->a, a, 32 * n);
  if (e == hipSuccess) e = copy(st->b, b, 32 * n);
  if (e == hipSuccess) e = h2d(ctx, st->u, u, 64, s);
  if (e == hipSuccess) {
    pc.queue(st->g, n, "g");
    pc.queue(st->h, n, "h");
    rc = pc.fetch();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { ipa_free(st); return fail(ctx, BPMI_E_HIP, std::string("ipa_create copy: ") + hipGetErrorString(e)); }
  if (rc == BPMI_OK) rc = pc.verdict();
  if (rc) { ipa_free(st); return rc; }
  if (on_device) { st->src_g = g; st->src_h = h; }
  *out = st;
  return BPMI_OK;
}
int bpmi_ipa_create_dev(bpmi_ctx *ctx, const void *d_g, const void *d_h, const void *d_a, const void *d_b, uint64_t n,
                        const uint8_t u[64], bpmi_ipa **out) {
  return ipa_create_from(ctx, true, d_g, d_h, d_a, d_b, n, u, out);
}
int bpmi_ipa_create(bpmi_ctx *ctx, const uint8_t *g, const uint8_t *h, const uint8_t *a, const uint8_t *b, uint64_t n,
                    const uint8_t u[64], bpmi_ipa **out) {
  return ipa_create_from(ctx, false, g, h, a, b, n, u, out);
}
int bpmi_ipa_create_scaled(bpmi_ctx *ctx, const uint8_t *g, const uint8_t *h, const uint8_t *a, const uint8_t *b, uint64_t n,
                           const uint8_t u[64], const uint8_t *h_scale, bpmi_ipa **out) {
  int rc = bpmi_ipa_create(ctx, g, h, a, b, n, u, out);
  if (rc || !h_scale) return rc;
  bpmi_ipa *st = *out;
  if (n >= st->big_m) {
    // large bases get folded by the shared-scalar ladder, which needs real points: scale them once
    HIPCHK(ctx, h2d(ctx, st->hscale_buf, h_scale, 32 * n, ctx->stream));
    rc = bpmi_ec_mul_batch_dev(ctx, st->h, st->hscale_buf, n, st->h);
    if (rc == BPMI_OK) { hipError_t e = hipStreamSynchronize(ctx->stream); if (e != hipSuccess) rc = fail(ctx, BPMI_E_HIP, hipGetErrorString(e)); }
  } else {
    // never folded: the factors ride in the scalars of every L / R MSM
    hipError_t e = h2d(ctx, st->hscale_buf, h_scale, 32 * n, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) rc = fail(ctx, BPMI_E_HIP, std::string("ipa_create_scaled: ") + hipGetErrorString(e));
    else st->hscale = st->hscale_buf;
  }
  if (rc) { bpmi_ipa_destroy(st); *out = nullptr; }
  return rc;
}
uint64_t bpmi_ipa_len(const bpmi_ipa *st) { return st ? st->n : 0; }

int bpmi_ipa_round_LR(bpmi_ipa *st, uint8_t L[64], uint8_t R[64]) {
  if (!st || !L || !R) return BPMI_E_ARG;
  bpmi_ctx *ctx = st->ctx;
  if (st->n < 2) return fail(ctx, BPMI_E_STATE, "ipa already reduced to length 1");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const uint64_t np = st->n / 2;
  u32 *a_lo = st->a, *a_hi = st->a + 8 * np, *b_lo = st->b, *b_hi = st->b + 8 * np;
  const bool prepared = st->prep_ready;          // k_ipa_small_step left c_L, c_R and the expanded scalars of this round on the device
  st->prep_ready = false;
  // cl = <a_lo, b_hi>, cr = <a_hi, b_lo>  (inner_product_prover.py:96-97), kept on the device
  if (!prepared) {
    DotJobs dj;
    dj.a[0] = a_lo; dj.b[0] = b_hi; dj.out[0] = st->cl;
    dj.a[1] = a_hi; dj.b[1] = b_lo; dj.out[1] = st->cr;
    sc_dot_jobs(ctx, dj, 2, np, st->partial);                 // both in one pair of launches
  }
  int rc;
  if (st->d == 0 && !st->hscale) {
    // bases are the current generators: L = <a_lo, g_hi> + <b_hi, h_lo> + cl*u  (:98) as ONE
    // three-segment MSM, R = <a_hi, g_lo> + <b_lo, h_hi> + cr*u  (:99)
    u32 *g_lo = st->g, *g_hi = st->g + 16 * np, *h_lo = st->h, *h_hi = st->h + 16 * np;
    Segs sL = segs_init();
    sL.pts[0] = g_hi; sL.sc[0] = a_lo; sL.n[0] = (u32)np;
    sL.pts[1] = h_lo; sL.sc[1] = b_hi; sL.n[1] = (u32)np;
    sL.pts[2] = st->u; sL.sc[2] = st->cl; sL.n[2] = 1;
    sL.total = (u32)(2 * np + 1);
    Segs sR = segs_init();
    sR.pts[0] = g_lo; sR.sc[0] = a_hi; sR.n[0] = (u32)np;
    sR.pts[1] = h_hi; sR.sc[1] = b_lo; sR.n[1] = (u32)np;
    sR.pts[2] = st->u; sR.sc[2] = st->cr; sR.n[2] = 1;
    sR.total = (u32)(2 * np + 1);
    rc = msm_run_pair(ctx, sL, L, sR, R);
    if (rc) return rc;
  } else {
    // deferred: MSM over the UNFOLDED bases with the fold coefficients multiplied into the
    // scalars (half of them are zero and drop out in the digit pass)
    const u32 logm = ipa_log2(st->n);
    Segs sg[2];
    if (!prepared) {
      StageTimer t(ctx, ST_SCFOLD);
      ExpandOut eo;
      eo.eg[0] = st->eg; eo.eh[0] = st->eh; eo.eg[1] = st->eg2; eo.eh[1] = st->eh2;
      hipLaunchKernelGGL(k_ipa_expand, dim3((u32)((st->M + 255) / 256), 2), dim3(256), 0, ctx->stream, st->a, st->b, st->cg[st->cur], st->ch[st->cur],
                         st->hscale, (u32)st->M, logm, eo);           // the scalars of L and of R in one launch
    }
    for (int right = 0; right < 2; right++) {
      u32 *eg = right ? st->eg2 : st->eg, *eh = right ? st->eh2 : st->eh;
      // only the non-zero half of every block of m logical positions takes part: for L the
      // upper g-halves and lower h-halves (g_hi with a_lo, h_lo with b_hi), for R the opposite
      sg[right] = segs_init();
      sg[right].pts[0] = st->g; sg[right].sc[0] = eg; sg[right].n[0] = (u32)(st->M / 2);
      sg[right].pts[1] = st->h; sg[right].sc[1] = eh; sg[right].n[1] = (u32)(st->M / 2);
      sg[right].hlog[0] = sg[right].hlog[1] = logm - 1;
      sg[right].phase[0] = right ? 0u : 1u; sg[right].phase[1] = right ? 1u : 0u;
      sg[right].pts[2] = st->u; sg[right].sc[2] = right ? st->cr : st->cl; sg[right].n[2] = 1;
      sg[right].total = (u32)(st->M + 1);
    }
    rc = msm_run_pair(ctx, sg[0], L, sg[1], R);
    if (rc) return rc;
  }
  st->lr_done = true;
  return BPMI_OK;
}

// ---- bpmi_ipa_fold: one function per algorithm, and the predicates that choose among them ---------------------------------------
// short vectors: the fold of a and b, the coefficient tables AND the next round's c_L, c_R and expanded scalars in one launch
// (only where no generator fold can come any more: not above the ladder's threshold, not above the product fold's length)
static bool ipa_small_step_applies(const bpmi_ipa *st) {
  return st->ctx->opt_ipa_step && st->M <= 4096 && st->M == st->n << st->d && st->M < st->big_m && !(st->small_m && st->M > st->small_m);
}
// the host keeps its copies of the K = 2^d coefficients (doubling now) while a fold that builds its digit tables from them can come
static bool ipa_tracks_host_coef(const bpmi_ipa *st, u32 K) {
  return ((2 * K <= MULTIFOLD_MAXK) && st->M >= st->big_m) ||
         (2 * K <= GLVF_MAXK && st->small_m && st->M < st->big_m && st->M > st->small_m && !st->hscale && st->hcg.size() == K);
}
static bool ipa_ladder16_due(const bpmi_ipa *st) { return st->M >= st->big_m && st->d == IPA_BIG_D && st->n > 1; }
static bool ipa_products_due(const bpmi_ipa *st) {
  return st->small_m && st->M < st->big_m && st->n == st->small_m && st->M > st->n && st->n > 1 &&
         (2 * st->M >= (uint64_t)MULB_MIN_N || st->ctx->opt_ipa_small > 1);
}
// shared coefficients: GLV halves in non-adjacent form from the host, two terms per thread (k_ec_fold_glv)
static bool ipa_products_shared(const bpmi_ipa *st, u32 K) {
  return !st->hscale && st->hcg.size() == K && K % GLVF_TERMS == 0 && K <= GLVF_MAXK && st->n % 64 == 0 && st->ctx->opt_fold_shared;
}

static int ipa_small_step(bpmi_ipa *st, const uint8_t x[32], const uint8_t xinv[32]) {
  bpmi_ctx *ctx = st->ctx;
  const uint64_t np = st->n / 2;
  IpaStep ps;
  ps.a = st->a; ps.b = st->b;
  ps.cg = st->cg[st->cur]; ps.ch = st->ch[st->cur]; ps.cg2 = st->cg[st->cur ^ 1]; ps.ch2 = st->ch[st->cur ^ 1];
  memcpy(ps.x_xinv.k1, x, 32); memcpy(ps.x_xinv.k2, xinv, 32);
  ps.np = (u32)np; ps.K = 1u << st->d; ps.M = (u32)st->M;
  ps.hscale = st->hscale; ps.cl = st->cl; ps.cr = st->cr;
  ps.eg[0] = st->eg; ps.eh[0] = st->eh; ps.eg[1] = st->eg2; ps.eh[1] = st->eh2;
  {
    StageTimer t(ctx, ST_SCFOLD);
    hipLaunchKernelGGL(k_ipa_small_step, dim3(1), dim3(1024), 0, ctx->stream, ps);
  }
  HIPCHK(ctx, hipGetLastError());
  st->cur ^= 1;
  st->d += 1;
  st->n = np;
  st->lr_done = false;
  st->prep_ready = np >= 2;
  return BPMI_OK;
}

// a, b and the coefficient tables of the deferred generator fold, on the device and (ipa_tracks_host_coef) on the host
static void ipa_fold_vectors(bpmi_ipa *st, const uint8_t x[32], const uint8_t xinv[32]) {
  bpmi_ctx *ctx = st->ctx;
  const uint64_t np = st->n / 2;
  // a' = x a_lo + x^-1 a_hi ; b' = x^-1 b_lo + x b_hi  (:109-110)
  {
    FoldJobs fj;
    fj.lo[0] = st->a; fj.hi[0] = st->a + 8 * np; fj.out[0] = st->a;
    fj.lo[1] = st->b; fj.hi[1] = st->b + 8 * np; fj.out[1] = st->b;
    memcpy(fj.xy[0].k1, x, 32); memcpy(fj.xy[0].k2, xinv, 32);
    memcpy(fj.xy[1].k1, xinv, 32); memcpy(fj.xy[1].k2, x, 32);
    StageTimer t(ctx, ST_SCFOLD);
    hipLaunchKernelGGL(k_sc_fold, dim3((u32)((np + 255) / 256), 2), dim3(256), 0, ctx->stream, fj, (u32)np);       // a and b in one launch
  }
  // g' = x^-1 g_lo + x g_hi ; h' = x h_lo + x^-1 h_hi  (:107-108): deferred -- only the
  // coefficient tables double
  const u32 K = 1u << st->d;
  Sc2 xs;
  memcpy(xs.k1, x, 32); memcpy(xs.k2, xinv, 32);
  {
    StageTimer t(ctx, ST_SCFOLD);
    hipLaunchKernelGGL(k_ipa_coef_update, dim3((2 * K + 255) / 256), dim3(256), 0, ctx->stream, st->cg[st->cur], st->ch[st->cur], xs, K, st->cg[st->cur ^ 1], st->ch[st->cur ^ 1]);
  }
  st->cur ^= 1;
  if (ipa_tracks_host_coef(st, K)) {
    sc X, XI;
    host_sc_from(X, x); host_sc_from(XI, xinv);
    std::vector<sc> ng(2 * K), nh(2 * K);
    for (u32 j = 0; j < 2 * K; j++) {
      sc_mul(ng[j], st->hcg[j >> 1], (j & 1u) ? X : XI);
      sc_mul(nh[j], st->hch[j >> 1], (j & 1u) ? XI : X);
    }
    st->hcg.swap(ng); st->hch.swap(nh);
  }
  st->d += 1;
  st->n = np;
  st->lr_done = false;
}

// the folded generators (g2, h2: st->n points each) become the new bases, the coefficient tables [1] again
static int ipa_adopt_folded(bpmi_ipa *st, bool sync) {
  bpmi_ctx *ctx = st->ctx;
  std::swap(st->g, st->g2);
  std::swap(st->h, st->h2);
  st->M = st->n;
  st->d = 0;
  static const uint8_t one[32] = {1};
  HIPCHK(ctx, h2d(ctx, st->cg[st->cur], one, 32, ctx->stream));
  HIPCHK(ctx, h2d(ctx, st->ch[st->cur], one, 32, ctx->stream));
  if (sync) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  ipa_host_coef_one(st);
  return BPMI_OK;
}

// The workspace of the 16-way fold's width-4 ladders in ctx->fold_tab:
//   tab_a | tab_b (3P, 5P, 7P of every base point) | scr | digit table a | digit table b | tabx_a | tabx_b (the beta x column, GLV only)
// tab_a == nullptr: there is none (option fold_wnaf off, fewer than 256 points, or no memory) and the plain NAF ladder folds
struct FoldTab { u32 *tab_a, *tab_b, *scr, *tabx_a, *tabx_b; char *dw; size_t wn_bytes; uint64_t nthr; bool glv; };
static int ipa_fold_tab(bpmi_ipa *st, FoldTab &T) {
  bpmi_ctx *ctx = st->ctx;
  const uint64_t npts = st->M;
  // width-4 NAF over affine tables of 3P, 5P, 7P: 2 x 216 B + 2 x 432 B of scratch per base point (1.4 GB at 2^20), allocated
  // HERE, when a fold is actually reached, and kept by the ctx for the next proof (round 3 allocated them with every state,
  // folded or not); if they do not fit the fold uses the plain NAF ladder
  void *wtab = nullptr;
  const uint64_t nthr = (npts + ODDMUL_PER_THREAD - 1) / ODDMUL_PER_THREAD;
  const bool glv = ctx->opt_fold_wnaf >= 2 && st->n % 64 == 0;          // k_ec_multifold_w4g reads its digits per WAVE: a wave must not straddle g and h
  const size_t tab_bytes = align_up(3ull * npts * 72, 256), scr_bytes = align_up(2ull * nthr * ODDMUL_PER_THREAD * 3 * 144, 256),
               wn_bytes = align_up(glv ? sizeof(WnafG) : sizeof(WnafK), 256), tabx_bytes = glv ? align_up(4ull * npts * 36, 256) : 0;
  if (ctx->opt_fold_wnaf && npts >= 256) {
    const size_t need = 2 * tab_bytes + scr_bytes + 2 * wn_bytes + 2 * tabx_bytes;
    if (need > ctx->fold_tab_bytes) {
      ctx->fold_key_g = ctx->fold_key_h = nullptr;
      if (ctx->fold_tab) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(ctx->fold_tab); ctx->fold_tab = nullptr; ctx->fold_tab_bytes = 0; }
      if (hipMalloc(&ctx->fold_tab, need) == hipSuccess) ctx->fold_tab_bytes = need; else { (void)hipGetLastError(); ctx->fold_tab = nullptr; }
    }
    wtab = ctx->fold_tab;
  }
  T.tab_a = (u32 *)wtab; T.nthr = nthr; T.glv = glv; T.wn_bytes = wn_bytes;
  if (!wtab) return BPMI_OK;
  T.tab_b = (u32 *)((char *)wtab + tab_bytes); T.scr = (u32 *)((char *)wtab + 2 * tab_bytes);
  T.dw = (char *)wtab + 2 * tab_bytes + scr_bytes;
  T.tabx_a = (u32 *)(T.dw + 2 * wn_bytes); T.tabx_b = (u32 *)(T.dw + 2 * wn_bytes + tabx_bytes);
  return BPMI_OK;
}

// the three engines of the 16-way fold: out[i] = sum_t coef[t] * base[i + t*m] for g (ja) and h (jb) in one launch
// width-4 NAF of the coefficients' GLV halves, as the ladder's operation list (fold_ops_host.hpp)
static int ipa_ladder_w4g(bpmi_ipa *st, const FoldTab &T, MultifoldJob ja, MultifoldJob jb) {
  bpmi_ctx *ctx = st->ctx;
  const u32 K2 = 1u << st->d;
  const uint64_t npts = st->M, nthr = T.nthr;
  char *dw = T.dw;
  const size_t wn_bytes = T.wn_bytes;
  static thread_local WnafG hga, hgb;
  if (!glv_fold_ops(hga, st->hcg.data(), K2) || !glv_fold_ops(hgb, st->hch.data(), K2))
    return fail(ctx, BPMI_E_STATE, "fold: operation list overflow");
  HIPCHK(ctx, h2d(ctx, dw, &hga, sizeof(WnafG), ctx->stream));
  HIPCHK(ctx, h2d(ctx, dw + wn_bytes, &hgb, sizeof(WnafG), ctx->stream));
  StageTimer t(ctx, ST_LINCOMB2);
  // Option ipa_fixed_generators: the generators of a deployment are constants, and so are the tables of their odd multiples
  // (3P, 5P, 7P and the beta x column: 1.1 ms of k_ec_odd_multiples at 2^20).  They are kept between proofs that name the SAME
  // caller arrays (bpmi_ipa_create_dev: d_g, d_h, n) -- the caller's promise that the arrays have not changed.
  // Only a fold whose input IS the caller's unfolded arrays (the first one: M == n0) may keep or reuse tables: a second 16-way fold (n0 >= 16
  // big_m) runs over the already folded, challenge-dependent bases, and tables recorded under (src_g, src_h, n0 / 16) would be served to a later
  // proof over a PREFIX of the same generator arrays.
  const bool from_source = ctx->opt_ipa_fixed && st->src_g && !st->hscale && st->M == st->n0;
  const bool kept = from_source && ctx->fold_key_g == st->src_g && ctx->fold_key_h == st->src_h && ctx->fold_key_n == npts;
  if (!kept) {
    hipLaunchKernelGGL(k_ec_odd_multiples<ODDMUL_PER_THREAD>, dim3((u32)((2 * nthr + 255) / 256)), dim3(256), 0, ctx->stream, st->g, st->h, (u32)npts, T.tab_a, T.tab_b, T.scr,
                       T.tabx_a, T.tabx_b);
    if (from_source) { ctx->fold_key_g = st->src_g; ctx->fold_key_h = st->src_h; ctx->fold_key_n = npts; }
    else ctx->fold_key_g = ctx->fold_key_h = nullptr;
  }
  hipLaunchKernelGGL(k_ec_multifold_w4g, dim3((u32)((2 * st->n + 255) / 256)), dim3(256), 0, ctx->stream, ja, jb, T.tab_a, T.tab_b, T.tabx_a, T.tabx_b,
                     (const WnafG *)dw, (const WnafG *)(dw + wn_bytes), (u32)st->n, K2);
  return BPMI_OK;
}
// width-4 NAF of the whole coefficients
static int ipa_ladder_w4(bpmi_ipa *st, const FoldTab &T, MultifoldJob ja, MultifoldJob jb) {
  bpmi_ctx *ctx = st->ctx;
  const u32 K2 = 1u << st->d;
  const uint64_t npts = st->M, nthr = T.nthr;
  WnafK *dwa = (WnafK *)T.dw, *dwb = (WnafK *)(T.dw + T.wn_bytes);
  static thread_local WnafK hwa, hwb;
  wnaf_fold_table(hwa, st->hcg.data(), K2);
  wnaf_fold_table(hwb, st->hch.data(), K2);
  HIPCHK(ctx, h2d(ctx, dwa, &hwa, sizeof(WnafK), ctx->stream));
  HIPCHK(ctx, h2d(ctx, dwb, &hwb, sizeof(WnafK), ctx->stream));
  StageTimer t(ctx, ST_LINCOMB2);
  ctx->fold_key_g = ctx->fold_key_h = nullptr;
  hipLaunchKernelGGL(k_ec_odd_multiples<ODDMUL_PER_THREAD>, dim3((u32)((2 * nthr + 255) / 256)), dim3(256), 0, ctx->stream, st->g, st->h, (u32)npts, T.tab_a, T.tab_b, T.scr,
                     (u32 *)nullptr, (u32 *)nullptr);
  hipLaunchKernelGGL(k_ec_multifold_w4, dim3((u32)((2 * st->n + 255) / 256)), dim3(256), 0, ctx->stream, ja, jb, T.tab_a, T.tab_b, dwa, dwb, (u32)st->n, K2);
  return BPMI_OK;
}
// plain NAF, no workspace
static int ipa_ladder_naf(bpmi_ipa *st, MultifoldJob ja, MultifoldJob jb) {
  bpmi_ctx *ctx = st->ctx;
  const u32 K2 = 1u << st->d;
  NafK ha, hb;
  naf_fold_table(ha, st->hcg.data(), K2);
  naf_fold_table(hb, st->hch.data(), K2);
  HIPCHK(ctx, h2d(ctx, st->nafk[0], &ha, sizeof(NafK), ctx->stream));
  HIPCHK(ctx, h2d(ctx, st->nafk[1], &hb, sizeof(NafK), ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));     // ha / hb are stack objects
  StageTimer t(ctx, ST_LINCOMB2);
  hipLaunchKernelGGL(k_ec_multifold, dim3((u32)((2 * st->n + 255) / 256)), dim3(256), 0, ctx->stream, ja, jb, st->nafk[0], st->nafk[1], (u32)st->n, K2);
  return BPMI_OK;
}
// materialise the 16-way folded generators
static int ipa_fold_ladder16(bpmi_ipa *st) {
  bpmi_ctx *ctx = st->ctx;
  MultifoldJob ja = {st->g, st->g2}, jb = {st->h, st->h2};
  FoldTab T;
  int rc = ipa_fold_tab(st, T);
  if (rc) return rc;
  if (T.tab_a) {
    rc = T.glv ? ipa_ladder_w4g(st, T, ja, jb) : ipa_ladder_w4(st, T, ja, jb);
    if (rc) return rc;
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));     // the host digit tables are thread-local statics
  } else {
    rc = ipa_ladder_naf(st, ja, jb);
    if (rc) return rc;
  }
  HIPCHK(ctx, hipGetLastError());
  return ipa_adopt_folded(st, true);
}

// the two engines of the product fold (point_kernels.hpp): out[i] = sum_t coef[t] (hscale) base[i + t m] with one thread per TERM
static int ipa_products_glv(bpmi_ipa *st, u32 K) {
  bpmi_ctx *ctx = st->ctx;
  const uint64_t m = st->n;
  static thread_local GlvFoldK hk;
  glv_fold_table(hk, st->hcg.data(), st->hch.data(), K);
  const u32 G = K / GLVF_TERMS;
  const size_t o_part = align_up(sizeof(GlvFoldK), 256);
  int rc = ensure_stage_in(ctx, o_part + 4ull * XYZZ_WORDS * 2 * G * m + 512);
  if (rc) return rc;
  char *buf = (char *)ctx->stage_in;
  HIPCHK(ctx, h2d(ctx, buf, &hk, sizeof(hk), ctx->stream));
  {
    StageTimer t(ctx, ST_LINCOMB2);
    hipLaunchKernelGGL(k_ec_fold_glv, dim3((u32)((2ull * G * m + 255) / 256)), dim3(256), 0, ctx->stream, st->g, st->h, (u32)m, K, (const GlvFoldK *)buf,
                       (u32 *)(buf + o_part));
    hipLaunchKernelGGL(k_ec_sum_partials, dim3((u32)((2 * m + 255) / 256)), dim3(256), 0, ctx->stream, (const u32 *)(buf + o_part), (u32)m, G, st->g2, st->h2);
  }
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));          // the digit table is a thread-local static
  return BPMI_OK;
}
// per-lane products: the coefficients (and hscale) expanded to one scalar per base point, multiplied out, summed per output
static int ipa_products_per_lane(bpmi_ipa *st, u32 K) {
  bpmi_ctx *ctx = st->ctx;
  const uint64_t M = st->M, m = st->n;
  const u32 logm = ipa_log2(m);
  const size_t o_sc = align_up(128 * M, 256), o_pr = o_sc + align_up(64 * M, 256);
  int rc = ensure_stage_in(ctx, o_pr + 128 * M + 512);
  if (rc) return rc;
  char *buf = (char *)ctx->stage_in;
  u32 *d_pts = (u32 *)buf, *d_sc = (u32 *)(buf + o_sc), *d_prod = (u32 *)(buf + o_pr);
  HIPCHK(ctx, hipMemcpyAsync(d_pts, st->g, 64 * M, hipMemcpyDeviceToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d_pts + 16 * M, st->h, 64 * M, hipMemcpyDeviceToDevice, ctx->stream));
  {
    StageTimer t(ctx, ST_SCFOLD);
    hipLaunchKernelGGL(k_ipa_fold_scalars, dim3((u32)((M + 255) / 256)), dim3(256), 0, ctx->stream, st->cg[st->cur], st->ch[st->cur], st->hscale, (u32)M, logm,
                       d_sc, d_sc + 8 * M);
  }
  rc = bpmi_ec_mul_batch_dev(ctx, d_pts, d_sc, 2 * M, d_prod);
  if (rc) return rc;
  {
    StageTimer t(ctx, ST_LINCOMB2);
    hipLaunchKernelGGL(k_ec_sum_strided, dim3((u32)((2 * m + 255) / 256)), dim3(256), 0, ctx->stream, d_prod, (u32)m, K, st->g2, st->h2);
  }
  HIPCHK(ctx, hipGetLastError());
  return BPMI_OK;
}
static int ipa_fold_products(bpmi_ipa *st) {
  const u32 K = (u32)(st->M / st->n);
  const int rc = ipa_products_shared(st, K) ? ipa_products_glv(st, K) : ipa_products_per_lane(st, K);
  if (rc) return rc;
  st->hscale = nullptr;                  // the factors are in the folded generators now
  return ipa_adopt_folded(st, false);
}

int bpmi_ipa_fold(bpmi_ipa *st, const uint8_t x[32], const uint8_t xinv[32]) {
  if (!st || !x || !xinv) return BPMI_E_ARG;
  bpmi_ctx *ctx = st->ctx;
  if (st->n < 2) return fail(ctx, BPMI_E_STATE, "ipa already reduced to length 1");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  st->prep_ready = false;
  if (ipa_small_step_applies(st)) return ipa_small_step(st, x, xinv);
  ipa_fold_vectors(st, x, xinv);
  if (ipa_ladder16_due(st)) return ipa_fold_ladder16(st);
  if (ipa_products_due(st)) return ipa_fold_products(st);
  return BPMI_OK;
}

// The whole halving loop of FastNIProver2.prove (/root/reference/src/innerproduct/inner_product_prover.py:94-110) in ONE call, the
// Fiat-Shamir edge included: per round L, R (bpmi_ipa_round_LR), the transcript items of the two points (base64 of the compressed
// point, '&'), the challenge x = mod_hash(transcript, q) (src/utils/utils.py:84-97), its decimal item, the fold (bpmi_ipa_fold with
// x and 1/x).  Byte for byte what utils/transcript.py builds -- the golden proofs pin it -- without a trip through the interpreter
// per round (20 rounds x ~40 us at n = 2^20).  The sharded prover keeps the round-by-round entry points (it exchanges L and R).
//   digest / digest_len   the transcript so far;  digest_out (capacity cap) receives the transcript after the last round
//   xs, Ls, Rs            32 / 64 / 64 bytes per round (little-endian scalars, 64-byte points), max_rounds entries each
int bpmi_ipa_prove_rounds(bpmi_ipa *st, const uint8_t *digest, uint64_t digest_len, uint8_t *digest_out, uint64_t cap, uint64_t *out_len, uint8_t *xs,
                          uint8_t *Ls, uint8_t *Rs, uint32_t max_rounds, uint32_t *rounds) {
  if (!st || (!digest && digest_len) || !digest_out || !out_len || !xs || !Ls || !Rs || !rounds) return BPMI_E_ARG;
  bpmi_ctx *ctx = st->ctx;
  std::vector<uint8_t> dg(digest, digest + digest_len);
  dg.reserve(digest_len + 256 * 24);
  uint32_t r = 0;
  while (st->n > 1) {
    if (r >= max_rounds) return fail(ctx, BPMI_E_ARG, "more rounds than max_rounds");
    uint8_t *L = Ls + 64 * (size_t)r, *R = Rs + 64 * (size_t)r;
    int rc = bpmi_ipa_round_LR(st, L, R);
    if (rc) return rc;
    rpt::append_point(dg, L);
    rpt::append_point(dg, R);
    rp::Sq x, xi;
    rpt::challenge(x, dg);
    rp::q_inv(xi, x);
    uint8_t xb[32], xib[32];
    rp::q_to_le(xb, x); rp::q_to_le(xib, xi);
    memcpy(xs + 32 * (size_t)r, xb, 32);
    rc = bpmi_ipa_fold(st, xb, xib);
    if (rc) return rc;
    r++;
  }
  if (!rpt::export_digest(dg, digest_out, cap, out_len)) return fail(ctx, BPMI_E_ARG, "digest_out too small");
  *rounds = r;
  return BPMI_OK;
}

int bpmi_ipa_finish(bpmi_ipa *st, uint8_t a[32], uint8_t b[32]) {
  if (!st || !a || !b) return BPMI_E_ARG;
  bpmi_ctx *ctx = st->ctx;
  if (st->n != 1) return fail(ctx, BPMI_E_STATE, "ipa not yet reduced to length 1");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemcpyAsync(a, st->a, 32, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(b, st->b, 32, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return BPMI_OK;
}

#define IPA_EXPORT_MAX 64
int bpmi_ipa_export(bpmi_ipa *st, uint8_t *g, uint8_t *h, uint8_t *a, uint8_t *b) {
  if (!st || !g || !h || !a || !b) return BPMI_E_ARG;
  bpmi_ctx *ctx = st->ctx;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const uint64_t m = st->n;
  HIPCHK(ctx, hipMemcpyAsync(a, st->a, 32 * m, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(b, st->b, 32 * m, hipMemcpyDeviceToHost, ctx->stream));
  if (st->d == 0 && !st->hscale) {
    // the bases are the current generators
    HIPCHK(ctx, hipMemcpyAsync(g, st->g, 64 * m, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(h, st->h, 64 * m, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return BPMI_OK;
  }
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (m > IPA_EXPORT_MAX) return fail(ctx, BPMI_E_STATE, "ipa export with deferred folds needs a current length <= 64");
  st->prep_ready = false;                 // the export's scalars go through the buffers a prepared round would read
  // deferred folds: every current generator is one MSM over the unfolded bases
  const u32 logm = ipa_log2(m);
  for (u32 pos = 0; pos < (u32)m; pos++) {
    {
      StageTimer t(ctx, ST_SCFOLD);
      hipLaunchKernelGGL(k_ipa_export_scalars, dim3((u32)((st->M + 255) / 256)), dim3(256), 0, ctx->stream, st->cg[st->cur],
                         st->ch[st->cur], st->hscale, (u32)st->M, logm, pos, st->eg, st->eh);
    }
    Segs sg = segs_init(), sh = segs_init();
    sg.pts[0] = st->g; sg.sc[0] = st->eg; sg.n[0] = (u32)st->M; sg.total = (u32)st->M;
    sh.pts[0] = st->h; sh.sc[0] = st->eh; sh.n[0] = (u32)st->M; sh.total = (u32)st->M;
    int rc = msm_run_pair(ctx, sg, g + 64 * pos, sh, h + 64 * pos);
    if (rc) return rc;
  }
  return BPMI_OK;
}

void bpmi_ipa_destroy(bpmi_ipa *st) {
  if (!st) return;
  (void)hipSetDevice(st->ctx->device);
  (void)hipStreamSynchronize(st->ctx->stream);
  ipa_free(st);
}

}  // extern "C"
