// rp_prove_host.hpp -- part of libbpmi (included by bpmi.hip; one translation unit).  HOST code.
// The batched range-proof prover's object and launch sequence (kernels: rp_prove_kernels.hpp): bpmi_rp_prover_create builds the
// fixed-base tables of a generator set once; bpmi_rp_prove_batch proves any number of single-value proofs over them, every protocol
// step as one launch over the whole batch, and returns the proofs as wire format 2.
#pragma once

#define PV_SPLIT_MIN 2048u               // a batch of 2 x this many proofs or more runs as two halves on two lanes
struct bpmi_rp_prover {
  bpmi_ctx *ctx = nullptr;
  u32 n = 0, k = 0, nbases = 0;                // n: elements of a proof's vectors = nb m
  u32 NT = 256;                                // threads of a block of the n-lanes-per-proof kernels (rp_prove_plan_host.hpp)
  uint64_t max_proofs = 0;                     // per call (rpp_batch_error)
  u32 nb = 0, m = 1;                           // bits per value, values per proof (m > 1: aggregated proofs)
  u32 *table = nullptr;                        // [(3 + 2n)][wt][bt] affine points
  u32 tw = 16, wt = 16, bt = 32768;            // table windows: tw bits, wt = ceil(256 / tw) per scalar, bt = 2^(tw-1) entries each
  unsigned short *bases = nullptr;             // device: the base lists of every job kind (rpp_class_bases(n, n); rpp_off_*: where each starts)
  unsigned short *mixed_bases = nullptr;       // device: the base lists of every class of this capacity (bpmi_rp_prove_batch_mixed: made by its first call)
  rpp::sc x_ip;                                // mod_hash(b"&", q): the Protocol-1 challenge of an empty seed (the same for every proof)
  std::string ip_prefix;                       // "&&" str(x_ip) "&"
  unsigned char *d_ip_prefix = nullptr;
  u32 u_new[16];                               // x_ip u, affine words
  rpp_host::Buffers mem;                       // the batch's device arrays; page-locked staging of the inputs / the proofs
  hipEvent_t ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};      // phase boundaries of a batch, created once with the prover
  hipEvent_t ev_chain[2] = {nullptr, nullptr};                                            // two halves of a batch: the last multi-scalar multiplication of each
  double last_ms[8] = {0};                     // device milliseconds of the last batch: blind+A/S | y,z+T | x+final+P_new | rounds | emit+copy | total
};

namespace rpp_host {

// decimal text of a 256-bit little-endian value
static std::string decimal_of(const uint8_t le[32]) {
  rp::Sq v;
  rp::q_from_le(v, le);
  std::vector<uint8_t> dg;
  rpt::append_decimal(dg, v);
  return std::string((const char *)dg.data(), dg.size() - 1);
}

// The fixed-base tables of nb bases (basepts: nb x 64 bytes on the host), shared by the batched provers: the window bases 2^(tw k) base_b
// by the engine's batched multiplication, then the multiples level by level (rp_prove_kernels.hpp).  *d_base <- the bases in device
// memory with `tail` spare bytes behind them (the caller's, to free); *table <- [nb][wt][bt] affine points (the caller's).  fn: the
// entry point's name, for the messages.  On an error both may be set: the caller frees them as on success.
static int build_tables(bpmi_ctx *ctx, const char *fn, const std::vector<uint8_t> &basepts, u32 nb, size_t tail, u32 tw, u32 wt, u32 bt, u32 **d_base_out, u32 **table) {
  const size_t entries = (size_t)nb * wt * bt;
  const u32 nbk = nb * wt;                           // (base, window) pairs
  u32 *d_base = nullptr, *d_pts = nullptr, *d_sc = nullptr, *d_wb = nullptr;
  hipError_t e = hipMalloc(&d_base, 64 * (size_t)nb + tail);
  *d_base_out = d_base;
  if (e == hipSuccess) e = hipMalloc(&d_pts, 64 * (size_t)nbk);
  if (e == hipSuccess) e = hipMalloc(&d_sc, 32 * (size_t)nbk);
  if (e == hipSuccess) e = hipMalloc(&d_wb, 64 * (size_t)nbk);
  if (e == hipSuccess) e = hipMalloc(table, 64 * entries);
  auto free_tmp = [&]() { if (d_pts) (void)hipFree(d_pts); if (d_sc) (void)hipFree(d_sc); if (d_wb) (void)hipFree(d_wb); };
  if (e != hipSuccess) { free_tmp(); return fail(ctx, BPMI_E_NOMEM, std::string(fn) + ": " + hipGetErrorString(e)); }
  e = hipMemcpyAsync(d_base, basepts.data(), basepts.size(), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);          // (basepts is pageable)
  if (e != hipSuccess) { free_tmp(); return fail(ctx, BPMI_E_HIP, std::string(fn) + ": " + hipGetErrorString(e)); }
  rpp::Tab T0 = {nullptr, tw, wt, bt};
  hipLaunchKernelGGL(rpp::k_pv_window_scalars, dim3((nbk + 255) / 256), dim3(256), 0, ctx->stream, d_base, nb, T0, d_pts, d_sc);
  int rc = bpmi_ec_mul_batch_dev(ctx, d_pts, d_sc, nbk, d_wb);
  if (rc == BPMI_OK) {
    hipLaunchKernelGGL(rpp::k_pv_table_seed, dim3((nbk + 255) / 256), dim3(256), 0, ctx->stream, d_wb, nbk, T0, *table);
    for (u32 j = 0; j + 1 < tw; j++) {
      const size_t threads = (size_t)nbk << j;
      hipLaunchKernelGGL(rpp::k_pv_table_level, dim3((u32)((threads + 255) / 256)), dim3(256), 0, ctx->stream, nbk, T0, j, *table);
    }
    e = hipGetLastError();
    if (e != hipSuccess) rc = fail(ctx, BPMI_E_HIP, std::string(fn) + ": " + hipGetErrorString(e));
  }
  free_tmp();
  return rc;
}

// ---- what bpmi_rp_prove_batch and bpmi_rp_prove_batch_mixed (rp_prove_mixed_host.hpp) share: a call of the latter is the former's host
// work once per class

// The rpp::Batch of P proofs of shape g whose arrays sit at `at` in the device buffer d.  hs0: the base of hs_0 (3 + the generators the
// tables were built over); p0: the call-wide index of proof 0
static rpp::Batch make_batch(const bpmi_rp_prover *pv, char *d, const RppRegions &at, const RppGeom &g, u32 P, const RppStrides &stride, u32 hs0, u32 p0) {
  rpp::Batch B;
  memset(&B, 0, sizeof(B));
  B.P = P; B.n = g.n; B.k = g.k; B.nb = pv->nb; B.m = g.m; B.hs0 = hs0; B.p0 = p0; B.table = rpp::Tab{pv->table, pv->tw, pv->wt, pv->bt};
  B.dig0 = (const unsigned char *)(d + at.o_dig0); B.dig0_stride = stride.dig0_stride; B.dig0_len = (const u32 *)(d + at.o_dlen);
  B.values = (const u32 *)(d + at.o_val); B.gammas = (const u32 *)(d + at.o_gam);
  B.ip_prefix = pv->d_ip_prefix; B.ip_prefix_len = (u32)pv->ip_prefix.size(); B.x_ip = pv->x_ip;
  memcpy(B.u_new, pv->u_new, 64);
  B.tr = (unsigned char *)(d + at.o_tr); B.tr_stride = stride.tr_stride; B.tr_len = (u32 *)(d + at.o_trlen);
  B.slr = (u32 *)(d + at.o_slr); B.alpha = (u32 *)(d + at.o_alpha); B.chal = (u32 *)(d + at.o_chal); B.tau = (u32 *)(d + at.o_tau); B.tsc = (u32 *)(d + at.o_tsc);
  B.res = (u32 *)(d + at.o_res); B.xs = (u32 *)(d + at.o_xs); B.xr = (u32 *)(d + at.o_xr);
  B.a = (u32 *)(d + at.o_a); B.b = (u32 *)(d + at.o_b); B.cg = (u32 *)(d + at.o_cg); B.hf = (u32 *)(d + at.o_hf);
  B.jsc = (u32 *)(d + at.o_jsc); B.jout = (u32 *)(d + at.o_jout); B.pts = (u32 *)(d + at.o_pts);
  return B;
}

// The inputs of P proofs of m values into the staging buffer hp (zeroed): base64(seed) || '&', which starts every range-proof transcript
// (transcript.py:13-14), with its length; the values and blinding factors; the seeds' bytes at `seeds_at`; and the proofs' rows of the seed
// and output offsets, soff / ooff (row P too: the next class's first, or the call's end).  seed0, out0: where the first seed and the first
// proof sit in the call's seed and output bytes; fixed_bytes: a proof without its seed
static void stage_inputs(char *hp, const RppRegions &at, const RppStrides &stride, u32 m, u32 P, const uint8_t *values, const uint8_t *gammas, const uint8_t *seeds,
                         const uint64_t *seed_off, char *seeds_at, uint64_t *soff, uint64_t *ooff, uint64_t seed0, uint64_t out0, uint64_t fixed_bytes) {
  for (u32 p = 0; p < P; p++) {
    uint8_t *dg = (uint8_t *)hp + at.o_dig0 + (size_t)p * stride.dig0_stride;          // (stride.dig0_stride >= 4 ceil(len / 3) + 1)
    const uint64_t sl = seed_off[p + 1] - seed_off[p];
    size_t tl = rp::b64_encode(dg, seeds + seed_off[p], sl);
    dg[tl++] = '&';
    ((u32 *)(hp + at.o_dlen))[p] = (u32)tl;
    soff[p] = seed0 + (seed_off[p] - seed_off[0]);
    ooff[p] = out0;
    out0 += fixed_bytes + sl;
  }
  soff[P] = seed0 + (seed_off[P] - seed_off[0]);
  ooff[P] = out0;
  memcpy(hp + at.o_val, values, 32ull * P * m);
  memcpy(hp + at.o_gam, gammas, 32ull * P * m);
  if (seed_off[P] > seed_off[0]) memcpy(seeds_at, seeds + seed_off[0], seed_off[P] - seed_off[0]);
}

// The end of a call whose kernels are queued on the prover's stream: the proofs (total_out bytes at d_out) go straight into the caller's
// buffer when it is page-locked (bpmi_host_alloc: what BatchRangeProver hands in), else through the prover's staging buffer and one host
// copy (18 MB for 2^14 64-bit proofs: 2-3 ms of a 27 ms batch); then the phases of bpmi_rp_prover_last_ms.  fn: "entry point: "
static int finish_call(bpmi_rp_prover *pv, const char *fn, const char *d_out, size_t total_out, uint8_t *out) {
  bpmi_ctx *ctx = pv->ctx;
  hipStream_t st = ctx->stream;
  hipEvent_t *ev = pv->ev;
  (void)hipEventRecord(ev[5], st);
  hipError_t e = hipGetLastError();
  bool direct = false;
  {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, out) == hipSuccess && attr.type == hipMemoryTypeHost) direct = true;
    else (void)hipGetLastError();                              // an ordinary host pointer is "invalid value" to the query
  }
  if (e == hipSuccess) e = hipMemcpyAsync(direct ? (void *)out : pv->mem.pin, d_out, total_out, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipEventRecord(ev[6], st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail(ctx, BPMI_E_HIP, std::string(fn) + hipGetErrorString(e));
  if (!direct) memcpy(out, pv->mem.pin, total_out);
  for (int i = 0; i < 6; i++) { float ms = 0; (void)hipEventElapsedTime(&ms, ev[i], ev[i + 1]); pv->last_ms[i] = ms; }
  { float ms = 0; (void)hipEventElapsedTime(&ms, ev[0], ev[6]); pv->last_ms[6] = ms; }
  return BPMI_OK;
}

}  // namespace rpp_host

extern "C" {

void bpmi_rp_prover_destroy(bpmi_rp_prover *pv) {
  if (!pv) return;
  if (pv->ctx) { (void)hipSetDevice(pv->ctx->device); (void)hipStreamSynchronize(pv->ctx->stream); }
  if (pv->table) (void)hipFree(pv->table);
  if (pv->bases) (void)hipFree(pv->bases);
  if (pv->mixed_bases) (void)hipFree(pv->mixed_bases);
  if (pv->d_ip_prefix) (void)hipFree(pv->d_ip_prefix);
  pv->mem.release();
  for (auto e : pv->ev) if (e) (void)hipEventDestroy(e);
  for (auto e : pv->ev_chain) if (e) (void)hipEventDestroy(e);
  delete pv;
}

static int rp_prover_create_impl(bpmi_ctx *ctx, uint32_t vbits, uint32_t m, const uint8_t g[64], const uint8_t h[64], const uint8_t u[64], const uint8_t *gs, const uint8_t *hs,
                                 bpmi_rp_prover **out, bpmi_rp_prover *&partial);
int bpmi_rp_prover_create_aggregated(bpmi_ctx *ctx, uint32_t nbits, uint32_t m, const uint8_t g[64], const uint8_t h[64], const uint8_t u[64], const uint8_t *gs,
                                     const uint8_t *hs, bpmi_rp_prover **out) {
  bpmi_rp_prover *partial = nullptr;
  return rpp_host::guarded(ctx, "bpmi_rp_prover_create", [&] { return rp_prover_create_impl(ctx, nbits, m, g, h, u, gs, hs, out, partial); },
                           [&] { if (partial) bpmi_rp_prover_destroy(partial); if (out) *out = nullptr; });
}
int bpmi_rp_prover_create(bpmi_ctx *ctx, uint32_t nbits, const uint8_t g[64], const uint8_t h[64], const uint8_t u[64], const uint8_t *gs, const uint8_t *hs,
                          bpmi_rp_prover **out) {
  return bpmi_rp_prover_create_aggregated(ctx, nbits, 1, g, h, u, gs, hs, out);
}
static int rp_prover_create_impl(bpmi_ctx *ctx, uint32_t vbits, uint32_t m, const uint8_t g[64], const uint8_t h[64], const uint8_t u[64], const uint8_t *gs, const uint8_t *hs,
                                 bpmi_rp_prover **out, bpmi_rp_prover *&partial) {
  if (!ctx || !g || !h || !u || !gs || !hs || !out) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  *out = nullptr;
  const RppPlan plan = rpp_plan(vbits, m, ctx->opt_prover_tw);        // (option "prover_table_bits" is read HERE)
  if (plan.err) return fail(ctx, plan.err, plan.msg);
  const uint32_t nbits = plan.n;                         // elements of a proof's vectors
  HIPCHK(ctx, hipSetDevice(ctx->device));
  {
    const PointCheck pc(ctx, "bpmi_rp_prover_create", ctx->stream, ctx->opt_validate >= 1);
    int vrc = pc.host(g, 1, "g");
    if (!vrc) vrc = pc.host(h, 1, "h");
    if (!vrc) vrc = pc.host(u, 1, "u");
    if (!vrc) vrc = pc.host(gs, nbits, "gs");
    if (!vrc) vrc = pc.host(hs, nbits, "hs");
    if (vrc) return vrc;
  }
  bpmi_rp_prover *pv = new bpmi_rp_prover();
  partial = pv;
  pv->ctx = ctx; pv->n = nbits; pv->nb = vbits; pv->m = m; pv->k = plan.k;
  pv->NT = plan.NT; pv->max_proofs = plan.max_proofs;
  const u32 n = nbits, nb = plan.nbases;
  pv->nbases = nb;
  auto bail = [&](int rc) { bpmi_rp_prover_destroy(pv); partial = nullptr; return rc; };
  for (int i = 0; i < 7; i++) { hipError_t ee = hipEventCreate(&pv->ev[i]); if (ee != hipSuccess) return bail(fail(ctx, BPMI_E_HIP, std::string("bpmi_rp_prover_create: ") + hipGetErrorString(ee))); }
  for (int i = 0; i < 2; i++) { hipError_t ee = hipEventCreateWithFlags(&pv->ev_chain[i], hipEventDisableTiming); if (ee != hipSuccess) return bail(fail(ctx, BPMI_E_HIP, std::string("bpmi_rp_prover_create: ") + hipGetErrorString(ee))); }
  // the Protocol-1 challenge of the empty seed: transcript b"&" (inner_product_prover.py:33; transcript.py:13-14)
  {
    const uint8_t amp = '&';
    rp::Sha one;
    rp::sha_init(one);
    rp::sha_update(one, (const uint8_t *)"1", 1);
    rp::sha_update(one, &amp, 1);
    rp::Sq x;
    rp::mod_hash_q(x, one, &amp, 1);
    uint8_t le[32];
    rp::q_to_le(le, x);
    memcpy(pv->x_ip.v, le, 32);
    pv->ip_prefix = "&&" + rpp_host::decimal_of(le) + "&";
  }
  // points of the bases, the table's inputs and the table: entry (b, k, d) = d 2^(8k) base_b by the engine's batched multiplication
  // table windows (ctx option "prover_table_bits"; the default by size: rpp_default_table_bits): wider windows are fewer additions per term and a larger table
  // (measured at 2^14 64-bit proofs, profiles/r05_batch_prover_table_bits.txt: 8 bits 36.0 ms / 34 MB / 16 ms to build, 10: 31.0 / 112 / 29,
  // 11: 29.3 / 206 / 44, 12: 28.1 / 378 / 72, 13: 26.6 / 687 / 126 with round 5's builder; round 6's builder and 14 .. 16 bits:
  // profiles/r06_batch_prover_table_bits.txt)
  pv->tw = plan.tw; pv->wt = plan.wt; pv->bt = plan.bt;
  std::vector<uint8_t> basepts(64 * (size_t)nb);
  memcpy(&basepts[0], g, 64); memcpy(&basepts[64], h, 64); memcpy(&basepts[128], u, 64);
  memcpy(&basepts[192], gs, 64 * (size_t)n); memcpy(&basepts[192 + 64 * (size_t)n], hs, 64 * (size_t)n);
  u32 *d_base = nullptr;                             // the bases, and 96 bytes for x_ip and u_new
  hipError_t e = hipSuccess;
  int rc = rpp_host::build_tables(ctx, "bpmi_rp_prover_create", basepts, nb, 96, pv->tw, pv->wt, pv->bt, &d_base, &pv->table);
  auto free_tmp = [&]() { if (d_base) (void)hipFree(d_base); };
  // u_new = x_ip u
  if (rc == BPMI_OK) {
    e = hipMemcpyAsync((char *)d_base + 64 * (size_t)nb, pv->x_ip.v, 32, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) rc = fail(ctx, BPMI_E_HIP, hipGetErrorString(e));
  }
  if (rc == BPMI_OK) rc = bpmi_ec_mul_batch_dev(ctx, (char *)d_base + 128, (char *)d_base + 64 * (size_t)nb, 1, (char *)d_base + 64 * (size_t)nb + 32);
  if (rc == BPMI_OK) {
    e = hipMemcpyAsync(pv->u_new, (char *)d_base + 64 * (size_t)nb + 32, 64, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) rc = fail(ctx, BPMI_E_HIP, hipGetErrorString(e));
  }
  free_tmp();
  if (rc) return bail(rc);
  // the base lists of every job kind (rpp_plan)
  const std::vector<unsigned short> &bl = plan.bases;
  e = hipMalloc(&pv->bases, 2 * bl.size());
  if (e == hipSuccess) e = hipMemcpy(pv->bases, bl.data(), 2 * bl.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc(&pv->d_ip_prefix, pv->ip_prefix.size() + 16);
  if (e == hipSuccess) e = hipMemcpy(pv->d_ip_prefix, pv->ip_prefix.data(), pv->ip_prefix.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) return bail(fail(ctx, BPMI_E_HIP, std::string("bpmi_rp_prover_create: ") + hipGetErrorString(e)));
  *out = pv;
  partial = nullptr;
  return BPMI_OK;
}

uint64_t bpmi_rp_prove_batch_proof_bytes(const bpmi_rp_prover *pv, uint64_t seed_len) {
  if (!pv) return 0;
  return rpp_fixed_bytes(pv->k, pv->ctx->opt_prover_wire) + seed_len;
}

static int rp_prove_batch_impl(bpmi_rp_prover *pv, uint64_t n_proofs, const uint8_t *values, const uint8_t *gammas, const uint8_t *seeds, const uint64_t *seed_off,
                               uint8_t *out, uint64_t cap, uint64_t *out_off) {
  if (!pv) return BPMI_E_ARG;
  bpmi_ctx *ctx = pv->ctx;
  if (!values || !gammas || !seed_off || !out || !out_off) return fail(ctx, BPMI_E_ARG, "null argument");
  if (n_proofs == 0) { out_off[0] = 0; return BPMI_OK; }
  // the per-call caps come first: nothing of a batch beyond them is read or allocated
  if (const char *over = rpp_batch_error(pv->max_proofs, n_proofs)) return fail(ctx, BPMI_E_ARG, over);
  if (!seeds && seed_off[n_proofs] != seed_off[0]) return fail(ctx, BPMI_E_ARG, "null argument");
  if (const std::string bad = rpp_host::unreduced({{"values", values, n_proofs * pv->m}, {"gammas", gammas, n_proofs * pv->m}}); !bad.empty())
    return fail(ctx, BPMI_E_ARG, "bpmi_rp_prove_batch: " + bad);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const RppGeom g = rpp_geom(pv->nb, pv->m);
  const u32 P = (u32)n_proofs, n = g.n, k = g.k, npt = g.npt;
  const int wire_fmt = ctx->opt_prover_wire;                  // 2, or 3: with the points' y coordinates (bpmi_rp_prove_batch_proof_bytes counts them)
  // the proofs' seeds: base64(seed) || '&' starts every range-proof transcript (transcript.py:13-14)
  uint64_t max_seed = 0, total_out = 0;
  for (u32 p = 0; p < P; p++) {
    if (seed_off[p + 1] < seed_off[p]) return fail(ctx, BPMI_E_ARG, "seed offsets must not decrease");
    const uint64_t sl = seed_off[p + 1] - seed_off[p];
    if (sl > 0xFFFF) return fail(ctx, BPMI_E_ARG, "a seed is longer than 65535 bytes");
    max_seed = std::max(max_seed, sl);
    out_off[p] = total_out;
    total_out += bpmi_rp_prove_batch_proof_bytes(pv, sl);
  }
  out_off[P] = total_out;
  if (total_out > cap) return fail(ctx, BPMI_E_ARG, "the output buffer is too small (bpmi_rp_prove_batch_proof_bytes per proof)");
  const RppLayout L = rpp_layout(g, P, seed_off[P] - seed_off[0], max_seed, total_out, pv->ip_prefix.size());
  if (int rc = pv->mem.grow(ctx, L.need, std::max(L.in_bytes, (size_t)total_out))) return rc;        // (the output half is only used when `out` is pageable)
  char *d = (char *)pv->mem.buf, *hp = (char *)pv->mem.pin;
  memset(hp, 0, L.in_bytes);
  rpp_host::stage_inputs(hp, L, L, g.m, P, values, gammas, seeds, seed_off, hp + L.o_seeds, (uint64_t *)(hp + L.o_soff), (uint64_t *)(hp + L.o_ooff), 0, 0,
                         rpp_fixed_bytes(k, wire_fmt));
  hipStream_t st = ctx->stream;
  HIPCHK(ctx, hipMemcpyAsync(d, hp, L.in_bytes, hipMemcpyHostToDevice, st));
  const rpp::Batch B = rpp_host::make_batch(pv, d, L, g, P, L, 3 + n, 0);
  const u32 dig0_stride = L.dig0_stride, tr_stride = L.tr_stride;
  hipEvent_t *ev = pv->ev;
  auto blocks = [](uint64_t threads, u32 per) { return dim3((u32)((threads + per - 1) / per)); };
  // Round 6 experiment (option "prover_split", off): a large batch as TWO halves on the ctx's two lanes.  Between two multi-scalar
  // multiplications a half is a chain of one-lane-per-proof kernels (transcript hash, inversion: a quarter of the SIMDs busy) and short vector
  // kernels, 0.45 ms of a 2.3 ms round, which the other half's additions could hide.  Measured twice -- the halves free-running, and their
  // multiplications alternating through events (the form below) -- 19.2-19.4 ms per 2^14 proofs either way against 19.1-19.2 unsplit
  // (profiles/r06_batch_prover_table_bits.txt): the chains' instructions are issue slots the additions lose.
  struct Half { rpp::Batch H; hipStream_t st; u32 p0; bool rec; };
  auto make_half = [&](u32 p0, u32 cnt, hipStream_t hs, bool rec) {
    Half h;
    h.H = B; h.st = hs; h.p0 = p0; h.rec = rec;
    rpp::Batch &H = h.H;
    H.P = cnt;
    H.dig0 += (size_t)p0 * dig0_stride; H.dig0_len += p0;
    H.values += 8ull * p0 * pv->m; H.gammas += 8ull * p0 * pv->m;
    H.tr += (size_t)p0 * tr_stride; H.tr_len += p0;
    H.slr += 8ull * p0 * (2 * n + 1); H.alpha += 8ull * p0; H.chal += 32ull * p0; H.tau += 16ull * p0; H.tsc += 32ull * p0;
    H.res += 40ull * p0; H.xs += 8ull * p0 * k; H.xr += 16ull * p0;
    H.a += 8ull * p0 * n; H.b += 8ull * p0 * n; H.cg += 8ull * p0 * n; H.hf += 8ull * p0 * n;
    H.jsc += 8ull * p0 * (2 * n + 2); H.jout += 36ull * 2 * p0; H.pts += 16ull * p0 * npt;
    return h;
  };
  // step s of a half: 0 A and S; 1 y, z, T1, T2; 2 x, the vectors, P_new; 3 .. 2 + k the rounds; 3 + k the wire bytes.  Every step is
  // [kernels before] [ONE multi-scalar multiplication] [kernels behind]; with two halves (`other` set) the multiplication waits for the other
  // half's previous one and is followed by an event of its own: the additions of the two halves alternate on the chip, and a half's
  // one-lane-per-proof chains (hash, inversion) run beside the OTHER half's additions instead of beside their own twin's.
  const u32 NT = pv->NT, per_block = NT / n;             // proofs per block of the n-lanes-per-proof kernels
  const int job_lanes = ctx->opt_prover_job_lanes;       // 0: by the launch's job count (rpp_job_lanes_log2)
  const u32 nsteps = 4 + k;
  // an n-lanes-per-proof kernel in the instantiation of the prover's block size
#define PV_WIDE(kern, ...)                                                                                                           \
  do {                                                                                                                               \
    const dim3 grid_((Pc + per_block - 1) / per_block);                                                                              \
    if (NT == 256u) hipLaunchKernelGGL(rpp::kern<256>, grid_, dim3(256), 0, hs, __VA_ARGS__);                                        \
    else if (NT == 512u) hipLaunchKernelGGL(rpp::kern<512>, grid_, dim3(512), 0, hs, __VA_ARGS__);                                   \
    else hipLaunchKernelGGL(rpp::kern<1024>, grid_, dim3(1024), 0, hs, __VA_ARGS__);                                                 \
  } while (0)
  auto step = [&](Half &h, u32 sidx, hipEvent_t mine, hipEvent_t other) {
    rpp::Batch &H = h.H;
    hipStream_t hs = h.st;
    const u32 Pc = H.P;
    auto msm = [&](u32 njobs, u32 ntypes, u32 T, u32 base_off, const u32 *scalars, u32 stride, int gl) {
      if (other) (void)hipStreamWaitEvent(hs, other, 0);
      rpp_host::launch_msm(hs, rpp::MsmJobs{njobs, ntypes, T, pv->bases + base_off, scalars, stride, H.jout}, H.table, gl);
      if (mine) (void)hipEventRecord(mine, hs);
    };
    auto affine = [&](u32 count, u32 per, u32 slot0, u32 stp) {
      hipLaunchKernelGGL(rpp::k_pv_affine, blocks(count, 256), dim3(256), 0, hs, (const u32 *)H.jout, count, per, H.pts, npt, slot0, stp);
    };
    if (sidx == 0) {                                     // A, S (rangeproof_prover.py:40-59)
      if (h.rec) (void)hipEventRecord(ev[0], hs);
      hipLaunchKernelGGL(rpp::k_pv_blind, blocks((uint64_t)Pc * (2 * n + 2), 256), dim3(256), 0, hs, H);
      hipLaunchKernelGGL(rpp::k_pv_commit_A, blocks((uint64_t)Pc * 16, 256), dim3(256), 0, hs, H, H.jout);
      affine(Pc, 1, PV_PT_A, 0);
      msm(Pc, 1, 2 * n + 1, rpp_off_S(n), H.slr, 2 * n + 1, rpp_job_lanes_log2(n, Pc, job_lanes));
      affine(Pc, 1, PV_PT_S, 0);
      if (h.rec) (void)hipEventRecord(ev[1], hs);
    } else if (sidx == 1) {                              // y, z, tau1, tau2; t1, t2; T1, T2 (:60-67)
      hipLaunchKernelGGL(rpp::k_pv_chal_yz, blocks(Pc, 64), dim3(64), 0, hs, H);
      PV_WIDE(k_pv_poly, H);
      msm(2 * Pc, 1, 2, rpp_off_T(n), H.tsc, 2, 1);
      affine(2 * Pc, 2, PV_PT_T1, 1);
      if (h.rec) (void)hipEventRecord(ev[2], hs);
    } else if (sidx == 2) {                              // x; l, r, t_hat, taux, mu; P_new (:68-90; inner_product_prover.py:33-37)
      hipLaunchKernelGGL(rpp::k_pv_final_chal, blocks(Pc, 64), dim3(64), 0, hs, H);
      PV_WIDE(k_pv_final_wide, H);
      msm(Pc, 1, 2 * n + 1, rpp_off_P(n), H.jsc, 2 * n + 1, rpp_job_lanes_log2(n, Pc, job_lanes));
      affine(Pc, 1, PV_PT_PNEW, 0);
      if (h.rec) (void)hipEventRecord(ev[3], hs);
      PV_WIDE(k_pv_round_wide, H, 0u, 1u);
    } else if (sidx < 3 + k) {                           // a round of Protocol 2 (inner_product_prover.py:94-110)
      const u32 r = sidx - 3;
      msm(2 * Pc, 2, n + 1, rpp_off_round(n, r), H.jsc, n + 1, rpp_job_lanes_log2(n, 2 * (uint64_t)Pc, job_lanes));
      affine(2 * Pc, 2, 6 + r, k);
      hipLaunchKernelGGL(rpp::k_pv_round_chal, blocks(Pc, 64), dim3(64), 0, hs, H, r);
      PV_WIDE(k_pv_round_wide, H, r, 0u);
    } else {
      if (h.rec) (void)hipEventRecord(ev[4], hs);
      hipLaunchKernelGGL(rpp::k_pv_emit, blocks(Pc, 64), dim3(64), 0, hs, H, (const unsigned char *)(d + L.o_seeds), (const uint64_t *)(d + L.o_soff) + h.p0,
                         (unsigned char *)(d + L.o_out), (const uint64_t *)(d + L.o_ooff) + h.p0, (u32)wire_fmt);
    }
  };
#undef PV_WIDE
  const bool split = ctx->opt_prover_split && P >= 2u * (ctx->opt_prover_split > 1 ? (u32)ctx->opt_prover_split : PV_SPLIT_MIN);
  if (split) {
    int rc = ensure_lane(ctx, 1);
    if (rc) return rc;
    const u32 P0 = (P + 1) / 2;
    HIPCHK(ctx, hipEventRecord(ctx->ev_fork, st));                  // (the inputs are up)
    HIPCHK(ctx, hipStreamWaitEvent(ctx->lane[1].stream, ctx->ev_fork, 0));
    Half ha = make_half(0, P0, st, true), hb = make_half(P0, P - P0, ctx->lane[1].stream, false);
    for (u32 sidx = 0; sidx < nsteps; sidx++) {
      step(ha, sidx, pv->ev_chain[0], sidx ? pv->ev_chain[1] : nullptr);          // (queued alternately: an event is recorded before it is waited for)
      step(hb, sidx, pv->ev_chain[1], pv->ev_chain[0]);
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev_join, ctx->lane[1].stream));
    HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev_join, 0));
  } else {
    Half ha = make_half(0, P, st, true);
    for (u32 sidx = 0; sidx < nsteps; sidx++) step(ha, sidx, nullptr, nullptr);
  }
  return rpp_host::finish_call(pv, "bpmi_rp_prove_batch: ", d + L.o_out, total_out, out);
}
int bpmi_rp_prove_batch(bpmi_rp_prover *pv, uint64_t n_proofs, const uint8_t *values, const uint8_t *gammas, const uint8_t *seeds, const uint64_t *seed_off,
                        uint8_t *out, uint64_t cap, uint64_t *out_off) {
  return rpp_host::guarded(pv ? pv->ctx : nullptr, "bpmi_rp_prove_batch", [&] { return rp_prove_batch_impl(pv, n_proofs, values, gammas, seeds, seed_off, out, cap, out_off); });
}

// out[i] = values[i] g + gammas[i] h from the prover's tables: the pairs laid out as the scalars of count two-term jobs over the base
// list T (g, h: what T1 and T2 run on), k_pv_msm<1>, k_pv_affine.  The prover's device and staging buffers are shared with proving.
static int rp_prover_commit_batch_impl(bpmi_rp_prover *pv, uint64_t count, const uint8_t *values, const uint8_t *gammas, uint8_t *out) {
  if (!pv) return BPMI_E_ARG;
  bpmi_ctx *ctx = pv->ctx;
  if (count == 0) return BPMI_OK;
  if (!values || !gammas || !out) return fail(ctx, BPMI_E_ARG, "null argument");
  if (count > PROVER_COMMIT_MAX) return fail(ctx, BPMI_E_ARG, "at most 2^24 commitments per call");
  if (const std::string bad = rpp_host::unreduced({{"values", values, count}, {"gammas", gammas, count}}); !bad.empty())
    return fail(ctx, BPMI_E_ARG, "bpmi_rp_prover_commit_batch: " + bad);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  using rpp_host::up256;
  const u32 C = (u32)count;
  const size_t o_val = 0, o_gam = up256(32ull * C), in_bytes = o_gam + up256(32ull * C);
  const size_t o_jsc = in_bytes, o_jout = o_jsc + up256(64ull * C), o_pts = o_jout + up256(144ull * C), need = o_pts + up256(64ull * C);
  if (int rc = pv->mem.grow(ctx, need, std::max(in_bytes, (size_t)(64ull * C)))) return rc;
  char *d = (char *)pv->mem.buf, *hp = (char *)pv->mem.pin;
  hipStream_t st = ctx->stream;
  memcpy(hp + o_val, values, 32ull * C);
  memcpy(hp + o_gam, gammas, 32ull * C);
  HIPCHK(ctx, hipMemcpyAsync(d, hp, in_bytes, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(rpp::k_pv_commit_pairs, dim3((2u * C + 255u) / 256u), dim3(256), 0, st, (const u32 *)(d + o_val), (const u32 *)(d + o_gam), C, (u32 *)(d + o_jsc));
  rpp_host::launch_msm(st, rpp::MsmJobs{C, 1, 2, pv->bases + rpp_off_T(pv->n), (const u32 *)(d + o_jsc), 2, (u32 *)(d + o_jout)}, rpp::Tab{pv->table, pv->tw, pv->wt, pv->bt}, 1);
  hipLaunchKernelGGL(rpp::k_pv_affine, dim3((C + 255u) / 256u), dim3(256), 0, st, (const u32 *)(d + o_jout), C, 1u, (u32 *)(d + o_pts), 1u, 0u, 0u);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(hp, d + o_pts, 64ull * C, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail(ctx, BPMI_E_HIP, std::string("bpmi_rp_prover_commit_batch: ") + hipGetErrorString(e));
  memcpy(out, hp, 64ull * C);
  return BPMI_OK;
}
int bpmi_rp_prover_commit_batch(bpmi_rp_prover *pv, uint64_t count, const uint8_t *values, const uint8_t *gammas, uint8_t *out) {
  return rpp_host::guarded(pv ? pv->ctx : nullptr, "bpmi_rp_prover_commit_batch", [&] { return rp_prover_commit_batch_impl(pv, count, values, gammas, out); });
}

int bpmi_rp_prover_last_ms(const bpmi_rp_prover *pv, double ms[7]) {
  if (!pv || !ms) return BPMI_E_ARG;
  for (int i = 0; i < 7; i++) ms[i] = pv->last_ms[i];
  return BPMI_OK;
}

}  // extern "C"
