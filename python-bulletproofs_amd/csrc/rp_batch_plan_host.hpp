// rp_batch_plan_host.hpp -- part of libbpmi; plain C++17 (no HIP, no bpmi_ctx), also compiled for the host by tests/csrc_host.
// The plan of one batch preparation on the device as a pure function of (options, sizes, the caller's offset table): the argument
// errors, the wire format and the bound of its expansion, the layout of the two device buffers, rows per launch, upload slices, the
// launch parameters and the group mode's geometry.  Everything that decides a buffer size or a launch shape on bytes from the
// network is here, where tests/test_rp_plan_cpu.py checks it without a GPU; rp_batch_dev_host.hpp queues what rp_prepare_plan returns.
#pragma once
#include <algorithm>

#include "shared_defs.hpp"

// A buffer is laid out by appending regions: each starts on a 256-byte line, `end` is the end of the last one (not rounded up)
struct RpRegion { size_t off = 0, bytes = 0; };
struct RpLayout {
  size_t end = 0;
  RpRegion add(size_t bytes) { RpRegion r; r.off = align_up(end, 256); r.bytes = bytes; end = r.off + bytes; return r; }
};
struct RpSlice { u32 g0, g1; uint64_t b0, b1; };      // proofs [g0, g1) = bytes [b0, b1) of the blobs
// how the groups' MSMs run (bpmi_rp_batch_group_values_dev): one launch of k_msm_group in its light or its k_msm_mid shape, or msm_run group by group
enum RpGroupRoute { RP_GROUPS_NONE = 0, RP_GROUPS_LIGHT = 1, RP_GROUPS_MID = 2, RP_GROUPS_MSM_RUN = 3 };
// where the proofs' points are decoded: beside the uploads on the second lane (option rp_overlap = 1), or in one launch on the
// ctx stream in front of the row loop (group mode: the verdicts read the point flags) or behind it (rp_prepare_enqueue)
enum RpDecodeAt { RP_DECODE_BESIDE = 0, RP_DECODE_FIRST = 1, RP_DECODE_LAST = 2 };

struct RpPlan {
  int err = 0; const char *msg = nullptr;      // an argument error: nothing else is set
  // shape
  u32 P = 0, m = 0, k = 0, per = 0, ncols = 0, nslots = 0;      // proofs, values per proof, log2 n_gens, points per proof, 5 + 2 n_gens columns, context slots per proof
  uint8_t fmt0 = '1';                                    // the wire format of the call: the first proof's
  bool v2 = false;                                       // format 2 or 3: the device expands the proofs
  u32 rp_prio = 0;
  uint64_t maxlen = 0;                                   // the longest proof (formats 2 / 3: the bound of its expansion)
  u32 W = 0;                                             // rows of 8-byte words of the word-major proof array
  // ctx->stage_in: blobs | offsets | weights | role status
  size_t o_off = 0, o_w = 0, o_st = 0, stage_bytes = 0;
  // ctx->rp_buf
  RpRegion contrib, ctx, shared, T, lens;                // cells of a launch | context slots | summed columns, verdict, MSM scalars | word-major proofs | expanded lengths
  RpRegion gsum, gfin, verdict, ptflag, E, vals;         // group mode only (bytes = 0 without it)
  size_t o_bad = 0, o_fin = 0;                           // inside `shared`: the first bad proof's index, the scalars of the shared generators
  size_t need = 0;
  // launches
  size_t cell_row = 0, out_row = 0;
  u32 rows = 0, lanes = 0, el_log = 0, ranges = 0;       // proofs per launch, proofs per wave, the ElemGeom values
  size_t lds_bytes = 0, pin_bytes = 0;
  u32 nsl = 0;
  RpSlice sl[RP_UPLOAD_SLICES];
  RpDecodeAt decode = RP_DECODE_BESIDE;
  // group mode
  u32 group = 0, ngroups = 0, msm_windows = 0;
  RpGroupRoute route = RP_GROUPS_NONE;
};

// Longest expansion a format-2 (fmt '2') or format-3 ('3') proof of `len` bytes can have.  Its seeds' lengths are NOT read (2^14
// scattered reads of the receive buffer cost more than the upload saves): S seed bytes in all, base64 of them at most three times
// (the Protocol-1 seed appears in two transcripts), every point item 45 bytes, every decimal item 79.  Monotone in len.
static inline uint64_t rp_expansion_bound(uint64_t len, u32 k, uint8_t fmt) {
  const uint64_t hint_bytes = fmt == '3' ? 32ull * (6 + 2 * k) : 0;             // format 3: the points' y coordinates behind the format-2 proof
  const uint64_t body = 6 + 32ull * (5 + k) + 33ull * (6 + 2 * k);
  const uint64_t S = len > body + 132 + hint_bytes ? len - body - 132 - hint_bytes : 0;
  return body + 2 + 12 + 3 * (4 * ((S + 2) / 3) + 1) + 4 * 45 + 3 * 79 + 2 * 79 + 1 + (uint64_t)k * (45 + 45 + 79);
}

struct RpGroupShape { u32 group, ngroups; };      // `group` proofs per group (at most the batch), ngroups of them
static inline RpGroupShape rp_group_shape(uint64_t group, uint64_t n_proofs) {
  RpGroupShape s;
  s.group = (u32)std::min<uint64_t>(group, n_proofs);
  s.ngroups = (u32)((n_proofs + s.group - 1) / s.group);
  return s;
}
// the route of a class by the pairs of a FULL group's MSM, 3 + 2 n + group (m + 6 + 2k)
static inline RpGroupRoute rp_group_route(uint64_t pairs) {
  return pairs <= GROUP_LIGHT_NMAX ? RP_GROUPS_LIGHT : (pairs <= MID_NMAX ? RP_GROUPS_MID : RP_GROUPS_MSM_RUN);
}
// k_rp_group_colsum over the proofs [base, base + cnt): the groups [t0, t0 + nt) have proofs among them; lpg lanes per group, gpb groups per wave
struct RpGroupChunk { u32 t0, nt, lpg, gpb, nblk; };
static inline RpGroupChunk rp_group_chunk(u32 group, u32 base, u32 cnt) {
  RpGroupChunk c;
  c.t0 = base / group; c.nt = (base + cnt - 1) / group - c.t0 + 1;
  c.lpg = 1;
  while (c.lpg < 64u && c.lpg < group) c.lpg <<= 1;
  c.gpb = 64u / c.lpg; c.nblk = (c.nt + c.gpb - 1) / c.gpb;
  return c;
}

static inline RpPlan rp_plan_error(const char *msg) { RpPlan p; p.err = BPMI_E_ARG; p.msg = msg; return p; }

// the argument checks, the offset table (never trusted: a table that decreases or leaves the buffer is refused before a byte of
// `blobs` is read) and the shape
static inline RpPlan rp_plan_shape(const BpmiOptions &o, uint32_t n_gens, uint32_t m, uint64_t n_proofs, const uint8_t *blobs, uint64_t blobs_len,
                                   const uint64_t *blob_off) {
  if (n_gens < 2 || (n_gens & (n_gens - 1)) || n_gens > 65536) return rp_plan_error("n_gens must be a power of two in [2, 65536]");
  if (m < 1 || n_gens % m) return rp_plan_error("values_per_proof must divide n_gens");
  if (n_proofs == 0 || n_proofs > (1ull << 22)) return rp_plan_error("n_proofs must be in [1, 2^22]");
  if (blobs_len > (1ull << 32)) return rp_plan_error("at most 4 GiB of proofs per call");
  if (blob_off[0] > blobs_len) return rp_plan_error("offset table leaves the buffer");
  uint64_t longest = 0;
  for (uint64_t g = 0; g < n_proofs; g++) {
    if (blob_off[g] > blob_off[g + 1] || blob_off[g + 1] > blobs_len) return rp_plan_error("offset table leaves the buffer");
    longest = std::max(longest, blob_off[g + 1] - blob_off[g]);
  }
  RpPlan p;
  (void)log2_exact(n_gens, p.k);
  p.P = (u32)n_proofs; p.m = m; p.ncols = 5 + 2 * n_gens; p.per = 6 + 2 * p.k; p.nslots = CTX_SLOTS(p.k, m);
  // wire format 2 (rp_wire_v2_host.hpp): told by the first proof's magic; every proof of the call must then be format 2 (the device
  // expander refuses the others).  The array the roles read holds the EXPANDED proofs: its rows are sized by the longest expansion
  p.fmt0 = (blob_off[1] >= blob_off[0] + 5 && blob_off[0] + 5 <= blobs_len) ? blobs[blob_off[0] + 4] : (uint8_t)'1';
  p.v2 = p.fmt0 == '2' || p.fmt0 == '3';
  // The expander, the roles and the element kernel are chains of dependent instructions, one wave per SIMD; on formats 1 and 2 they run beside
  // the second lane's square roots (k_ec_decompress_wire: every issue slot it can get).  Raised issue priority lets the chains run at their
  // own speed: format 2 alone 1.71-1.73 -> 1.64-1.68 ms, ten in flight +2.4-2.8 % (two boxes, profiles/r06_C5_preparation_priority_ab.txt);
  // format 3 has no square roots beside it and gains nothing (option "rp_priority": 0 off, 1 = formats 1 and 2 (default), 2 = always)
  p.rp_prio = (o.opt_rp_prio == 2 || (o.opt_rp_prio == 1 && p.fmt0 != '3')) ? 1u : 0u;
  p.maxlen = p.v2 ? rp_expansion_bound(longest, p.k, p.fmt0) : longest;
  // the proofs as 8-byte words, word-major (k_rp_transpose): W rows of P words, 16 rows of zero padding for loads that run past a proof
  p.W = (u32)((std::min<uint64_t>(p.maxlen, RP_MAX_PROOF_BYTES) + 7) / 8) + 16;
  return p;
}

// the two device buffers and the rows per launch
static inline void rp_plan_layout(RpPlan &p, const BpmiOptions &o, uint64_t blobs_len, bool has_weights) {
  const size_t P = p.P, ncols = p.ncols;
  RpLayout in;
  in.add(blobs_len + 128);      // 128 bytes of slack: the kernel's batched 8-byte loads may run past the last proof
  p.o_off = in.add(8 * (P + 1)).off;
  p.o_w = in.add(has_weights ? 128 * P : 0).off;
  p.o_st = in.add(RP_ROLES * P).off;
  p.stage_bytes = align_up(in.end, 256);
  // contributions + contexts: at most ~256 MB of cells per launch
  p.cell_row = 36 * (ncols + p.nslots); p.out_row = 32 * ncols;       // scratch cells are 9 limbs, the result 8 words
  p.rows = (u32)std::min<size_t>(P, std::max<size_t>(1, ((size_t)256 << 20) / p.cell_row));
  if (o.opt_rp_rows > 0) p.rows = std::min<u32>(p.rows, (u32)o.opt_rp_rows);
  RpLayout buf;
  p.contrib = buf.add(36 * ncols * p.rows);
  p.ctx = buf.add(36 * (size_t)p.nslots * p.rows);
  p.shared = buf.add(2 * p.out_row + 256);
  p.T = buf.add(8 * (size_t)p.W * P);
  p.lens = buf.add(4 * P + 256);              // format 2: lengths of the expanded proofs
  p.o_bad = p.shared.off + p.out_row; p.o_fin = p.o_bad + 128;
  if (p.group) {
    const size_t ng = p.ngroups;
    p.gsum = buf.add(32 * ncols * ng);        // ngroups x (5 + 2n) raw column sums
    p.gfin = buf.add(32 * (ncols - 2) * ng);  // the ngroups x (3 + 2n) scalars of the groups' MSMs
    p.verdict = buf.add(P);
    p.ptflag = buf.add(P);
    p.E = buf.add(4ull * XYZZ_WORDS * p.msm_windows * ng);      // the window sums
    p.vals = buf.add(64 * ng + 256);          // the 64-byte values
  }
  p.need = buf.end;
}

// Upload in slices of whole proofs (with the point decoding of a slice beside the upload of the next one).  Format 3's points are
// checked, not computed: 0.02 ms for 2^14 proofs -- nothing to hide behind an upload, and four uploads with their events cost more
// than one: a batch alone 1.63 ms against 1.72
static inline void rp_plan_slices(RpPlan &p, const BpmiOptions &o, uint64_t blobs_len, const uint64_t *blob_off) {
  p.nsl = (p.P >= 4096 && o.opt_rp_overlap) ? (o.opt_rp_slices > 0 ? (u32)o.opt_rp_slices : (p.fmt0 != '3' ? RP_UPLOAD_SLICES : 1u)) : 1u;
  p.nsl = std::min<u32>(p.nsl, RP_UPLOAD_SLICES);      // (bpmi_set_option refuses more)
  for (u32 c = 0; c < p.nsl; c++) {
    RpSlice &s = p.sl[c];
    s.g0 = (u32)((uint64_t)p.P * c / p.nsl); s.g1 = (u32)((uint64_t)p.P * (c + 1) / p.nsl);
    s.b0 = c == 0 ? 0 : blob_off[s.g0]; s.b1 = c + 1 == p.nsl ? blobs_len : blob_off[s.g1];
  }
}

// The whole plan.  group: proofs per group of bpmi_rp_batch_group_values_dev, 0 = the batch as one (no group regions, no group stages)
static inline RpPlan rp_prepare_plan(const BpmiOptions &o, uint32_t n_gens, uint32_t m, uint64_t n_proofs, const uint8_t *blobs, uint64_t blobs_len,
                                     const uint64_t *blob_off, bool has_weights, uint64_t group) {
  RpPlan p = rp_plan_shape(o, n_gens, m, n_proofs, blobs, blobs_len, blob_off);
  if (p.err) return p;
  if (group) {
    const RpGroupShape gs = rp_group_shape(group, n_proofs);
    p.group = gs.group; p.ngroups = gs.ngroups;
    p.msm_windows = 255u / MID_C + 1u;
    const uint64_t pairs = 3 + 2 * (uint64_t)n_gens + (uint64_t)p.group * (m + p.per);          // of a full group
    p.route = rp_group_route(pairs);
  }
  rp_plan_layout(p, o, blobs_len, has_weights);
  rp_plan_slices(p, o, blobs_len, blob_off);
  p.decode = o.opt_rp_overlap ? RP_DECODE_BESIDE : (group ? RP_DECODE_FIRST : RP_DECODE_LAST);
  p.lanes = o.opt_rp_lanes ? (u32)o.opt_rp_lanes : 64u;
  p.lds_bytes = ((size_t)p.k + 1) * 9 * 64 * sizeof(u32);            // role 2: k + 1 prefix products of 9 limbs per lane
  u32 lb = 0;
  while ((1u << lb) < n_gens / m) lb++;
  p.el_log = std::min<u32>(3u, lb);
  p.ranges = n_gens >> p.el_log;
  p.pin_bytes = 32 * (size_t)p.ncols + 64;
  return p;
}
