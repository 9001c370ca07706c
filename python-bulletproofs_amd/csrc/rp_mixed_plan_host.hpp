// rp_mixed_plan_host.hpp -- part of libbpmi; plain C++17 (no HIP, no bpmi_ctx), also compiled for the host by tests/csrc_host.
// The plan of a MIXED batch of range proofs (bpmi_rp_batch_verify_mixed_dev): classes of different (n_gens, values_per_proof) over the
// prefixes of one generator list, verified by ONE MSM.  A pure function of (options, the classes' sizes and offset tables): the argument
// errors, the unchanged rp_prepare_plan of every class, where each class's regions sit inside the two device buffers, its first global
// proof index, its block of the point / scalar arrays, the merged region and the ROUNDS -- round r holds the r-th row chunk
// (RpPlan::rows) of every class that has one; the two chain kernels run once per round over all its units.  tests/test_rp_mixed_plan_cpu.py
// checks it without a GPU; rp_mixed_dev_host.hpp queues what rp_mixed_plan returns.
#pragma once
#include <string>
#include <vector>

#include "rp_batch_plan_host.hpp"

struct RpMixedClass {
  RpPlan pl;                       // the class as a batch of its own: offsets inside its regions
  size_t in_base = 0, buf_base = 0;      // its regions inside ctx->stage_in / ctx->rp_buf (256-byte lines)
  uint64_t first = 0;              // global index of its proof 0 (class-major numbering of the whole call)
  uint64_t nv = 0, npts = 0;       // commitments, proof points
  uint64_t pair_off = 0;           // its block [commitments | proof points] starts at this pair of d_points / d_scalars
  uint64_t v_off = 0;              // its commitments inside the staged commitment array (points)
  u32 chunks = 0;                  // row chunks: ceil(P / rows)
};
struct RpMixedUnit { u32 cls, chunk; };
struct RpMixedRound { u32 first_unit = 0, n_units = 0; size_t lds_bytes = 0; };      // units[first_unit, first_unit + n_units); LDS: the largest of its classes

struct RpMixedPlan {
  int err = 0; std::string msg;    // an argument error: nothing else is set
  u32 n_classes = 0, N = 0;        // N = n_gens_max
  std::vector<RpMixedClass> cls;
  uint64_t n_proofs = 0, n_pairs = 0, n_v = 0;      // of the whole call; n_pairs: pairs of d_points / d_scalars
  // ctx->stage_in: the classes' regions | the staged commitments (one on-curve check over all of them)
  size_t o_vstage = 0, stage_bytes = 0;
  // ctx->rp_buf: the classes' regions | merged scalars | the one bad word | the unit table
  RpRegion merged, bad, units;
  size_t need = 0, pin_bytes = 0;
  std::vector<RpMixedUnit> unit;   // round-major; slot i of the unit table
  std::vector<RpMixedRound> round;
};

static inline RpMixedPlan rp_mixed_error(const std::string &msg) { RpMixedPlan p; p.err = BPMI_E_ARG; p.msg = msg; return p; }

// others_present: every pointer argument of the call besides the classes and the weights (d_gens, d_points, d_scalars, out, first_bad)
static inline RpMixedPlan rp_mixed_plan(const BpmiOptions &o, uint32_t n_classes, const bpmi_rp_class *classes, uint32_t n_gens_max, bool has_weights, bool has_seed,
                                        bool others_present) {
  if (!classes || (!has_weights && !has_seed) || !others_present) return rp_mixed_error("null argument");
  if (n_classes < 1 || n_classes > RP_MIXED_MAX_CLASSES) return rp_mixed_error("n_classes must be in [1, 64]");
  if (n_gens_max < 2 || n_gens_max > 65536) return rp_mixed_error("n_gens_max must be in [2, 65536]");
  RpMixedPlan p;
  p.cls.resize(n_classes);
  RpLayout in, buf;
  uint64_t first = 0, pairs = 0, nv = 0;
  for (u32 c = 0; c < n_classes; c++) {
    const bpmi_rp_class &k = classes[c];
    const std::string who = "class " + std::to_string(c) + ": ";
    if (!k.blobs || !k.blob_off || !k.v_points) return rp_mixed_error(who + "null argument");
    RpMixedClass &m = p.cls[c];
    m.pl = rp_prepare_plan(o, k.n_gens, k.values_per_proof, k.n_proofs, k.blobs, k.blobs_len, k.blob_off, has_weights, 0);
    if (m.pl.err) return rp_mixed_error(who + m.pl.msg);
    if (k.n_gens > n_gens_max) return rp_mixed_error(who + "n_gens exceeds n_gens_max");
    m.in_base = in.add(m.pl.stage_bytes).off;
    m.buf_base = buf.add(m.pl.need).off;
    m.first = first; m.nv = k.n_proofs * k.values_per_proof; m.npts = k.n_proofs * m.pl.per;
    m.pair_off = pairs; m.v_off = nv;
    m.chunks = (m.pl.P + m.pl.rows - 1) / m.pl.rows;
    first += k.n_proofs; pairs += m.nv + m.npts; nv += m.nv;
    if (3 + 2 * (uint64_t)n_gens_max + pairs > (1ull << 23)) return rp_mixed_error("at most 2^23 points in the batch's MSM");
  }
  p.n_classes = n_classes; p.N = n_gens_max;
  p.n_proofs = first; p.n_pairs = pairs; p.n_v = nv;
  p.o_vstage = in.add(64 * (size_t)nv).off;
  p.stage_bytes = align_up(in.end, 256);
  // rounds: the r-th row chunk of every class that has one, classes in order
  u32 max_chunks = 0;
  for (const RpMixedClass &m : p.cls) max_chunks = std::max(max_chunks, m.chunks);
  for (u32 r = 0; r < max_chunks; r++) {
    RpMixedRound rd;
    rd.first_unit = (u32)p.unit.size();
    for (u32 c = 0; c < n_classes; c++)
      if (r < p.cls[c].chunks) { p.unit.push_back(RpMixedUnit{c, r}); rd.n_units++; rd.lds_bytes = std::max(rd.lds_bytes, p.cls[c].pl.lds_bytes); }
    p.round.push_back(rd);
  }
  p.merged = buf.add(32 * (3 + 2 * (size_t)n_gens_max));
  p.bad = buf.add(8);
  p.units = buf.add((size_t)RP_MIXED_UNIT_STRIDE * p.unit.size());
  p.need = buf.end;
  p.pin_bytes = 64;
  for (const RpMixedClass &m : p.cls) p.pin_bytes = std::max(p.pin_bytes, m.pl.pin_bytes);
  return p;
}
