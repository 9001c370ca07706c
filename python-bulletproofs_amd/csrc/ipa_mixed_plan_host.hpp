// ipa_mixed_plan_host.hpp -- part of libbpmi; plain C++17 (no HIP, no bpmi_ctx), also compiled for the host by tests/csrc_host.
// The plan of a batch of inner-product verifications of DIFFERENT lengths over the prefixes of one generator list
// (bpmi_sc_svector_sum_mixed, bpmi_ipa_verify_batch_mixed_dev) as a pure function of the sizes: the argument errors, the order of the
// proofs, the per-proof descriptors, the units of the summing kernel, the layout of the workspace in ctx->stage_in and the pair count
// of the one MSM.  tests/test_ipa_mixed_plan_cpu.py checks it without a GPU; ipa_mixed_host.hpp consumes it.  Kernels:
// ipa_mixed_kernels.hpp over the bodies of svector_mixed.hpp.  The caps and the constants are those of ipa_batch_plan_host.hpp.
//
// Proof p has n_p = 2^k_p elements over g[:n_p], h[:n_p]; n_top = max n_p.  The proofs are sorted by descending k_p (stable), so the
// proofs that cover element i -- those with n_p > i, i.e. k_p >= bitlen(i) -- are the prefix [0, C[bitlen(i)]) of the sorted list,
// C[j] = number of proofs with k_p >= j.
//
// Units.  k_sc_svector_sum_mixed runs one block per UNIT = (element block e of IPAB_THREADS lanes, proof range [p0, p1), slot).  Block
// e covers the elements [256 e, 256 e + 256) and the proofs [0, Cmax(e)), Cmax(e) = C[bitlen(256 e)]; that range is cut into ranges of
// at most per_part proofs.  A lane clips p1 to its own C[bitlen(i)]: only block 0 and blocks of fewer than 64 elements diverge.
// The rule for per_part, one value per call:
//   waves    = sum_p ceil(n_p / 64)                    the (proof, wave of elements) pairs of the call
//   per_part = clamp(ceil(waves / IPAB_SIMDS), 1, B)   about one wave per SIMD where the work allows it
// For a batch of one length this is the per_part of ipa_batch_plan, and every block then has that plan's `parts` units.
// The slot of a unit is its index: its partial sums are 256 values of A, then 256 values of B.  Where every block has one unit and
// there is no scale the kernel writes SA / SB itself (`direct`): no partial sums, no finish.
#pragma once
#include <algorithm>
#include <vector>

#include "ipa_batch_plan_host.hpp"

#define IPAM_DESC_WORDS 4u                     // per proof: table offset in records, k, kl = k / 2, record offset in words
#define IPAM_UNIT_WORDS 4u                     // per unit: element block, p0, p1, slot
#define IPAM_PART_WORDS (16u * IPAB_THREADS)   // per slot: 256 x 8 words of A, then of B

struct IpamDesc { u32 tab_off, k, kl, rec_off; };
struct IpamUnit { u32 block, p0, p1, slot; };

static inline u32 ipam_bitlen(uint64_t i) { u32 b = 0; while (i >> b) b++; return b; }

struct IpamPlan {
  int err = 0; const char *msg = nullptr;      // an argument error: nothing else is set
  u32 K = 0, k_top = 0;                        // n_gens = 2^K; n_top = 2^k_top
  uint64_t n_gens = 0, n_top = 0, n_proofs = 0, n_extra = 0;
  uint64_t work = 0, waves = 0;                // sum n_p; sum ceil(n_p / 64)
  uint64_t tab_entries = 0;                    // of all proofs: sum (2^kl_p + 2^kh_p) records of 64 bytes, packed
  uint64_t rec_words = 0;                      // of all proofs: sum (16 k_p + 24) words, packed -- k_p pairs (x_j, x_j^-1), then a, b, w
  u32 per_part = 0, n_blocks = 0, n_units = 0;
  bool direct = false;
  std::vector<u32> perm;                       // sorted position -> the caller's index
  std::vector<u32> C;                          // K + 2 entries; C[K + 1] = 0
  std::vector<IpamDesc> desc;                  // sorted order
  std::vector<IpamUnit> unit;                  // block-major
  std::vector<u32> block_first;                // n_blocks + 1: the units of block e are [block_first[e], block_first[e + 1])
  // the workspace: byte offsets into ctx->stage_in, every region on a 256-byte line
  //   SA 32 n_top | SB 32 n_top | records 4 rec_words | descriptors 16 B | C table 4 (K + 2) | units 16 n_units |
  //   block index 4 (n_blocks + 1) | tables 64 tab_entries | partial sums 4 IPAM_PART_WORDS n_units (none when direct) |
  //   extra points 64 n_extra | extra scalars 32 n_extra | scale 32 n_top (only when the scale comes from the host: has_scale = 2)
  // records .. block index are uploaded as one piece.
  uint64_t o_sa = 0, o_sb = 0, o_rec = 0, o_desc = 0, o_ctab = 0, o_units = 0, o_blocks = 0, o_tab = 0, o_part = 0, o_expt = 0, o_exsc = 0, o_scale = 0;
  uint64_t b_sa = 0, b_sb = 0, b_rec = 0, b_desc = 0, b_ctab = 0, b_units = 0, b_blocks = 0, b_tab = 0, b_part = 0, b_expt = 0, b_exsc = 0, b_scale = 0;
  uint64_t total_bytes = 0;
  uint64_t msm_pairs = 0;                      // 2 n_top + n_extra: the MSM reads the first n_top generators only
};

static inline IpamPlan ipam_plan_error(const char *msg) { IpamPlan p; p.err = BPMI_E_ARG; p.msg = msg; return p; }

// ks: n_proofs round counts in the caller's order.  n_extra, has_scale: as in ipa_batch_plan.  No option changes the plan today.
static inline IpamPlan ipa_mixed_plan(const BpmiOptions &, uint64_t n_gens, uint64_t n_proofs, const u32 *ks, uint64_t n_extra, int has_scale) {
  u32 K;
  if (!log2_exact(n_gens, K) || K > IPAB_K_MAX) return ipam_plan_error("n_gens must be 2^K, K <= 22");
  if (n_proofs < 1 || n_proofs > IPAB_PROOFS_MAX) return ipam_plan_error("between 1 and 2^16 proofs per call");
  if (!ks) return ipam_plan_error("null argument");
  uint64_t work = 0, waves = 0, tab_entries = 0;
  u32 k_top = 0;
  for (uint64_t p = 0; p < n_proofs; p++) {
    const u32 k = ks[p];
    if (k > K) return ipam_plan_error("every k_p must be at most K (a proof of 2^k_p elements over n_gens = 2^K generators)");
    const u32 kl = k / 2;
    work += 1ull << k; waves += ((1ull << k) + 63) / 64; tab_entries += (1ull << kl) + (1ull << (k - kl));
    if (k > k_top) k_top = k;
  }
  if (work > IPAB_WORK_MAX) return ipam_plan_error("at most 2^32 elements (the sum of the proofs' 2^k_p) per call");
  if (64 * tab_entries > IPAB_TABLE_BYTES_MAX) return ipam_plan_error("the half tables of the batch (64 (2^(k_p/2) + 2^(k_p - k_p/2)) bytes per proof) exceed 1 GiB");
  if (n_extra > IPAB_EXTRA_MAX) return ipam_plan_error("at most 2^22 extra points per call");
  IpamPlan p;
  const u32 B = (u32)n_proofs;
  p.K = K; p.k_top = k_top; p.n_gens = n_gens; p.n_top = 1ull << k_top; p.n_proofs = n_proofs; p.n_extra = n_extra;
  p.work = work; p.waves = waves; p.tab_entries = tab_entries;
  p.perm.resize(B);
  for (u32 s = 0; s < B; s++) p.perm[s] = s;
  std::stable_sort(p.perm.begin(), p.perm.end(), [ks](u32 x, u32 y) { return ks[x] > ks[y]; });
  p.C.assign(K + 2, 0);
  for (u32 s = 0; s < B; s++) p.C[ks[s]]++;
  for (u32 j = K; j-- > 0;) p.C[j] += p.C[j + 1];          // C[j] = proofs with k_p >= j
  p.desc.resize(B);
  u32 off = 0, rec = 0;                                    // (2^16 proofs x 376 words and 2^24 table records fit 32 bits)
  for (u32 s = 0; s < B; s++) {
    const u32 k = ks[p.perm[s]], kl = k / 2;
    p.desc[s] = IpamDesc{off, k, kl, rec};
    off += (1u << kl) + (1u << (k - kl));
    rec += 16u * k + 24u;
  }
  const uint64_t pp = (waves + IPAB_SIMDS - 1) / IPAB_SIMDS;
  p.rec_words = rec;
  p.per_part = (u32)(pp < 1 ? 1 : pp > B ? B : pp);
  p.n_blocks = (u32)((p.n_top + IPAB_THREADS - 1) / IPAB_THREADS);
  p.block_first.resize(p.n_blocks + 1);
  bool one_each = true;
  for (u32 e = 0; e < p.n_blocks; e++) {
    p.block_first[e] = (u32)p.unit.size();
    const u32 cmax = p.C[ipam_bitlen((uint64_t)IPAB_THREADS * e)];       // >= 1: the longest proof covers every block
    for (u32 p0 = 0; p0 < cmax; p0 += p.per_part) {
      const u32 p1 = cmax - p0 < p.per_part ? cmax : p0 + p.per_part;
      p.unit.push_back(IpamUnit{e, p0, p1, (u32)p.unit.size()});
    }
    one_each = one_each && cmax <= p.per_part;
  }
  p.n_units = (u32)p.unit.size();
  p.block_first[p.n_blocks] = p.n_units;
  p.direct = one_each && !has_scale;
  p.b_sa = p.b_sb = 32 * p.n_top;
  p.b_rec = 4ull * p.rec_words;
  p.b_desc = 4ull * IPAM_DESC_WORDS * n_proofs;
  p.b_ctab = 4ull * (K + 2);
  p.b_units = 4ull * IPAM_UNIT_WORDS * p.n_units;
  p.b_blocks = 4ull * (p.n_blocks + 1);
  p.b_tab = 64 * tab_entries;
  p.b_part = p.direct ? 0 : 4ull * IPAM_PART_WORDS * p.n_units;
  p.b_expt = 64 * n_extra; p.b_exsc = 32 * n_extra;
  p.b_scale = has_scale == 2 ? 32 * p.n_top : 0;
  uint64_t at = 0;
  auto take = [&at](uint64_t bytes) { const uint64_t o = at; at += align_up(bytes, 256); return o; };
  p.o_sa = take(p.b_sa); p.o_sb = take(p.b_sb); p.o_rec = take(p.b_rec); p.o_desc = take(p.b_desc); p.o_ctab = take(p.b_ctab);
  p.o_units = take(p.b_units); p.o_blocks = take(p.b_blocks); p.o_tab = take(p.b_tab); p.o_part = take(p.b_part);
  p.o_expt = take(p.b_expt); p.o_exsc = take(p.b_exsc); p.o_scale = take(p.b_scale);
  p.total_bytes = at;
  p.msm_pairs = 2 * p.n_top + n_extra;
  return p;
}
