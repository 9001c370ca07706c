// rp_prove_mixed_kernels.hpp -- part of libbpmi (included by bpmi.hip behind rp_prove_kernels.hpp; one translation unit).  DEVICE code.
// The batched range-proof prover over CLASSES of different sizes in one call (bpmi_rp_prove_batch_mixed, rp_prove_mixed_host.hpp): every
// kernel of rp_prove_kernels.hpp has a `_mixed` twin that runs the SAME per-block body (pv_*_block) for the blocks of every class of a
// step in ONE launch -- the shape of rpd::k_rp_roles_mixed.  A launch reads
//   * a table of units {class, first block}: blocks [first, the next unit's first) are that class's blocks 0 ..; the lookup depends on
//     blockIdx alone, so it is uniform per block and the class record comes in by scalar loads;
//   * a device array with one rpp::Batch per class (slots of RPPM_BATCH_SLOT bytes), and for a multi-scalar multiplication the step's
//     MsmJobs per class: a block's jobs belong to one class, the plan pads every class's job range to whole blocks.
// Between two multiplications a step is a chain of one-lane-per-proof kernels; a call of five classes queued class after class would
// serialise five such chains, here they are one launch each (rp_prove_mixed_plan_host.hpp lists the launches of every step).
#pragma once

namespace rpp {

struct MixedUnit { u32 cls, first; };            // (RppmUnit of the plan)
static_assert(sizeof(Batch) <= RPPM_BATCH_SLOT, "the plan lays the class records out in RPPM_BATCH_SLOT-byte slots (rp_prove_mixed_plan_host.hpp)");
static_assert(sizeof(MsmJobs) == RPPM_JOBS_SLOT, "the plan lays the job records out in RPPM_JOBS_SLOT-byte slots (rp_prove_mixed_plan_host.hpp)");
static_assert(sizeof(MixedUnit) == sizeof(RppmUnit), "the unit table is uploaded as the plan's");
struct MixedTab { const u8 *batches; const MixedUnit *units; u32 n_units; };
// the unit whose blocks hold blockIdx.x: the last one with first <= blockIdx.x (at most 64 units per launch; the firsts ascend from 0)
__device__ __forceinline__ MixedUnit mixed_unit(const MixedTab &M) {
  u32 u = 0;
  while (u + 1 < M.n_units && M.units[u + 1].first <= blockIdx.x) u++;
  return M.units[u];
}
__device__ __forceinline__ const Batch *mixed_batch(const MixedTab &M, u32 cls) { return (const Batch *)(M.batches + (size_t)RPPM_BATCH_SLOT * cls); }

// Two bodies are DUPLICATED here, not shared: as functions of (record, block index) called from k_pv_msm and k_pv_emit they moved those
// kernels' registers (k_pv_msm<1> 164 -> 167 VGPRs, k_pv_emit 36 -> 35), so rp_prove_kernels.hpp keeps both kernels' text as it was and
// the twins run the copies below -- the same statements with `blk` for blockIdx.x.  Change one, change the other.
template <int GL> __device__ __forceinline__ void pv_msm_block(const MsmJobs &J, const Tab &T, const u32 blk) {
  const u32 t = blk * blockDim.x + threadIdx.x;
  const u32 job = t >> GL, l = t & ((1u << GL) - 1u);
  const bool live = job < J.njobs;
  xyzz acc;
  bpmi::xyzz_set_inf(acc);
  if (live) {
    const unsigned short *bl = J.bases + (size_t)(job % J.ntypes) * J.T;
    const u32 Tfull = J.T & ~((1u << GL) - 1u);
    for (u32 term = l; term < Tfull; term += (1u << GL)) {
      sc s = ld_sc(J.scalars + 8ull * ((size_t)job * J.stride + term));
      if (bpmi::sc_is_zero(s)) continue;
      const bool neg = bpmi::sc_is_high(s);
      if (neg) bpmi::sc_neg(s, s);
      const u32 *tb = T.p + 16ull * ((size_t)bl[term] * T.wt * T.bt);
      // window k + 1's entry is requested before window k's addition
      u32 carry = 0;
      u32 wv[16];
      u32 d_cur, sg_cur;
      next_digit(s, T, carry, d_cur, sg_cur);
      ::load_words16(wv, tb + 16ull * (d_cur ? d_cur - 1u : 0u));
      for (u32 k = 0; k < T.wt; k++) {
        affine Pt;
        bpmi::affine_from_words(Pt, wv);
        const u32 d = d_cur, sg = sg_cur;
        if (k + 1u < T.wt) {
          next_digit(s, T, carry, d_cur, sg_cur);
          ::load_words16(wv, tb + 16ull * ((size_t)(k + 1u) * T.bt + (d_cur ? d_cur - 1u : 0u)));
        }
        if (d) bpmi::xyzz_madd_signed(acc, Pt, (sg != 0u) != neg);
      }
    }
    for (u32 term = Tfull; term < J.T; term++) {            // the remainder terms: every lane recodes the scalar, and adds its own windows
      sc s = ld_sc(J.scalars + 8ull * ((size_t)job * J.stride + term));
      if (bpmi::sc_is_zero(s)) continue;
      const bool neg = bpmi::sc_is_high(s);
      if (neg) bpmi::sc_neg(s, s);
      const u32 *tb = T.p + 16ull * ((size_t)bl[term] * T.wt * T.bt);
      // lane l: windows l, l + 2^GL, ...  -- every lane reaches ITS window by a walk of digits (a few instructions each) and all lanes add
      // in the same iteration: an `if (window is mine)` inside ONE loop over the windows made the wave run wt additions with a lane in
      // sixteen active, i.e. exactly the time the fifth term had cost
      u32 carry = 0, walked = 0;
      for (u32 k = l; k < T.wt; k += (1u << GL)) {
        u32 d = 0, sg = 0;
        do { next_digit(s, T, carry, d, sg); walked++; } while (walked <= k);
        affine Pt;
        ::load_affine(Pt, tb + 16ull * ((size_t)k * T.bt + (d ? d - 1u : 0u)));
        if (d) bpmi::xyzz_madd_signed(acc, Pt, (sg != 0u) != neg);
      }
    }
  }
#pragma unroll 1
  for (u32 m = 1; m < (1u << GL); m <<= 1) {
    xyzz o;
    ::xyzz_shfl_xor(o, acc, (int)m);
    bpmi::xyzz_add(acc, acc, o);
  }
  if (live && l == 0) ::xyzz_store_g(J.out + 36ull * job, acc);
}
__device__ __forceinline__ void pv_emit_block(const Batch &B, const u8 *__restrict__ seeds, const u64 *__restrict__ seed_off, u8 *__restrict__ out, const u64 *__restrict__ out_off,
                                              const u32 fmt, const u32 blk) {
  const u32 p = blk * blockDim.x + threadIdx.x;
  if (p >= B.P) return;
  u8 *o = out + out_off[p];
  const u32 k = B.k, npt = 6u + 2u * k;
  u8 *ys = fmt == 3u ? out + out_off[p + 1] - 32u * npt : nullptr;              // format 3: the points' y coordinates end the proof
  o[0] = 'B'; o[1] = 'P'; o[2] = 'R'; o[3] = 'P'; o[4] = (u8)('0' + fmt); o[5] = (u8)k;
  u32 pos = 6;
  for (u32 j = 0; j < 5u; j++) { put_be32(o + pos, ld_sc(B.res + 40ull * p + 8u * j)); pos += 32; }
  for (u32 j = 0; j < k; j++) { put_be32(o + pos, ld_sc(B.xs + 8ull * ((size_t)p * k + j))); pos += 32; }
  const u32 *pt = B.pts + 16ull * (size_t)p * npt;
  for (u32 j = 0; j < npt; j++) {
    u32 w[16];
    if (j == PV_PT_UNEW) { for (int i = 0; i < 16; i++) w[i] = B.u_new[i]; }
    else ::load_words16(w, pt + 16u * j);
    u32 any = 0;
    for (int i = 0; i < 16; i++) any |= w[i];
    if (!any) { for (int i = 0; i < 33; i++) o[pos + i] = 0; }
    else {
      o[pos] = (u8)(2u + (w[8] & 1u));
      for (int i = 0; i < 32; i++) o[pos + 1 + i] = (u8)(w[7 - (i >> 2)] >> (8 * (3 - (i & 3))));
    }
    if (ys) for (int i = 0; i < 32; i++) ys[32u * j + i] = (u8)(w[15 - (i >> 2)] >> (8 * (3 - (i & 3))));      // (zeros for the identity)
    pos += 33;
  }
  for (u32 j = 0; j < 3u; j++) { put_be32(o + pos, ld_sc(B.chal + 32ull * p + 8u * j)); pos += 32; }
  put_be32(o + pos, B.x_ip); pos += 32;
  const u64 s0 = seed_off[p], sl = seed_off[p + 1] - s0;
  o[pos] = (u8)(sl >> 8); o[pos + 1] = (u8)sl; pos += 2;
  for (u64 i = 0; i < sl; i++) o[pos + i] = seeds[s0 + i];
  pos += (u32)sl;
  o[pos] = 0; o[pos + 1] = 0;
}

__global__ void __launch_bounds__(256) k_pv_blind_mixed(MixedTab M) {
  const MixedUnit un = mixed_unit(M);
  const Batch B = *mixed_batch(M, un.cls);
  pv_blind_block(B, blockIdx.x - un.first);
}
__global__ void __launch_bounds__(256) k_pv_commit_A_mixed(MixedTab M) {
  const MixedUnit un = mixed_unit(M);
  const Batch B = *mixed_batch(M, un.cls);
  pv_commit_A_block(B, B.jout, blockIdx.x - un.first);
}
// the class's results B.jout -> B.pts: per results a proof from slot0 on, slot_step apart (step_k: the class's k, the L_r / R_r of a round)
__global__ void __launch_bounds__(256) k_pv_affine_mixed(MixedTab M, u32 per, u32 slot0, u32 slot_step, u32 step_k) {
  const MixedUnit un = mixed_unit(M);
  const Batch *B = mixed_batch(M, un.cls);
  const u32 k = B->k;
  pv_affine_block(B->jout, per * B->P, per, B->pts, 6u + 2u * k, slot0, step_k ? k : slot_step, blockIdx.x - un.first);
}
// jobs: the step's MsmJobs per class
template <int GL> __global__ void __launch_bounds__(256) k_pv_msm_mixed(MixedTab M, const MsmJobs *__restrict__ jobs, Tab T) {
  const MixedUnit un = mixed_unit(M);
  const MsmJobs J = jobs[un.cls];
  pv_msm_block<GL>(J, T, blockIdx.x - un.first);
}
__global__ void __launch_bounds__(64) k_pv_chal_yz_mixed(MixedTab M) {
  const MixedUnit un = mixed_unit(M);
  const Batch B = *mixed_batch(M, un.cls);
  pv_chal_yz_block(B, blockIdx.x - un.first);
}
template <u32 NT> __global__ void __launch_bounds__(NT) k_pv_poly_mixed(MixedTab M) {
  const MixedUnit un = mixed_unit(M);
  const Batch B = *mixed_batch(M, un.cls);
  pv_poly_block<NT>(B, blockIdx.x - un.first);
}
__global__ void __launch_bounds__(64) k_pv_final_chal_mixed(MixedTab M) {
  const MixedUnit un = mixed_unit(M);
  const Batch B = *mixed_batch(M, un.cls);
  pv_final_chal_block(B, blockIdx.x - un.first);
}
template <u32 NT> __global__ void __launch_bounds__(NT) k_pv_final_wide_mixed(MixedTab M) {
  const MixedUnit un = mixed_unit(M);
  const Batch B = *mixed_batch(M, un.cls);
  pv_final_wide_block<NT>(B, blockIdx.x - un.first);
}
__global__ void __launch_bounds__(64) k_pv_round_chal_mixed(MixedTab M, u32 round) {
  const MixedUnit un = mixed_unit(M);
  const Batch B = *mixed_batch(M, un.cls);
  pv_round_chal_block(B, round, blockIdx.x - un.first);
}
template <u32 NT> __global__ void __launch_bounds__(NT) k_pv_round_wide_mixed(MixedTab M, u32 round, u32 first) {
  const MixedUnit un = mixed_unit(M);
  const Batch B = *mixed_batch(M, un.cls);
  pv_round_wide_block<NT>(B, round, first, blockIdx.x - un.first);
}
// seed_off, out_off: call-wide, class-major; a class's rows start at its B.p0
__global__ void __launch_bounds__(64) k_pv_emit_mixed(MixedTab M, const u8 *__restrict__ seeds, const u64 *__restrict__ seed_off, u8 *__restrict__ out, const u64 *__restrict__ out_off, u32 fmt) {
  const MixedUnit un = mixed_unit(M);
  const Batch B = *mixed_batch(M, un.cls);
  pv_emit_block(B, seeds, seed_off + B.p0, out, out_off + B.p0, fmt, blockIdx.x - un.first);
}

}  // namespace rpp
