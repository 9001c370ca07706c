// ipa_prove_mixed_kernels.hpp -- part of libbpmi (included by bpmi.hip behind ipa_prove_kernels.hpp; one translation unit).  DEVICE code.
// The batched inner-product prover over CLASSES of different lengths in one call (bpmi_ipa_prove_batch_mixed and
// bpmi_ipa_batch_prover_commit_batch_mixed, ipa_prove_mixed_host.hpp): every kernel of ipa_prove_kernels.hpp has a `_mixed` twin that
// runs the SAME per-block body (ip_*_block) for the blocks of every class of a step in ONE launch -- the shape of
// rp_prove_mixed_kernels.hpp, whose unit table (rpp::MixedTab, rpp::mixed_unit) and multiplication (rpp::k_pv_msm_mixed, which reads
// only the unit table and the step's MsmJobs) are used as they are.  A twin looks its unit {class, first block} up from blockIdx.x,
// copies the class's record from a device array of fixed slots (ipa_prove_mixed_plan_host.hpp) and calls the body with the block's index
// inside the class.
//
// Why the bodies' barriers and shuffles stay legal.  Every early return, __syncthreads and wave shuffle of ip_round_wide_block and
// ip_commit_scalars_block depends on
//   * the launch arguments (round, first), the same for every block of a launch, and
//   * fields of the record that are uniform per class: n (hence len, half, the reduction's trip count and `n > 64`), proto, c_in (the
//     block `first && proto == 1 && !c_in` with its barriers), u_mode and the NULL halves a_in / b_in (the returns of the statements'
//     kernel before its shuffles and its barrier).
// `live` (p < P) guards loads and stores only, never a barrier or a shuffle: the lanes of proofs beyond the class's count carry zeros
// through both.  The one return between barriers, `len == 1`, depends on n, round and first alone.  In the single-class kernels these
// values are uniform over the launch; a twin's block belongs to ONE class -- the lookup depends on blockIdx.x alone and the plan gives
// every class whole blocks -- so they are uniform over the block, which is all __syncthreads and the 64-lane shuffles ask for (a wave
// never spans two blocks).  Neighbouring classes may differ in any of them: one class sums <a, b> in LDS (c_in NULL), the next does not.
#pragma once

namespace ipp {

// a class's results of a multiplication made affine: result j of `count` goes to pts[(j / per) pt_stride + slot0 + (j % per) slot_step].
// Proving: in = jout, count = 2 P, per = 2, pts = lr, pt_stride = 2 k_c, slot_step = k_c, slot0 = the round.  Statements: count, 1, pts, 1, 0.
struct AffineJob { const u32 *in; u32 *pts; u32 count, per, pt_stride, slot_step; };

static_assert(sizeof(Batch) <= IPPM_BATCH_SLOT, "the plan lays the class records out in IPPM_BATCH_SLOT-byte slots (ipa_prove_mixed_plan_host.hpp)");
static_assert(sizeof(Commit) <= IPPM_COMMIT_SLOT, "the plan lays the statements' records out in IPPM_COMMIT_SLOT-byte slots (ipa_prove_mixed_plan_host.hpp)");
static_assert(sizeof(AffineJob) == IPPM_AFFINE_SLOT, "the plan lays the affine records out in IPPM_AFFINE_SLOT-byte slots (ipa_prove_mixed_plan_host.hpp)");
static_assert(sizeof(rpp::MsmJobs) == IPPM_JOBS_SLOT, "the plan lays the job records out in IPPM_JOBS_SLOT-byte slots");

using rpp::MixedTab;
using rpp::MixedUnit;
// M.batches: this call's array of records, IPPM_BATCH_SLOT (proving) or IPPM_COMMIT_SLOT (statements) bytes each
__device__ __forceinline__ const Batch *ip_mixed_batch(const MixedTab &M, u32 cls) { return (const Batch *)(M.batches + (size_t)IPPM_BATCH_SLOT * cls); }
__device__ __forceinline__ const Commit *ip_mixed_commit(const MixedTab &M, u32 cls) { return (const Commit *)(M.batches + (size_t)IPPM_COMMIT_SLOT * cls); }

__global__ void __launch_bounds__(64) k_ip_begin_mixed(MixedTab M) {
  const MixedUnit un = rpp::mixed_unit(M);
  const Batch B = *ip_mixed_batch(M, un.cls);
  ip_begin_block(B, blockIdx.x - un.first);
}
__global__ void __launch_bounds__(256) k_ip_head_mixed(MixedTab M) {
  const MixedUnit un = rpp::mixed_unit(M);
  const Batch B = *ip_mixed_batch(M, un.cls);
  ip_head_block(B, blockIdx.x - un.first);
}
__global__ void __launch_bounds__(64) k_ip_round_chal_mixed(MixedTab M, u32 round) {
  const MixedUnit un = rpp::mixed_unit(M);
  const Batch B = *ip_mixed_batch(M, un.cls);
  ip_round_chal_block(B, round, blockIdx.x - un.first);
}
template <u32 NT> __global__ void __launch_bounds__(NT) k_ip_round_wide_mixed(MixedTab M, u32 round, u32 first) {
  const MixedUnit un = rpp::mixed_unit(M);
  const Batch B = *ip_mixed_batch(M, un.cls);
  ip_round_wide_block<NT>(B, round, first, blockIdx.x - un.first);
}
template <u32 NT> __global__ void __launch_bounds__(NT) k_ip_commit_scalars_mixed(MixedTab M) {
  const MixedUnit un = rpp::mixed_unit(M);
  const Commit C = *ip_mixed_commit(M, un.cls);
  ip_commit_scalars_block<NT>(C, blockIdx.x - un.first);
}
// (rpp::k_pv_affine_mixed assumes the range prover's `pts` layout; this one takes the layout from the class's AffineJob)
__global__ void __launch_bounds__(256) k_ip_affine_mixed(MixedTab M, const AffineJob *__restrict__ jobs, u32 slot0) {
  const MixedUnit un = rpp::mixed_unit(M);
  const AffineJob A = jobs[un.cls];
  rpp::pv_affine_block(A.in, A.count, A.per, A.pts, A.pt_stride, slot0, A.slot_step, blockIdx.x - un.first);
}

}  // namespace ipp
