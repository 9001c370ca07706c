// ipa_mixed_kernels.hpp -- part of libbpmi (included by bpmi.hip; one translation unit).  DEVICE code.
// The s-vectors of a batch of proofs of DIFFERENT lengths over the prefixes of one generator list, summed under random weights
// (bpmi_ipa_verify_batch_mixed_dev):  SA_i = sum_{p : n_p > i} w_p a_p s_{p,i},  SB_i = c_i sum_{p : n_p > i} w_p b_p s_{p,i}^-1.
// The per-thread bodies are svector_mixed.hpp (plain C++: tests/test_ipa_mixed_host_cpu.py runs the host build through every unit);
// the launch shapes, the tables the kernels read and the workspace are ipa_mixed_plan_host.hpp.
#pragma once

// Every proof's half tables in one launch: one thread per record of the PACKED table array, which finds its proof by bisection over the
// descriptors' table offsets (16 steps at 2^16 proofs, beside the k / 2 + 1 multiplications mod q of a record).  A grid of (records
// of the longest proof) x (proofs) whose surplus threads return was measured first: one proof of 2^20 beside 2^14 of 64 elements
// launched 131 080 blocks for 4 112 of work and took 0.67 ms (profiles/r16_ipa_verify_mixed.txt).
__global__ void __launch_bounds__(256) k_sc_svector_tables_mixed(const u32 *__restrict__ recs, const u32 *__restrict__ desc, u32 n_proofs, u32 n_records,
                                                                 u32 *__restrict__ tabs) {
  const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_records) return;
  u32 e[16];
  svm_table_record(e, recs, desc, n_proofs, r);
  store_words8(tabs + 16ull * r, e);
  store_words8(tabs + 16ull * r + 8, e + 8);
}
// The hot loop: block = unit (element block, p0, p1, slot), lane = element.  direct: SA and SB themselves (every block has one unit,
// no scale); else the slot's partial sums, 256 values of A and 256 of B.
__global__ void __launch_bounds__(256) k_sc_svector_sum_mixed(const u32 *__restrict__ tabs, const u32 *__restrict__ desc, const u32 *__restrict__ C,
                                                              const u32 *__restrict__ units, u32 n_top, u32 direct, u32 *__restrict__ out_a,
                                                              u32 *__restrict__ out_b) {
  const u32 *un = units + 4ull * blockIdx.x;
  const u32 e = un[0], p0 = un[1], p1 = un[2], slot = un[3];
  const u32 i = e * 256u + threadIdx.x;
  if (i >= n_top) return;
  u32 ra[8], rb[8];
  svm_sum_element(ra, rb, tabs, desc, C, i, p0, p1);
  if (direct) {
    store_words8(out_a + 8ull * i, ra);
    store_words8(out_b + 8ull * i, rb);
  } else {
    store_words8(out_a + 4096ull * slot + 8ull * threadIdx.x, ra);
    store_words8(out_a + 4096ull * slot + 8ull * (256u + threadIdx.x), rb);
  }
}
// SA_i, SB_i from the partial sums of the units of element i's block; SB_i times the shared scale c_i (or scale == null)
__global__ void __launch_bounds__(256) k_sc_svector_sum_finish_mixed(const u32 *__restrict__ part, const u32 *__restrict__ block_first, u32 n_top,
                                                                     const u32 *__restrict__ scale, u32 *__restrict__ sa, u32 *__restrict__ sb) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_top) return;
  u32 ra[8], rb[8];
  svm_finish_element(ra, rb, part, block_first, scale, i);
  store_words8(sa + 8ull * i, ra);
  store_words8(sb + 8ull * i, rb);
}
// The sums per GROUP of consecutive proofs of one class, for every class of a mixed packed batch in ONE launch
// (bpmi_ipa_group_values_packed_mixed_dev; plan: ipa_group_mixed_plan_host.hpp): rows SA[t][i], SB[t][i] of n_c = 2^k_c scalars,
// canonical, SB with the shared scale c_i -- k_sc_svector_sum_groups (scalar_kernels.hpp) over classes of different row lengths.  A
// class's rows start at a multiple of 256 scalars, so a block belongs to one class and looks it up with its own index
// (svm_group_row_element, svector_mixed.hpp); pad lanes behind a class's last row return.
__global__ void __launch_bounds__(256) k_sc_svector_sum_groups_mixed(const u32 *__restrict__ tabs, const u32 *__restrict__ ctab, u32 n_cls,
                                                                     const u32 *__restrict__ scale, u32 *__restrict__ sa, u32 *__restrict__ sb) {
  u32 ra[8], rb[8], idx;
  if (!svm_group_row_element(ra, rb, idx, tabs, ctab, n_cls, scale, blockIdx.x, threadIdx.x)) return;
  store_words8(sa + 8ull * idx, ra);
  store_words8(sb + 8ull * idx, rb);
}
