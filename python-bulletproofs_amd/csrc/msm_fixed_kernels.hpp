// msm_fixed_kernels.hpp -- part of libbpmi (included by bpmi.hip; one translation unit).
// Kernels of the fixed-base MSM (msm_fixed_plan_host.hpp): the table of multiples T[r][i] = 2^(c Wv r) P_i, and the recoding that turns
// the W real windows of n scalars into the Wv virtual windows of n R virtual pairs.  Everything behind the recoding -- the LDS sort, both
// accumulations, the segmented scan, the bucket reduction, both tails -- is the bucket pipeline's own (msm_kernels.hpp), run on the
// virtual geometry with the table as its points.
#pragma once

// ---- the table, row by row -----------------------------------------------------------------------------------------------
// One launch builds row r from row r - 1: `doublings` = c Wv doublings of every point, then the affine, canonical form the MSM's
// input layout wants (16 words, the identity 64 zero bytes).  A thread takes FIXED_TAB_PER points (strided: consecutive threads read
// consecutive points) and normalises them with ONE inversion (Montgomery's trick): the doubled points wait as XYZZ records in global
// scratch beside the prefix products of their ZZ ZZZ -- eight 36-word records and the inversion's temporaries do not fit a thread's
// registers.  An identity stays the identity (xyzz_dbl copies it) and enters the product chain as 1.
//   scratch: FIXED_TAB_PER x ncols records of 36 words (record e of column t at (e ncols + t) 36), then as many prefixes of 9 words
#define FIXED_TAB_PER 8u
static inline size_t fixed_table_scratch_bytes(uint64_t n) {
  const uint64_t ncols = (n + FIXED_TAB_PER - 1u) / FIXED_TAB_PER;
  return (size_t)(4ull * (XYZZ_WORDS + 9u) * FIXED_TAB_PER * ncols);
}
__global__ void __launch_bounds__(256) k_fixed_table_row(const u32 *__restrict__ prev, u32 *__restrict__ next, u32 n, u32 doublings, u32 *__restrict__ scratch) {
  const u32 ncols = (n + FIXED_TAB_PER - 1u) / FIXED_TAB_PER;
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ncols) return;
  u32 *const prefs = scratch + (u64)XYZZ_WORDS * FIXED_TAB_PER * ncols;
  fe pref;
  fe_set_one(pref);
  for (u32 e = 0; e < FIXED_TAB_PER; e++) {
    const u32 k = t + e * ncols;
    xyzz A;
    xyzz_set_inf(A);
    if (k < n) {
      affine P;
      load_affine(P, prev + 16ull * k);
      xyzz_from_affine(A, P);
    }
#pragma unroll 1
    for (u32 d = 0; d < doublings; d++) xyzz_dbl(A, A);
    const u64 rec = (u64)e * ncols + t;
    xyzz_store_g(scratch + rec * XYZZ_WORDS, A);
#pragma unroll
    for (int l = 0; l < 9; l++) prefs[rec * 9u + l] = pref.v[l];
    if (!xyzz_is_inf(A)) {
      fe z;
      fe_mul(z, A.ZZ, A.ZZZ);
      fe_mul(pref, pref, z);
    }
  }
  fe inv;
  fe_inv(inv, pref);                                          // 1 / (product of every finite point's ZZ ZZZ)
  for (int e = (int)FIXED_TAB_PER - 1; e >= 0; e--) {
    const u32 k = t + (u32)e * ncols;
    const u64 rec = (u64)e * ncols + t;
    xyzz A;
    xyzz_load_g(A, scratch + rec * XYZZ_WORDS);
    u32 w16[16];
    if (xyzz_is_inf(A)) {
#pragma unroll
      for (int l = 0; l < 16; l++) w16[l] = 0;
    } else {
      fe pj, z, zi, izz, izzz;
#pragma unroll
      for (int l = 0; l < 9; l++) pj.v[l] = prefs[rec * 9u + l];
      fe_mul(zi, inv, pj);                                    // 1 / (ZZ ZZZ) of this point
      fe_mul(z, A.ZZ, A.ZZZ);
      fe_mul(inv, inv, z);
      fe_mul(izz, zi, A.ZZZ);                                 // 1 / ZZ
      fe_mul(izzz, zi, A.ZZ);                                 // 1 / ZZZ
      affine r;
      fe_mul(r.x, A.X, izz);
      fe_mul(r.y, A.Y, izzz);
      affine_to_words(w16, r);                                // canonical: x, y < p
    }
    if (k < n) store_words16(next + 16ull * k, w16);
  }
}

// ---- the recoding ----------------------------------------------------------------------------------------------------------
// Stands in for k_coarse_hist on the fixed-base path.  Reads the n_scalars real scalars through for_each_digit_raw over the real
// uniform geometry {n, c, W} and writes, for the virtual geometry g (g.n = n R pairs, g.W = Wv windows):
//   dig16[wv g.n + r n + i]  the code of real window w = r Wv + wv of scalar i (fixed_window_slot), the digit's own sign in bit 15 as in
//                            k_coarse_hist; DIG_NONE for the slots beyond window W - 1 and for i >= n_scalars: EVERY one of the Wv g.n codes
//   negs[r n + i]            1 = scalar i was replaced by q - s, for every row: k_partition reads negs[v] for every virtual pair v.  (The
//                            scalar's sign cannot ride in bit 15: at c = 16 a digit of magnitude 2^15 has b - 1 = 0x7FFF, and with the
//                            bit set the code would be DIG_NONE.)
//   coarse_hist              the counts of the virtual partitions (wv, (b - 1) >> 8), through the block's LDS histogram
// The scan of the counts is always k_coarse_scan's launch: the last-block fusion ("hist_scan_fused") is k_coarse_hist's.
struct MsmRecode {
  MsmPlan plan;            // the virtual geometry: msm_enqueue runs it instead of picking one
  Segs sc;                 // the real scalars as one dense segment of n_scalars
  MsmGeom real;            // {n, c, W}: the recoding's own geometry (fixed_real_geometry)
  u32 n_scalars, R, Wv;
};
__global__ void __launch_bounds__(1024) k_fixed_recode(Segs sc, MsmGeom real, u32 n_scalars, u32 R, u32 Wv, MsmGeom g, u32 P, u32 *coarse_hist,
                                                      unsigned short *__restrict__ dig16, unsigned char *__restrict__ negs) {
  raise_priority(g.prio & PRIO_SORT);
  __shared__ u32 lh[PART_MAX];
  for (u32 p = threadIdx.x; p < P; p += blockDim.x) lh[p] = 0;
  __syncthreads();
  const u32 Bc = g.B >> 8, n = real.n, slots = Wv * R;
  const u32 stride = gridDim.x * blockDim.x;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    bool neg = false;
    u32 w_none = 0;                                         // the slots from real window w_none on hold no digit
    if (i < n_scalars) {
      neg = for_each_digit_raw(sc, real, i, [&](u32 w, u32 b, u32 dsign) {
        const FixedSlot s = fixed_window_slot(w, Wv);
        dig16[(u64)s.wv * g.n + (u64)s.r * n + i] = (unsigned short)(b ? ((b - 1u) | (dsign << 15)) : DIG_NONE);
        if (b) atomicAdd(&lh[s.wv * Bc + ((b - 1u) >> 8)], 1u);
      });
      w_none = real.W;
    }
    for (u32 w = w_none; w < slots; w++) {
      const FixedSlot s = fixed_window_slot(w, Wv);
      dig16[(u64)s.wv * g.n + (u64)s.r * n + i] = (unsigned short)DIG_NONE;
    }
    for (u32 r = 0; r < R; r++) negs[(u64)r * n + i] = neg ? 1 : 0;
  }
  __syncthreads();
  for (u32 p = threadIdx.x; p < P; p += blockDim.x) { const u32 v = lh[p]; if (v) atomicAdd(&coarse_hist[p], v); }
}
