// ipa_wire_kernels.hpp -- part of libbpmi (included by bpmi.hip; one translation unit).  DEVICE code.
// Inner-product proofs in the wire format BPIP2 (format, validity and host twin: ipa_wire_host.hpp) become, IN DEVICE MEMORY, the
// packed form the preparation kernels of ipa_packed_kernels.hpp read -- ab, xs, LR, start, the offsets and the word-major transcript
// array T -- so a batch of wire proofs is uploaded as its bytes and nothing of its expansion crosses the link:
//   k_ipaw_decompress   one lane per point: the 2k SEC1 encodings of a proof where they lie in its blob -> its LR rows (64 bytes
//                       affine, zero for the identity and for an encoding that does not decode, which sets the proof's point flag).
//                       A sibling of k_ec_decompress_wire (point_kernels.hpp) over the same ec_decompress_one
//   k_ipaw_expand       sixteen lanes per proof, the shape of rpd::k_rp_expand_v2 and its TWriter: the lanes measure the items whose
//                       length depends on the data (the digits of a scalar, "AA==" or 44 characters for a point), lane 0 lays the
//                       rounds out behind the prefix, then the items are written KIND BY KIND -- all decimal items, all point
//                       items, the prefix in 64-byte pieces -- so that the lanes of a wave run the same code.  Whole words go out
//                       with plain stores, the first and last word of an item with atomicOr into the zeroed array.  It also writes
//                       ab and xs little-endian, start, the transcript's length and the proof's malformed flag
//   k_ipaw_offsets      the lengths of a launch's proofs summed into the offsets region: the preparation reads a transcript's length
//                       as tr_off[g + 1] - tr_off[g], so its kernels run unchanged
//   k_ipaw_verdicts     the two flags of a proof written over its role verdicts between k_ipap_roles and k_ipap_finish, which then
//                       treats the proof as any flagged one: its status byte, identity points, zero scalars, a zero record
// T is written for the rows of ONE launch (T[w * cnt + r], r = the proof's index inside the launch), as k_ipap_transpose leaves it.
#pragma once

namespace ipad {

#define IPAW_LPP 16u                       // lanes per proof of k_ipaw_expand
#define IPAW_K_MAX 22u                     // IPAB_K_MAX: 2 + k scalars and 2 k points are measured per proof

__device__ __forceinline__ bool ipaw_head_ok(const uint8_t *b, u64 len, u32 k) {
  return len >= 78ull + 98ull * k && b[0] == 'B' && b[1] == 'P' && b[2] == 'I' && b[3] == 'P' && b[4] == '2' && b[5] == k;
}
__device__ __forceinline__ u32 ipaw_be32(const uint8_t *p) { return ((u32)p[0] << 24) | ((u32)p[1] << 16) | ((u32)p[2] << 8) | p[3]; }

// blobs: the call's blobs from byte `origin` (= the host's off[0]) on; off: the call's offsets; proofs [first, first + cnt).
// LR: the call's rows; ptflag: one byte per proof of the call, zeroed by the caller
__global__ void __launch_bounds__(256, 3) k_ipaw_decompress(const uint8_t *__restrict__ blobs, const u64 *__restrict__ off, u64 origin, u32 k, u64 first, u32 cnt,
                                                            u32 *__restrict__ LR, uint8_t *__restrict__ ptflag) {
  const u32 per = 2 * k;
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cnt * per) return;
  const u64 g = first + i / per;
  const u32 t = i % per;
  u32 w16[16];
#pragma unroll
  for (int j = 0; j < 16; j++) w16[j] = 0;
  const uint8_t *b = blobs + (off[g] - origin);
  if (ipaw_head_ok(b, off[g + 1] - off[g], k)) {
    if (!::ec_decompress_one(b + 6 + 32 * (2 + k) + 33 * t, w16)) ptflag[g] = 1;
  }
  ::store_words16(LR + 16ull * (per * g + t), w16);
}

__global__ void __launch_bounds__(64) k_ipaw_expand(const uint8_t *__restrict__ blobs, const u64 *__restrict__ off, u64 origin, u32 k, u64 first, u32 cnt, u32 W,
                                                    u64 *__restrict__ T, u32 *__restrict__ ab, u32 *__restrict__ xs, u32 *__restrict__ start,
                                                    u32 *__restrict__ lens, uint8_t *__restrict__ badflag) {
  __shared__ u32 s_len[4][2 + 3 * IPAW_K_MAX];     // measured lengths: a b x_0 .. (0: not below q), then the points L_0 .. R_0 ..
  __shared__ u32 s_dec[4][IPAW_K_MAX];             // byte offsets of the decimal items x_0 ..
  __shared__ u32 s_pt[4][2 * IPAW_K_MAX];          // byte offsets of the point items L_0 R_0 L_1 R_1 ..
  const u32 pw = threadIdx.x >> 4, lane = threadIdx.x & (IPAW_LPP - 1u);
  const u32 r = blockIdx.x * 4u + pw;
  const bool live = r < cnt;
  const u64 g = first + (live ? r : 0u);
  const uint8_t *b = blobs + (off[g] - origin);
  const u64 n_wire = off[g + 1] - off[g];
  const u32 fixed = 78u + 98u * k, pts_at = 6u + 32u * (2u + k), start_at = pts_at + 66u * k;
  bool ok = live && ipaw_head_ok(b, n_wire, k);
  u32 prefix_len = 0;
  if (ok) {
    prefix_len = ipaw_be32(b + start_at + 4);
    ok = (u64)fixed + prefix_len == n_wire;
  }
  const uint8_t *sc = b + 6, *pts = b + pts_at, *prefix = b + start_at + 8;
  const u32 nsc = 2 + k, nmeas = nsc + 2 * k;
  if (ok)
    for (u32 j = lane; j < nmeas; j += IPAW_LPP) s_len[pw][j] = j < nsc ? dec_item_len(sc + 32 * j) : (comp_is_identity(pts + 33 * (j - nsc)) ? 5u : 45u);
  __syncthreads();
  const u32 *L = s_len[pw];
  if (ok) for (u32 j = 0; j < nsc; j++) ok = ok && L[j] != 0;                   // a, b or a challenge >= q
  u64 out_len = prefix_len;
  if (ok) {
    for (u32 j = 0; j < k; j++) out_len += L[nsc + j] + L[nsc + k + j] + L[2 + j];
    ok = out_len <= IPAP_MAX_TRANSCRIPT && (out_len + 7u) / 8u <= W;
  }
  if (ok && lane == 0) {                                        // the layout, once per proof
    u32 pos = prefix_len;
    for (u32 j = 0; j < k; j++) {
      s_pt[pw][2 * j] = pos; pos += L[nsc + j];                 // L_j
      s_pt[pw][2 * j + 1] = pos; pos += L[nsc + k + j];         // R_j
      s_dec[pw][j] = pos; pos += L[2 + j];                      // x_j
    }
  }
  __syncthreads();
  if (ok) {
    u64 *base = T + r;
    for (u32 j = lane; j < k; j += IPAW_LPP) {                  // decimal items
      TWriter t = tw_at(base, cnt, W, s_dec[pw][j]);
      tw_decimal(t, sc + 32 * (2 + j));
      tw_flush(t);
    }
    for (u32 j = lane; j < 2 * k; j += IPAW_LPP) {              // point items
      TWriter t = tw_at(base, cnt, W, s_pt[pw][j]);
      tw_point(t, pts + 33 * ((j >> 1) + (j & 1u) * k));
      tw_flush(t);
    }
    for (u32 o = 64u * lane; o < prefix_len; o += 64u * IPAW_LPP) {      // the prefix in pieces of 64 bytes
      const u32 n = prefix_len - o < 64u ? prefix_len - o : 64u;
      TWriter t = tw_at(base, cnt, W, o);
      for (u32 i = 0; i < n; i++) tw_put(t, prefix[o + i]);
      tw_flush(t);
    }
  }
  if (live) {
    // a, b, x_j: 32 bytes big-endian -> 8 little-endian words (zero rows for a malformed proof)
    for (u32 j = lane; j < nsc; j += IPAW_LPP) {
      u32 *dst = j < 2 ? ab + 16 * g + 8 * j : xs + 8 * ((u64)k * g + (j - 2));
#pragma unroll
      for (int i = 0; i < 8; i++) dst[i] = ok ? ipaw_be32(sc + 32 * j + 28 - 4 * i) : 0u;
    }
    if (lane == 0) {
      start[g] = ok ? ipaw_be32(b + start_at) : 0u;
      lens[g] = ok ? (u32)out_len : 0u;
      badflag[g] = ok ? 0 : 1;
    }
  }
}

// tr_off[first + i + 1] = tr_off[first] + lens[first] + .. + lens[first + i] for i < cnt (tr_off[0] = 0).  One block: a launch
// is at most 2^16 proofs, every thread sums one contiguous run
__global__ void __launch_bounds__(256) k_ipaw_offsets(const u32 *__restrict__ lens, u64 *__restrict__ tr_off, u64 first, u32 cnt) {
  __shared__ u64 part[256];
  const u32 run = (cnt + 255u) / 256u;
  const u32 lo = threadIdx.x * run < cnt ? threadIdx.x * run : cnt, hi = lo + run < cnt ? lo + run : cnt;
  u64 sum = 0;
  for (u32 i = lo; i < hi; i++) sum += lens[first + i];
  part[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 at = first ? tr_off[first] : 0ull;
    if (!first) tr_off[0] = 0;
    for (u32 t = 0; t < 256; t++) { const u64 s = part[t]; part[t] = at; at += s; }
  }
  __syncthreads();
  u64 at = part[threadIdx.x];
  for (u32 i = lo; i < hi; i++) { at += lens[first + i]; tr_off[first + i + 1] = at; }
}

// A proof the wire layer flagged -- bit 0 malformed, bit 1 a point that does not decode -- takes that verdict for its status: role 0's
// byte holds it and the other roles' bytes are cleared (they judged rows that are zero or half filled).  Proofs [first, first + cnt)
__global__ void __launch_bounds__(256) k_ipaw_verdicts(uint8_t *__restrict__ roles, u32 Pall, const uint8_t *__restrict__ badflag, const uint8_t *__restrict__ ptflag,
                                                       u64 first, u32 cnt) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i >= cnt) return;
  const u32 bits = (badflag[first + i] ? 1u : 0u) | (ptflag[first + i] ? 2u : 0u);
  if (!bits) return;
  for (u32 r = 0; r < IPAP_ROLES; r++) roles[(size_t)r * Pall + first + i] = (uint8_t)(r ? 0u : bits);
}

}  // namespace ipad
