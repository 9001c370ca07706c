// h2c_kernels.hpp -- part of libbpmi (included by bpmi.hip; one translation unit).  DEVICE code.
// Bulk hash to the curve: n messages -> n generators, the reference's elliptic_hash (/root/reference/src/utils/elliptic_curve_hash.py:7-23)
// with the per-candidate bodies of h2c.hpp.  Two message sources behind one body:
//   batch form   message i = bytes[off[i], off[i + 1])
//   range form   message i = str(lo + i) || bytes[0, tail_len): the index digits are made in registers, only the tail is uploaded
//                (the idiom  [elliptic_hash(str(i).encode() + seed) for i in range(n)]  of every generator list)
//
// The retry loop.  A candidate succeeds with probability 1/2, so a message takes 2 candidates on average but the slowest of 64 takes
// about 7: with one message per lane and a loop per lane (k_h2c_plain: the kernel of calls so small that a lane has one message
// anyway, h2c_host.hpp, and the other side of the A/B run of tools/bench_hash_to_curve.py) three
// quarters of a wave's issue slots are masked off, and a candidate is ~266 dependent field multiplications.  k_h2c_queue instead gives a
// WAVE a contiguous span of messages, several per lane: in every iteration each lane with a message does exactly ONE candidate of it,
// and a lane whose message is finished takes the next unclaimed message of the span -- the ballot of the finished lanes and a prefix
// count over a wave-uniform cursor, no atomics, no LDS.  Only the last few iterations of a span run with idle lanes.  The claim step
// stands in wave-uniform control flow, outside every lane-dependent branch: all 64 lanes of a wave stay in the loop until the
// wave-uniform exit, so the ballot always sees the whole wave.
// Every loop is bounded: a message gets at most max_tries (<= 255) candidates, a span at most span x max_tries iterations.
#pragma once

struct H2cArgs {
  const uint8_t *bytes;         // batch form: the packed messages; range form: the tail
  const u64 *off;               // batch form: n + 1 offsets into bytes
  u64 lo;                       // range form: the index of message 0
  u32 tail_len;                 // range form
  u32 n;
  u32 max_tries;                // 1 .. 255
  u32 span;                     // k_h2c_queue: messages per wave
  u32 *out;                     // n x 16 words
  uint8_t *tries;               // n: the counter that succeeded, 0 = none did (the point is then 16 zero words)
  u32 *first_bad;               // the smallest index without a point (atomicMin; ~0 before the launch)
};

template <bool RANGE> __device__ __forceinline__ H2cMsg h2c_message(const H2cArgs &a, u32 i) {
  H2cMsg m;
  if (RANGE) { m.bytes = a.bytes; m.len = a.tail_len; m.idx = (u32)(a.lo + i); m.ranged = true; }
  else { const u64 o = a.off[i]; m.bytes = a.bytes + o; m.len = (u32)(a.off[i + 1] - o); m.idx = 0; m.ranged = false; }
  return m;
}
__device__ __forceinline__ void h2c_emit(const H2cArgs &a, u32 i, const u32 w16[16], u32 tries) {
  store_words16(a.out + 16ull * i, w16);
  a.tries[i] = (uint8_t)tries;
  if (!tries) atomicMin(a.first_bad, i);
}

// one message per lane, one loop per lane
template <bool RANGE> __global__ void __launch_bounds__(256, 3) k_h2c_plain(const H2cArgs a) {
  const u32 i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.n) return;
  u32 w16[16];
  const u32 t = h2c_hash(h2c_message<RANGE>(a, i), a.max_tries, w16);
  h2c_emit(a, i, w16, t);
}

// one span of messages per wave, one candidate per lane and iteration
template <bool RANGE> __global__ void __launch_bounds__(256, 3) k_h2c_queue(const H2cArgs a) {
  const u32 wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + threadIdx.x / 64u);
  const u32 lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  const u64 first = (u64)wave * a.span;
  if (first >= a.n) return;                                     // wave-uniform
  const u32 end = (u32)(first + a.span < a.n ? first + a.span : a.n);
  u32 next = (u32)first;                                        // wave-uniform cursor: the first unclaimed message of the span
  const u32 NONE = ~0u;
  u32 cur = NONE, c = 0;                                        // this lane's message, and the candidates it has had
  const u32 bound = (end - next) * a.max_tries + 1u;            // span <= 2^16, max_tries <= 255
#pragma unroll 1
  for (u32 it = 0; it <= bound; it++) {
    // the claim step, in wave-uniform control flow: lanes without a message take the next ones of the span, in lane order
    const bool want = cur == NONE;
    const unsigned long long free_lanes = __ballot(want);
    if (want) {
      const u32 mine = next + (u32)__popcll(free_lanes & ((1ull << lane) - 1ull));
      if (mine < end) { cur = mine; c = 0; }
    }
    const u32 taken = (u32)__popcll(free_lanes);
    next = end - next < taken ? end : next + taken;
    if (__ballot(cur != NONE) == 0ull) break;                   // wave-uniform: the span is done
    if (cur != NONE) {
      u32 w16[16];
      c++;
      const bool ok = h2c_try(h2c_message<RANGE>(a, cur), c, w16);
      if (ok || c >= a.max_tries) {
        if (!ok) {
#pragma unroll
          for (int k = 0; k < 16; k++) w16[k] = 0;
        }
        h2c_emit(a, cur, w16, ok ? c : 0u);
        cur = NONE;
      }
    }
  }
}
