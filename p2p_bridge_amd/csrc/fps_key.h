// fps_key.h -- the maximum search of the furthest-point-sampling kernels that reproduce a reference block's tie order
// (pointnet2_legacy.hip, pointops.hip): 64-bit keys (running minimum, tie order of a T-thread block), their DPP maximum
// over a wave and the workgroup's maximum from the waves' maxima.
#pragma once
#include "common.h"

typedef unsigned long long u64;

// (The DPP maximum and the key helpers restate sampling.hip's, whose device code is pinned by its bit-exact tests and whose
//  key is fixed to the 512 threads of the PVCNN sampler; this one takes log2 T.)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned pn2_umax_step(unsigned v) {
  const unsigned o = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);  // (0 = identity of max)
  return o > v ? o : v;
}
// max over each 16-lane row, valid in the row's lane 15
__device__ __forceinline__ unsigned pn2_rowmax_u32(unsigned v) {
  v = pn2_umax_step<0x111, 0xf>(v);  // row_shr:1
  v = pn2_umax_step<0x112, 0xf>(v);  // row_shr:2
  v = pn2_umax_step<0x114, 0xf>(v);  // row_shr:4
  v = pn2_umax_step<0x118, 0xf>(v);  // row_shr:8
  return v;
}
__device__ __forceinline__ unsigned pn2_wavemax_u32(unsigned v) {
  v = pn2_rowmax_u32(v);
  v = pn2_umax_step<0x142, 0xa>(v);  // row_bcast:15 into rows 1, 3
  v = pn2_umax_step<0x143, 0xc>(v);  // row_bcast:31 into rows 2, 3 -> lane 63 holds the wave's maximum
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
// lexicographic maximum of 64-bit keys as two 32-bit reductions: the high words, then the low words of the lanes that
// hold the winning high word. WAVE: over the 64 lanes; else over the first 16-lane row. Returned in every lane.
template <bool WAVE>
__device__ __forceinline__ u64 pn2_max_u64(u64 v) {
  const unsigned hi = (unsigned)(v >> 32);
  unsigned H, L;
  if (WAVE) {
    H = pn2_wavemax_u32(hi);
    L = pn2_wavemax_u32(hi == H ? (unsigned)v : 0u);
  } else {
    H = (unsigned)__builtin_amdgcn_readlane((int)pn2_rowmax_u32(hi), 15);
    L = (unsigned)__builtin_amdgcn_readlane((int)pn2_rowmax_u32(hi == H ? (unsigned)v : 0u), 15);
  }
  return ((u64)H << 32) | L;
}
// best > 0: its bit pattern + 1 (monotonic); 0: 1; a thread without points carries -1 -> 0, the lowest key.
// low word: ~((k mod T) << 21 | k / T), lt = log2 T <= 10 (k / T < 2^21 for any int k)
__device__ __forceinline__ u64 pn2_fps_key(float best, int k, int lt) {
  const unsigned hi = best > 0.0f ? (__float_as_uint(best) + 1u) : (best == 0.0f ? 1u : 0u);
  const unsigned sec = (((unsigned)k & ((1u << lt) - 1u)) << 21) | ((unsigned)k >> lt);
  return ((u64)hi << 32) | (u64)(~sec);
}
__device__ __forceinline__ int pn2_fps_key_index(u64 key, int lt) {
  const unsigned sec = ~(unsigned)key;
  return (int)(((sec & 0x1FFFFFu) << lt) | (sec >> 21));
}
// the workgroup's maximum from the waves' maxima: one LDS slot per wave (double-buffered by round parity), one barrier,
// and a 16-entry row reduction that every wave repeats (slots [2][16], zero = identity beyond the last wave)
__device__ __forceinline__ u64 pn2_block_max(u64 key, u64 *slots, int j, int t) {
  u64 *sl = slots + (j & 1) * 16;
  if ((t & 63) == 0) sl[t >> 6] = key;
  __syncthreads();
  return pn2_max_u64<false>(sl[t & 15]);
}
