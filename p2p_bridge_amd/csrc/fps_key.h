// fps_key.h -- the maximum search of every furthest-point-sampling kernel (sampling.hip, fps_ref.hip): 64-bit keys (running
// minimum, tie order of the reference's block), their DPP maximum over a wave and the workgroup's maximum from the waves'
// maxima.
#pragma once
#include "common.h"

typedef unsigned long long u64;

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned umax_step(unsigned v) {
  const unsigned o = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);  // (0 = identity of max)
  return o > v ? o : v;
}
// max over each 16-lane row, valid in the row's lane 15
__device__ __forceinline__ unsigned rowmax_u32(unsigned v) {
  v = umax_step<0x111, 0xf>(v);  // row_shr:1
  v = umax_step<0x112, 0xf>(v);  // row_shr:2
  v = umax_step<0x114, 0xf>(v);  // row_shr:4
  v = umax_step<0x118, 0xf>(v);  // row_shr:8
  return v;
}
__device__ __forceinline__ unsigned wavemax_u32(unsigned v) {
  v = rowmax_u32(v);
  v = umax_step<0x142, 0xa>(v);  // row_bcast:15 into rows 1, 3
  v = umax_step<0x143, 0xc>(v);  // row_bcast:31 into rows 2, 3 -> lane 63 holds the wave's maximum
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
// lexicographic maximum of 64-bit keys as two 32-bit reductions: the high words, then the low words of the lanes that
// hold the winning high word -- v_max_u32 steps instead of a 64-bit compare and two selects per step (the round of a
// small-cloud FPS is bound by its VALU instruction count). WAVE: over the 64 lanes; else over the first 16-lane row (the
// callers' rows all hold the same 16 values). Returned in every lane.
template <bool WAVE>
__device__ __forceinline__ u64 max_u64(u64 v) {
  const unsigned hi = (unsigned)(v >> 32);
  unsigned H, L;
  if (WAVE) {
    H = wavemax_u32(hi);
    L = wavemax_u32(hi == H ? (unsigned)v : 0u);
  } else {
    H = (unsigned)__builtin_amdgcn_readlane((int)rowmax_u32(hi), 15);
    L = (unsigned)__builtin_amdgcn_readlane((int)rowmax_u32(hi == H ? (unsigned)v : 0u), 15);
  }
  return ((u64)H << 32) | L;
}
// the workgroup's maximum from the waves' maxima: one LDS slot per wave (double-buffered by round parity), one barrier,
// and a 16-entry row reduction that every wave repeats (slots [2][16], zero = identity beyond the last wave)
__device__ __forceinline__ u64 block_max(u64 key, u64 *slots, int j, int t) {
  u64 *sl = slots + (j & 1) * 16;
  if ((t & 63) == 0) sl[t >> 6] = key;
  __syncthreads();
  return max_u64<false>(sl[t & 15]);
}

// The keys. High word: the running minimum's bit pattern + 1 (monotonic for floats >= 0), 0 for a thread without points
// (it carries -1), the lowest key. Low word: ~sec, sec = (k mod T) << S | k / T, the order in which a reference block of T
// threads resolves equal minima (thread t scans k = t, t + T, ... and keeps its first strict maximum, the tree keeps the
// lower thread): (minimum desc, k mod T asc, k asc), so any thread layout reproduces it. There are two encodings, and
// they do not merge:
//  * fps_key / fps_key_index: the PVCNN sampler's block is always 512 threads (every kernel of sampling.hip). S = 20,
//    9 bits above it, so sec < 2^29 and bits 29..31 of the low word stay free: fps_coop_kernel tags the round number
//    there. k < 2^29.
//  * fps_key_lt / fps_key_lt_index: T = 2^lt <= 1024 is the caller's (the reference-order kernels of fps_ref.hip).
//    S = 21, since k / T needs 21 bits at lt = 10 for any int k, and up to 10 bits above it: the low word is full, which
//    the sampler's tag could not share. These kernels read the caller's running minima, so 0 is ordered explicitly
//    (-0.0f would otherwise rank above every positive minimum).
__device__ __forceinline__ u64 fps_key(float best, int k) {
  // best >= 0 for any real point; threads without points carry best = -1 -> lowest key
  const unsigned hi = best >= 0.0f ? (__float_as_uint(best) + 1u) : 0u;
  const unsigned sec = ((unsigned)(k & 511) << 20) | (unsigned)(k >> 9);  // lower is better
  return ((u64)hi << 32) | (u64)(~sec);
}
__device__ __forceinline__ int fps_key_index(u64 key) {
  const unsigned sec = ~(unsigned)key;
  return (int)(((sec & 0xFFFFFu) << 9) | (sec >> 20));
}
// best > 0: its bit pattern + 1; 0: 1; a thread without points carries -1 -> 0
__device__ __forceinline__ u64 fps_key_lt(float best, int k, int lt) {
  const unsigned hi = best > 0.0f ? (__float_as_uint(best) + 1u) : (best == 0.0f ? 1u : 0u);
  const unsigned sec = (((unsigned)k & ((1u << lt) - 1u)) << 21) | ((unsigned)k >> lt);
  return ((u64)hi << 32) | (u64)(~sec);
}
__device__ __forceinline__ int fps_key_lt_index(u64 key, int lt) {
  const unsigned sec = ~(unsigned)key;
  return (int)(((sec & 0x1FFFFFu) << lt) | (sec >> 21));
}
