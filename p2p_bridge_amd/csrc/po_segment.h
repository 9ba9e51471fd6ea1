// po_segment.h -- the point range of a segment of a packed cloud (pointops.hip, fps_ref.hip): cumulative ends offset i32[b],
// clamped to [0, n] whatever the array holds; an end below its start is an empty segment.
#pragma once
#include "common.h"

__device__ __forceinline__ int po_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// (The test and ONE address for both ends are spelled out, in this order: written as offset[s - 1] and offset[s], whether
//  the compiler shares the address depends on how many callers the translation unit has, and the searches of pointops.hip
//  get another register allocation -- ball query 5 % slower -- when this helper has no second caller there.)
__device__ __forceinline__ void po_segment_points(int s, int n, const int *__restrict__ offset, int &start, int &end) {
  const bool inner = s != 0;
  const int *__restrict__ o = offset + s;
  start = inner ? po_clamp(o[-1], 0, n) : 0;
  end = po_clamp(o[0], start, n);
}
