// cloud_layout.h -- the two memory layouts of a batch element's triples (a cloud's coordinates, or the three (index, weight)
// pairs of an interpolation), as the compile-time parameter of the kernels that serve both operator families
// (ball_query.hip, three_nn.hip):
//   ChannelMajor<T>  T[3][count]   the PVCNN operators' clouds f32[B,3,N], idx / weights [B,3,N]; also LDS planes
//   PointMajor<T>    T[count][3]   the classic pointnet2_batch operators' clouds f32[B,N,3], idx / weights [B,N,3]
// load(k, x, y, z) reads triple k. stage() copies the whole cloud into three LDS planes of `count` elements, stage_tile()
// triples k0 .. k0 + kn - 1 into planes of `pitch` elements; all `nthreads` threads of the workgroup call them, with
// lane-consecutive reads, and the caller puts the barriers round them. The objects hold a pointer and a count and
// dissolve into the kernel's own address arithmetic.
#pragma once
#include "common.h"

template <class T>
struct ChannelMajor {
  const T *p;
  int count;
  __device__ __forceinline__ void load(int k, T &x, T &y, T &z) const {
    x = p[k];
    y = p[k + count];
    z = p[k + 2 * count];
  }
  __device__ __forceinline__ void stage(T *planes, int nthreads) const {  // planes of `count`: the cloud as it lies
    for (int k = threadIdx.x; k < 3 * count; k += nthreads) planes[k] = p[k];
  }
  __device__ __forceinline__ void stage_tile(T *planes, int pitch, int k0, int kn, int nthreads) const {
    for (int k = threadIdx.x; k < kn; k += nthreads) {
      planes[k] = p[k0 + k];
      planes[pitch + k] = p[k0 + k + count];
      planes[2 * pitch + k] = p[k0 + k + 2 * count];
    }
  }
};

template <class T>
struct PointMajor {
  const T *p;
  int count;
  __device__ __forceinline__ void load(int k, T &x, T &y, T &z) const {
    x = p[(size_t)3 * k];
    y = p[(size_t)3 * k + 1];
    z = p[(size_t)3 * k + 2];
  }
  __device__ __forceinline__ void stage(T *planes, int nthreads) const { stage_tile(planes, count, 0, count, nthreads); }
  __device__ __forceinline__ void stage_tile(T *planes, int pitch, int k0, int kn, int nthreads) const {
    for (int k = threadIdx.x; k < 3 * kn; k += nthreads) planes[(k % 3) * pitch + k / 3] = p[(size_t)3 * k0 + k];
  }
};
