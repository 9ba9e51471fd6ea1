// wave_topk.h -- the k <= 64 R smallest keys a wave has seen, held in registers: rank 64 i + l lives in r[i] of lane l.
// Invariants: ascending over ranks; empty = the type's maximum (+inf for float); tau = the key of rank k - 1, wave-uniform;
// a candidate goes in behind its equals (position = the count of keys <= it), so equal keys stay in the order they came.
// Users: scan.hip (squared distances, <float, 1>), pairs.hip (distance bits << 32 | index, all different, <u64, 2>) and
// knn_grid.hip (the same keys over a whole cloud, <u64, 1> up to k = 64 and <u64, 2> above).
#pragma once
#include <limits>

template <class T, int R> struct WaveTopk {
  typedef std::numeric_limits<T> Lim;
  T r[R];
  T tau;

  __device__ __forceinline__ WaveTopk() { clear(); }
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int i = 0; i < R; ++i) r[i] = Lim::has_infinity ? Lim::infinity() : Lim::max();
    tau = r[0];
  }

  // v: wave-uniform and below tau
  __device__ __forceinline__ void insert(T v, int k, int lane) {
    int pos = 0;  // (< k: the key of rank k - 1 is tau > v)
#pragma unroll
    for (int i = 0; i < R; ++i) pos += __popcll(__ballot(r[i] <= v));
#pragma unroll
    for (int i = R - 1; i >= 0; --i) {  // downwards: lane 0 takes rank 64 i - 1 from the register below before that shifts
      T up = __shfl_up(r[i], 1);
      if (i > 0) {
        const T below = __shfl(r[i - 1], 63);
        if (lane == 0) up = below;
      }
      const int rank = 64 * i + lane;
      r[i] = rank < pos ? r[i] : (rank == pos ? v : up);
    }
#pragma unroll
    for (int i = 0; i < R; ++i)
      if (R == 1 || (k - 1) >> 6 == i) tau = __shfl(r[i], k - 1 - 64 * i);
  }

  // every lane offers one candidate c (the type's maximum, or NaN: none). Those below tau are inserted one at a time, in lane
  // order; after the first few steps of a stream almost none is.
  __device__ __forceinline__ void offer(T c, int k, int lane) {
    unsigned long long todo = __ballot(c < tau);
    while (todo) {
      const int src = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const T v = __shfl(c, src);
      if (v < tau) insert(v, k, lane);
    }
  }
};
