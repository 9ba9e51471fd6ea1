// knn_grid.hip -- exact k nearest neighbours WITH THEIR INDICES over a whole cloud, k <= 128: the room-size form of
// p2pb_knn_points (knn.hip: one 1024-thread workgroup and 4 n bytes of scratch per query, made for a few dozen queries with k
// a whole patch). The search is scan.hip's -- rings of cells over SORTED CELL KEYS (cell_grid.h), one wave per query, the
// wave's best-list of wave_topk.h -- with the list pairs.hip keeps: keys (distance bits << 32 | original row).
//
// Why the result is p2pb_knn_points' bit for bit ("Grid k-NN"):
//   * ties. The distance is sqdist3 of common.h, a function of the (point, query) pair alone, and it is >= +0, so its bits
//     order like the floats. A key is (those bits << 32) | the point's ORIGINAL row: all keys of one query are distinct and
//     ordered by (distance, index). The k smallest of a set of distinct keys do not depend on the order in which the set is
//     visited, so the grid's order (cells, columns, sorted rows) cannot change the result.
//   * finality. Ring rho is final when tau's distance <= cell_ring_bound(rho, cmax, cell)^2 * 0.999999: every point outside the
//     cube is at least that bound away, and the margin (1e-6 against the 2^-22 of sqdist3) makes every unvisited point's fp32
//     distance STRICTLY larger than tau's. An unvisited point can therefore not tie with a kept one and carry a lower index.
// Every output is written with plain vector stores by the one wave that owns the query; no atomics: the same inputs give the
// same bits. Contract: include/p2pb_hip.h, "grid k-NN".
#include "common.h"

#include "cell_grid.h"
#include "wave_topk.h"

typedef unsigned long long u64;
#define KNN_GRID_MAXK 128

__device__ __forceinline__ u64 knn_grid_key(float d, int row) { return ((u64)__float_as_uint(d) << 32) | (unsigned)row; }

// offers the points s..e to the wave's list; rows NULL: point j is row j
template <int R>
__device__ __forceinline__ void knn_grid_run(WaveTopk<u64, R> &best, const float *__restrict__ pts,
                                             const int *__restrict__ rows, int s, int e, float qx, float qy, float qz, int k,
                                             int lane) {
  for (int j0 = s; j0 < e; j0 += 64) {
    const int j = j0 + lane;
    u64 c = ~0ull;  // (none: never below tau)
    if (j < e)
      c = knn_grid_key(sqdist3(pts[(size_t)j * 3] - qx, pts[(size_t)j * 3 + 1] - qy, pts[(size_t)j * 3 + 2] - qz),
                       rows ? rows[j] : j);
    best.offer(c, k, lane);
  }
}

// rank 64 i + lane of the list -> dist2 / idx [q, rank]
template <int R>
__device__ __forceinline__ void knn_grid_write(const WaveTopk<u64, R> &best, int q, int k, int lane, float *__restrict__ dist2,
                                               int *__restrict__ idx) {
  const size_t ob = (size_t)q * k;
#pragma unroll
  for (int i = 0; i < R; ++i)
    if (64 * i + lane < k) {
      dist2[ob + 64 * i + lane] = __uint_as_float((unsigned)(best.r[i] >> 32));
      idx[ob + 64 * i + lane] = (int)(unsigned)best.r[i];
    }
}

// One wave per query qidx[w] (qidx NULL: query w): scan.hip's scan_knn_grid_kernel with (distance, row) keys. Ring rho =
// 1..max_ring: the cube of (2 rho + 1)^3 cells around the query's cell, one column per lane and binary-search pair, then the
// runs one after the other, 64 points per step. The list restarts with every ring (the cubes are nested: a point must not
// enter twice). Resolved: the k pairs ascending, unresolved[q] = 0. Otherwise (no final ring, fewer than k points seen, a
// query cell outside the key range) unresolved[q] = 1 and the rows of q are left alone.
template <int R>
__global__ __launch_bounds__(256) void knn_grid_kernel(int nq, int n, int k, int max_ring, const int *__restrict__ qidx,
                                                       const float *__restrict__ query, const float *__restrict__ pts,
                                                       const long long *__restrict__ keys, const int *__restrict__ rows,
                                                       float cell, float *__restrict__ dist2, int *__restrict__ idx,
                                                       unsigned char *__restrict__ unresolved) {
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= nq) return;
  const int lane = lane_id();
  const int q = qidx ? qidx[w] : w;
  const float qx = query[(size_t)q * 3], qy = query[(size_t)q * 3 + 1], qz = query[(size_t)q * 3 + 2];
  bool okx, oky, okz;
  const int cx = cell_of(qx, cell, &okx), cy = cell_of(qy, cell, &oky), cz = cell_of(qz, cell, &okz);
  bool done = false;
  WaveTopk<u64, R> best;
  if (okx && oky && okz) {
    const float cmax = (float)max(max(abs(cx), abs(cy)), abs(cz));
    for (int rho = 1; rho <= max_ring && !done; ++rho) {
      best.clear();
      const int side = 2 * rho + 1, cols = side * side;
      const int z0 = max(cz - rho, -CELL_KEY_HALF), z1 = min(cz + rho, CELL_KEY_HALF - 1);
      for (int c0 = 0; c0 < cols; c0 += 64) {
        const int col = c0 + lane;
        int s = 0, e = 0;
        if (col < cols) {
          const int x = cx - rho + col / side, y = cy - rho + col % side;
          if (x >= -CELL_KEY_HALF && x < CELL_KEY_HALF && y >= -CELL_KEY_HALF && y < CELL_KEY_HALF)
            cell_column(keys, n, x, y, z0, z1, s, e);
        }
        unsigned long long live = __ballot(e > s);
        while (live) {
          const int l = __ffsll((long long)live) - 1;
          live &= live - 1;
          knn_grid_run<R>(best, pts, rows, __shfl(s, l), __shfl(e, l), qx, qy, qz, k, lane);
        }
      }
      const float reach = cell_ring_bound(rho, cmax, cell);
      // (tau still empty = fewer than k points seen: its distance bits are a NaN, and the ring is not final)
      done = reach > 0.0f && best.tau != ~0ull && __uint_as_float((unsigned)(best.tau >> 32)) <= reach * reach * 0.999999f;
    }
  }
  if (lane == 0) unresolved[q] = done ? 0 : 1;
  if (done) knn_grid_write<R>(best, q, k, lane, dist2, idx);
}

// the same list from a walk over all n points in their original order, for the queries the rings left: one wave per query
// qidx[w], in the idiom of scan.hip's scan_knn_brute_kernel. n >= k is the entry point's to check.
template <int R>
__global__ __launch_bounds__(256) void knn_grid_brute_kernel(int nq, int n, int k, const int *__restrict__ qidx,
                                                             const float *__restrict__ query, const float *__restrict__ pts,
                                                             float *__restrict__ dist2, int *__restrict__ idx) {
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= nq) return;
  const int lane = lane_id();
  const int q = qidx ? qidx[w] : w;
  WaveTopk<u64, R> best;
  knn_grid_run<R>(best, pts, nullptr, 0, n, query[(size_t)q * 3], query[(size_t)q * 3 + 1], query[(size_t)q * 3 + 2], k, lane);
  knn_grid_write<R>(best, q, k, lane, dist2, idx);
}

// ---- entry points ----------------------------------------------------------------------------------------------------
extern "C" int p2pb_knn_grid(int nq, int n, int k, int max_ring, const int *qidx, const float *query,
                             const float *sorted_points, const long long *sorted_keys, const int *rows, float cell,
                             float *dist2, int *idx, unsigned char *unresolved, void *stream) {
  if (nq <= 0 || n <= 0 || k < 1 || k > KNN_GRID_MAXK || k > n || max_ring < 1 || max_ring > 16 || !query || !sorted_points ||
      !sorted_keys || !rows || !dist2 || !idx || !unresolved || !(cell > 0.0f) || !(cell < INFINITY))
    return P2PB_EINVAL;
  if (k <= 64)
    hipLaunchKernelGGL(knn_grid_kernel<1>, dim3(cdiv(nq, 4)), dim3(256), 0, (hipStream_t)stream, nq, n, k, max_ring, qidx,
                       query, sorted_points, sorted_keys, rows, cell, dist2, idx, unresolved);
  else
    hipLaunchKernelGGL(knn_grid_kernel<2>, dim3(cdiv(nq, 4)), dim3(256), 0, (hipStream_t)stream, nq, n, k, max_ring, qidx,
                       query, sorted_points, sorted_keys, rows, cell, dist2, idx, unresolved);
  return p2pb_launch_status();
}

extern "C" int p2pb_knn_grid_brute(int nq, int n, int k, const int *qidx, const float *query, const float *points,
                                   float *dist2, int *idx, void *stream) {
  if (nq <= 0 || n <= 0 || k < 1 || k > KNN_GRID_MAXK || k > n || !query || !points || !dist2 || !idx) return P2PB_EINVAL;
  if (k <= 64)
    hipLaunchKernelGGL(knn_grid_brute_kernel<1>, dim3(cdiv(nq, 4)), dim3(256), 0, (hipStream_t)stream, nq, n, k, qidx, query,
                       points, dist2, idx);
  else
    hipLaunchKernelGGL(knn_grid_brute_kernel<2>, dim3(cdiv(nq, 4)), dim3(256), 0, (hipStream_t)stream, nq, n, k, qidx, query,
                       points, dist2, idx);
  return p2pb_launch_status();
}
