// cell_grid.h -- the uniform grid held as SORTED CELL KEYS, stated once for its users: scan.hip (voxel keys, radius count,
// k-th neighbour), p2m_grid.hip (point <-> mesh search), knn_grid.hip (k nearest neighbours with indices) and nn_grid.hip
// (the nearest point, one lane per query). The grid is
// nothing but a set of entries sorted by the packed key of their cell (torch sorts; memory O(n), whatever the bounding box):
// the cells (x, y, z0..z1) of one column are consecutive keys, so one column of a neighbourhood is ONE contiguous run of the
// sorted entries, found by two binary searches.
// Whoever writes keys (p2pb_scan_cell_keys, p2pb_p2m_grid_fill) and whoever looks them up goes through these definitions, so
// the two sides cannot drift apart. Key format: include/p2pb_hip.h, "scan fusion".
#pragma once

#define CELL_KEY_HALF 1048576  // 2^20: cell indices lie in [-2^20, 2^20), three of them pack into 63 bits

// floor of the IEEE fp32 quotient (so -0.001 lies in cell -1). Monotone in p for a positive cell size: the searches lean on it.
__device__ __forceinline__ float cell_quotient(float p, float cell) { return floorf(__fdiv_rn(p, cell)); }

// the cell of a coordinate; *ok = false outside [-2^20, 2^20) (NaN included)
__device__ __forceinline__ int cell_of(float p, float cell, bool *ok) {
  const float q = cell_quotient(p, cell);
  *ok = q >= -(float)CELL_KEY_HALF && q < (float)CELL_KEY_HALF;
  return *ok ? (int)q : 0;
}

// the cell of a query coordinate, clamped to one cell beyond the key range (nothing lives there)
__device__ __forceinline__ int cell_clamped(float p, float cell) {
  const float q = cell_quotient(p, cell);
  return (int)fminf(fmaxf(q, -(float)CELL_KEY_HALF - 1.0f), (float)CELL_KEY_HALF);  // (NaN -> the lower clamp)
}

__device__ __forceinline__ long long cell_key(int kx, int ky, int kz) {
  return ((long long)(kx + CELL_KEY_HALF) << 42) | ((long long)(ky + CELL_KEY_HALF) << 21) | (long long)(kz + CELL_KEY_HALF);
}

// first index in the ascending keys[lo..n) whose key is >= key
__device__ __forceinline__ int cell_lower_bound(const long long *__restrict__ keys, int lo, int n, long long key) {
  int hi = n;
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the run [s, e) of the sorted keys[0..n) that holds the cells (x, y, z0..z1) of one column; x, y, z0 <= z1 within the range
__device__ __forceinline__ void cell_column(const long long *__restrict__ keys, int n, int x, int y, int z0, int z1, int &s,
                                            int &e) {
  s = cell_lower_bound(keys, 0, n, cell_key(x, y, z0));
  e = cell_lower_bound(keys, s, n, cell_key(x, y, z1) + 1);
}

// Everything outside the cube of ring rho around cells of magnitude <= cmax lies in a cell at least rho + 1 away on some axis,
// hence at least rho cell edges from the query, less the rounding of the two fp32 quotients (2^-23 of the cell indices), with a
// margin of 1e-6: the distance below which ring rho is final.
__device__ __forceinline__ float cell_ring_bound(int rho, float cmax, float cell) {
  return (((float)rho - 1.1920929e-7f * (cmax + (float)rho + 2.0f)) * cell) * 0.999999f;
}
