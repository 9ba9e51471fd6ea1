// scan.hip -- the device pieces of scan fusion (scan_fusion.py): depth frames -> one cleaned room cloud. Replaces what the
// reference runs through Open3D's CUDA tensor geometry and cuML (data/scannetpp/iphone/arkit_pcl.py, process_dataset.py):
//   * back-projection of the valid pixels of a depth frame (fp64, one rounding);
//   * voxel keys and per-voxel means (fp64 sums in a fixed order: sorted rows, no float atomics);
//   * a uniform-grid neighbour search over SORTED CELL KEYS: the exact radius count and the exact k-th neighbour distance.
// The grid -- cells, keys, the binary search, the run of one column, the bound of a ring -- is cell_grid.h's, the one
// p2m_grid.hip searches; the wave's list of the k best is wave_topk.h's.
// Contract: include/p2pb_hip.h, "scan fusion".
#include "common.h"

#include "cell_grid.h"
#include "wave_topk.h"

#define SCAN_BIG_CHUNK 4096  // rows of one workgroup of the large-voxel sum

// ---- back-projection -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void scan_depth_valid_kernel(int npix, const float *__restrict__ depth, float zmin,
                                                               float zmax, unsigned char *__restrict__ valid) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= npix) return;
  const float z = depth[i];
  valid[i] = (z >= zmin && z <= zmax) ? 1 : 0;  // == not (z < min or z > max or NaN or +-inf) for finite bounds
}

struct ScanCamera {
  double kinv[9];
  double c2w[12];
};

__global__ __launch_bounds__(256) void scan_backproject_kernel(int n, int width, const long long *__restrict__ pix,
                                                               const unsigned char *__restrict__ image,
                                                               const float *__restrict__ depth, ScanCamera cam,
                                                               float *__restrict__ xyz, float *__restrict__ rgb) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long p = pix[i];
  const double x = (double)(p % width), y = (double)(p / width), z = (double)depth[p];
  double c[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) c[r] = ((cam.kinv[r * 3] * x + cam.kinv[r * 3 + 1] * y) + cam.kinv[r * 3 + 2]) * z;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    xyz[(size_t)i * 3 + r] =
        (float)(((cam.c2w[r * 4] * c[0] + cam.c2w[r * 4 + 1] * c[1]) + cam.c2w[r * 4 + 2] * c[2]) + cam.c2w[r * 4 + 3]);
    rgb[(size_t)i * 3 + r] = (float)image[(size_t)p * 3 + r];
  }
}

// ---- cell keys -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void scan_cell_keys_kernel(int n, const float *__restrict__ xyz, float cell,
                                                             long long *__restrict__ keys, int *__restrict__ bad) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  bool okx, oky, okz;
  const int kx = cell_of(xyz[(size_t)i * 3], cell, &okx);
  const int ky = cell_of(xyz[(size_t)i * 3 + 1], cell, &oky);
  const int kz = cell_of(xyz[(size_t)i * 3 + 2], cell, &okz);
  keys[i] = cell_key(kx, ky, kz);
  if (!(okx && oky && okz)) *bad = 1;  // (every writer stores the same value)
}

// ---- per-voxel means -------------------------------------------------------------------------------------------------
// rows perm[starts[v] .. starts[v+1]) of src belong to voxel v, in ascending row index (stable sort). Voxels of up to `small`
// rows: one thread per (voxel, channel) adds them in that order. Larger ones are left to the chunked pair below.
__global__ __launch_bounds__(256) void scan_segment_mean_kernel(long long m, int c, int small, const float *__restrict__ src,
                                                                const long long *__restrict__ perm,
                                                                const long long *__restrict__ starts,
                                                                float *__restrict__ out) {
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  if (id >= m * c) return;
  const long long v = id / c;
  const int ch = (int)(id - v * c);
  const long long s = starts[v], e = starts[v + 1];
  if (e - s > small) return;
  double acc = 0.0;
  for (long long j = s; j < e; ++j) acc += (double)src[perm[j] * c + ch];
  out[id] = (float)(acc / (double)(e - s));
}

// one workgroup per chunk of up to SCAN_BIG_CHUNK rows of a large voxel -> partial f64[nchunks, c]. Channels are taken 256
// at a time; with cb channels in a pass, 256 / cb row slots read consecutive floats of consecutive rows, every slot adds
// its rows in ascending order, and one thread per channel adds the slots in slot order.
__global__ __launch_bounds__(256) void scan_segment_partial_kernel(int c, const float *__restrict__ src,
                                                                   const long long *__restrict__ perm,
                                                                   const long long *__restrict__ chunk_row0,
                                                                   const long long *__restrict__ chunk_rows,
                                                                   double *__restrict__ partial) {
  __shared__ double sm[256];
  const int t = threadIdx.x;
  const long long row0 = chunk_row0[blockIdx.x];
  const int rows = (int)chunk_rows[blockIdx.x];
  for (int ch0 = 0; ch0 < c; ch0 += 256) {
    const int cb = min(256, c - ch0), slots = 256 / cb;
    const int ch = t % cb, slot = t / cb;
    double acc = 0.0;
    if (slot < slots)
      for (int r = slot; r < rows; r += slots) acc += (double)src[perm[row0 + r] * c + ch0 + ch];
    sm[t] = acc;
    __syncthreads();
    if (t < cb) {
      double sum = 0.0;
      for (int g = 0; g < slots; ++g) sum += sm[g * cb + t];
      partial[(size_t)blockIdx.x * c + ch0 + t] = sum;
    }
    __syncthreads();
  }
}

// large voxel b = big[b_index]: its chunks chunk_begin[b] .. chunk_begin[b+1]) are added in chunk order
__global__ __launch_bounds__(256) void scan_segment_finish_kernel(int nbig, int c, const long long *__restrict__ big,
                                                                  const long long *__restrict__ chunk_begin,
                                                                  const long long *__restrict__ starts,
                                                                  const double *__restrict__ partial,
                                                                  float *__restrict__ out) {
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  if (id >= (long long)nbig * c) return;
  const int b = (int)(id / c), ch = (int)(id - (long long)b * c);
  const long long v = big[b];
  double sum = 0.0;
  for (long long q = chunk_begin[b]; q < chunk_begin[b + 1]; ++q) sum += partial[q * c + ch];
  out[v * c + ch] = (float)(sum / (double)(starts[v + 1] - starts[v]));
}

// ---- the grid search -------------------------------------------------------------------------------------------------
// counts[q] = min(limit, #{ j : sqdist3(p_j - q) <= r2 }) over the points sorted by cell key. One thread per query.
// Which cells: every point that can pass the fp32 test has |p_a - q_a| <= reach on each axis (reach: the radius with the
// roundings of the test added, computed by the caller), and the cell of a coordinate is monotone in the coordinate, so the
// cells of q_a - reach and q_a + reach (each moved one ulp outwards for the rounding of that sum) bracket the cells of all
// such points: the 27 cells around the query's when the cell edge is the radius, never fewer than needed.
__global__ __launch_bounds__(256) void scan_radius_count_kernel(int nq, int n, const float *__restrict__ query,
                                                                const float *__restrict__ pts,
                                                                const long long *__restrict__ keys, float cell, float r2,
                                                                float reach, int limit, int *__restrict__ counts) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  const float qp[3] = {query[(size_t)q * 3], query[(size_t)q * 3 + 1], query[(size_t)q * 3 + 2]};
  int lo[3], hi[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = max(cell_clamped(nextafterf(qp[a] - reach, -INFINITY), cell), -CELL_KEY_HALF);
    hi[a] = min(cell_clamped(nextafterf(qp[a] + reach, INFINITY), cell), CELL_KEY_HALF - 1);
  }
  int cnt = 0;
  if (lo[2] <= hi[2])
    for (int cx = lo[0]; cx <= hi[0] && cnt < limit; ++cx)
      for (int cy = lo[1]; cy <= hi[1] && cnt < limit; ++cy) {
        int s, e;
        cell_column(keys, n, cx, cy, lo[2], hi[2], s, e);
        for (int j = s; j < e && cnt < limit; ++j)
          cnt += sqdist3(pts[(size_t)j * 3] - qp[0], pts[(size_t)j * 3 + 1] - qp[1], pts[(size_t)j * 3 + 2] - qp[2]) <= r2;
      }
  counts[q] = cnt;
}

// the k <= 64 smallest squared distances a wave has seen, one per lane
typedef WaveTopk<float, 1> ScanTopk;

// offers the sorted points s..e to the wave's list
__device__ __forceinline__ void scan_topk_run(ScanTopk &best, const float *__restrict__ pts, int s, int e, float qx, float qy,
                                              float qz, int k, int lane) {
  for (int j0 = s; j0 < e; j0 += 64) {
    const int j = j0 + lane;
    float d = INFINITY;
    if (j < e) d = sqdist3(pts[(size_t)j * 3] - qx, pts[(size_t)j * 3 + 1] - qy, pts[(size_t)j * 3 + 2] - qz);
    best.offer(d, k, lane);  // (NaN distances never enter: NaN < tau is false)
  }
}

// One wave per query qidx[w] (qidx NULL: query w). Ring rho = 1..max_ring: the cube of (2 rho + 1)^3 cells around the
// query's cell, one column (2 rho + 1 cells along z = one run of the sorted points) per lane and binary-search pair, then the
// runs one after the other, 64 points per step. Every point outside the cube is at least cell_ring_bound away: the
// ring is final when the k-th best squared distance is no larger than that bound squared, which then holds for every
// unvisited point's fp32 distance too (margins 1e-6 against the 2^-22 of sqdist3). out[q] = sqrt of it, unresolved[q] = 0;
// otherwise unresolved[q] = 1 and out[q] is left alone. The list restarts with every ring (the cubes are nested).
__global__ __launch_bounds__(256) void scan_knn_grid_kernel(int nq, int n, int k, int max_ring,
                                                            const int *__restrict__ qidx, const float *__restrict__ query,
                                                            const float *__restrict__ pts,
                                                            const long long *__restrict__ keys, float cell,
                                                            float *__restrict__ out, unsigned char *__restrict__ unresolved) {
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= nq) return;
  const int lane = lane_id();
  const int q = qidx ? qidx[w] : w;
  const float qx = query[(size_t)q * 3], qy = query[(size_t)q * 3 + 1], qz = query[(size_t)q * 3 + 2];
  bool okx, oky, okz;
  const int cx = cell_of(qx, cell, &okx), cy = cell_of(qy, cell, &oky), cz = cell_of(qz, cell, &okz);
  bool done = false;
  ScanTopk best;
  if (okx && oky && okz) {  // (a query outside the key range is nobody's neighbour cell: left to the next stage)
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
          scan_topk_run(best, pts, __shfl(s, l), __shfl(e, l), qx, qy, qz, k, lane);
        }
      }
      const float reach = cell_ring_bound(rho, cmax, cell);
      done = reach > 0.0f && best.tau <= reach * reach * 0.999999f;
    }
  }
  if (lane == 0) {
    unresolved[q] = done ? 0 : 1;
    if (done) out[q] = __fsqrt_rn(best.tau);
  }
}

// brute force for the queries the rings left: one wave per query qidx[w] walks the whole cloud, 64 points per step, in the
// idiom of room.hip's radius_count_kernel. n >= k is the caller's to check.
__global__ __launch_bounds__(256) void scan_knn_brute_kernel(int nq, int n, int k, const int *__restrict__ qidx,
                                                             const float *__restrict__ query,
                                                             const float *__restrict__ pts, float *__restrict__ out) {
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= nq) return;
  const int lane = lane_id();
  const int q = qidx ? qidx[w] : w;
  ScanTopk best;
  scan_topk_run(best, pts, 0, n, query[(size_t)q * 3], query[(size_t)q * 3 + 1], query[(size_t)q * 3 + 2], k, lane);
  if (lane == 0) out[q] = __fsqrt_rn(best.tau);
}

// ---- entry points ----------------------------------------------------------------------------------------------------
extern "C" int p2pb_scan_depth_valid(int npix, const float *depth, float min_depth, float max_depth, unsigned char *valid,
                                     void *stream) {
  if (npix <= 0 || !depth || !valid || !(min_depth <= max_depth) || !(fabsf(min_depth) < INFINITY) ||
      !(fabsf(max_depth) < INFINITY))
    return P2PB_EINVAL;
  hipLaunchKernelGGL(scan_depth_valid_kernel, dim3(cdiv(npix, 256)), dim3(256), 0, (hipStream_t)stream, npix, depth,
                     min_depth, max_depth, valid);
  return p2pb_launch_status();
}

extern "C" int p2pb_scan_backproject(int n, int width, int height, const long long *pix, const unsigned char *image,
                                     const float *depth, const double *kinv, const double *camera_to_world, float *xyz,
                                     float *rgb, void *stream) {
  if (n <= 0 || width <= 0 || height <= 0 || (long long)width * height >= (1LL << 31) || !pix || !image || !depth || !kinv ||
      !camera_to_world || !xyz || !rgb)
    return P2PB_EINVAL;
  ScanCamera cam;
  for (int i = 0; i < 9; ++i) cam.kinv[i] = kinv[i];
  for (int i = 0; i < 12; ++i) cam.c2w[i] = camera_to_world[i];
  hipLaunchKernelGGL(scan_backproject_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, n, width, pix, image,
                     depth, cam, xyz, rgb);
  return p2pb_launch_status();
}

extern "C" int p2pb_scan_cell_keys(int n, const float *xyz, float cell, long long *keys, int *bad, void *stream) {
  if (n <= 0 || !xyz || !keys || !bad || !(cell > 0.0f) || !(cell < INFINITY)) return P2PB_EINVAL;
  hipLaunchKernelGGL(scan_cell_keys_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, n, xyz, cell, keys, bad);
  return p2pb_launch_status();
}

extern "C" int p2pb_scan_segment_mean(long long m, int c, int small, const float *src, const long long *perm,
                                      const long long *starts, float *out, void *stream) {
  if (m <= 0 || c <= 0 || small < 0 || m * c >= (1LL << 31) * 256 || !src || !perm || !starts || !out) return P2PB_EINVAL;
  hipLaunchKernelGGL(scan_segment_mean_kernel, dim3(cdiv(m * c, 256)), dim3(256), 0, (hipStream_t)stream, m, c, small, src,
                     perm, starts, out);
  return p2pb_launch_status();
}

extern "C" int p2pb_scan_segment_mean_big(int nbig, int nchunks, int c, const float *src, const long long *perm,
                                          const long long *starts, const long long *big, const long long *chunk_begin,
                                          const long long *chunk_row0, const long long *chunk_rows, double *partial,
                                          float *out, void *stream) {
  if (nbig <= 0 || nchunks < nbig || c <= 0 || !src || !perm || !starts || !big || !chunk_begin || !chunk_row0 ||
      !chunk_rows || !partial || !out)
    return P2PB_EINVAL;
  hipLaunchKernelGGL(scan_segment_partial_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, c, src, perm, chunk_row0,
                     chunk_rows, partial);
  hipLaunchKernelGGL(scan_segment_finish_kernel, dim3(cdiv((long long)nbig * c, 256)), dim3(256), 0, (hipStream_t)stream,
                     nbig, c, big, chunk_begin, starts, partial, out);
  return p2pb_launch_status();
}

extern "C" int p2pb_scan_big_chunk_rows(void) { return SCAN_BIG_CHUNK; }

extern "C" int p2pb_scan_radius_count(int nq, int n, const float *query, const float *sorted_points,
                                      const long long *sorted_keys, float cell, float r2, float reach, int limit,
                                      int *counts, void *stream) {
  if (nq <= 0 || n <= 0 || limit <= 0 || !query || !sorted_points || !sorted_keys || !counts || !(cell > 0.0f) ||
      !(cell < INFINITY) || !(r2 >= 0.0f) || !(reach >= 0.0f) || !(reach < INFINITY))
    return P2PB_EINVAL;
  hipLaunchKernelGGL(scan_radius_count_kernel, dim3(cdiv(nq, 256)), dim3(256), 0, (hipStream_t)stream, nq, n, query,
                     sorted_points, sorted_keys, cell, r2, reach, limit, counts);
  return p2pb_launch_status();
}

extern "C" int p2pb_scan_knn_grid(int nq, int n, int k, int max_ring, const int *qidx, const float *query,
                                  const float *sorted_points, const long long *sorted_keys, float cell, float *out,
                                  unsigned char *unresolved, void *stream) {
  if (nq <= 0 || n <= 0 || k < 1 || k > 64 || max_ring < 1 || max_ring > 16 || !query || !sorted_points || !sorted_keys ||
      !out || !unresolved || !(cell > 0.0f) || !(cell < INFINITY))
    return P2PB_EINVAL;
  hipLaunchKernelGGL(scan_knn_grid_kernel, dim3(cdiv(nq, 4)), dim3(256), 0, (hipStream_t)stream, nq, n, k, max_ring, qidx,
                     query, sorted_points, sorted_keys, cell, out, unresolved);
  return p2pb_launch_status();
}

extern "C" int p2pb_scan_knn_brute(int nq, int n, int k, const int *qidx, const float *query, const float *points, float *out,
                                   void *stream) {
  if (nq <= 0 || n <= 0 || k < 1 || k > 64 || k > n || !query || !points || !out) return P2PB_EINVAL;
  hipLaunchKernelGGL(scan_knn_brute_kernel, dim3(cdiv(nq, 4)), dim3(256), 0, (hipStream_t)stream, nq, n, k, qidx, query,
                     points, out);
  return p2pb_launch_status();
}
