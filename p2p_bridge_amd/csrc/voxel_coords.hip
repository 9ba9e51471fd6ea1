// voxel_coords.hip -- the coordinate half of the point -> voxel kernels for gfx950 (the feature half: voxel_gather.hip).
//   p2pb_voxel_coords  (models/pvcnn.py:215-228)
//   p2pb_voxel_sort    occupancy counts + per-voxel sorted point lists (the first four steps of PN2/vox_gpu.cu:18,50)
#include "voxel_common.h"

// ------------------------------------------------------------------------------------------------
// voxel_coords: one workgroup per cloud. Summation order is part of the contract (see oracle):
// 256 lane-strided double partials, then a fixed binary tree.
// ------------------------------------------------------------------------------------------------
// (round 5: since the level-0 preparation runs on the sampler's main stream this kernel is on the critical path. The first form --
//  256 threads, 32 dependent load + add steps per axis, then two more strided passes -- took 44-63 us for 98 KB per cloud. Now 1024
//  threads; the 256 partials are summed by threads 0..255 in the SAME order, their loads issued eight at a time; the maximum and
//  the normalisation pass, which have no order, use every thread.)
__global__ __launch_bounds__(1024) void voxel_coords_kernel(int n, int r, int normalize, float eps,
                                                            const float *__restrict__ coords,
                                                            float *__restrict__ norm, int *__restrict__ vox) {
  __shared__ double part[3][256];
  __shared__ float smax[1024];
  const int t = threadIdx.x;
  const float *c = coords + (size_t)blockIdx.x * 3 * n;
  float *o = norm + (size_t)blockIdx.x * 3 * n;
  int *v = vox + (size_t)blockIdx.x * 3 * n;
  if (t < 256) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int k0 = t; k0 < n; k0 += 8 * 256) {
      float x0[8], x1[8], x2[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int k = k0 + u * 256;
        const bool ok = k < n;
        x0[u] = ok ? c[k] : 0.0f;
        x1[u] = ok ? c[n + k] : 0.0f;
        x2[u] = ok ? c[2 * n + k] : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (k0 + u * 256 < n) {
          s0 += (double)x0[u];
          s1 += (double)x1[u];
          s2 += (double)x2[u];
        }
    }
    part[0][t] = s0;
    part[1][t] = s1;
    part[2][t] = s2;
  }
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      part[0][t] += part[0][t + s];
      part[1][t] += part[1][t + s];
      part[2][t] += part[2][t + s];
    }
    __syncthreads();
  }
  const float m0 = (float)(part[0][0] / (double)n);
  const float m1 = (float)(part[1][0] / (double)n);
  const float m2 = (float)(part[2][0] / (double)n);
  float mx = 0.0f;
#pragma unroll 4
  for (int k = t; k < n; k += 1024) {
    float s = sqdist3(c[k] - m0, c[n + k] - m1, c[2 * n + k] - m2);
    mx = s > mx ? s : mx;
  }
  smax[t] = mx;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {  // (a maximum: exact in any order)
    if (t < s) smax[t] = smax[t + s] > smax[t] ? smax[t + s] : smax[t];
    __syncthreads();
  }
  const float denom = sqrtf(smax[0]) * 2.0f + eps;  // sqrtf: correctly rounded (IEEE) under hipcc's default; __fsqrt_rn maps to the 1-ulp native v_sqrt_f32 (found at N = 12500: 40 % of the voxel coordinates one ulp off)
  const float mean[3] = {m0, m1, m2};
  const float rf = (float)r, hi = (float)(r - 1);
  for (int a = 0; a < 3; ++a)
#pragma unroll 4
    for (int k = t; k < n; k += 1024) {
      float x = c[a * n + k] - mean[a];
      if (normalize)
        x = __fdiv_rn(x, denom) + 0.5f;
      else
        x = __fdiv_rn(x + 1.0f, 2.0f);
      x = x * rf;
      x = fminf(fmaxf(x, 0.0f), hi);
      o[a * n + k] = x;
      v[a * n + k] = (int)rintf(x);
    }
}

extern "C" int p2pb_voxel_coords(int b, int n, int r, int normalize, float eps, const float *coords, float *norm,
                                 int *vox, void *stream) {
  if (b <= 0 || n <= 0 || r <= 0) return P2PB_EINVAL;
  hipLaunchKernelGGL(voxel_coords_kernel, dim3(b), dim3(1024), 0, (hipStream_t)stream, n, r, normalize, eps, coords,
                     norm, vox);
  return p2pb_launch_status();
}

// ------------------------------------------------------------------------------------------------
// avg_voxelize forward, deterministic (each voxel sums its points in ascending point index):
//   1 count  : ind[i] = x*r2 + y*r + z ; cnt[ind]++                    (int atomics: order independent)
//   2 scan   : cur[v] = exclusive prefix of cnt; occ[] = compacted list of non-empty voxels, nocc
//   3 fill   : list[cur[v]++] = i                                     (order inside a voxel arbitrary ...)
//   4 sort   : ... one WAVE per non-empty voxel ranks its ids by counting and writes slist[] ascending
// and, in voxel_gather.hip:
//   5 zero   : the dense [C, r^3] grid is streamed out as zeros (16-byte stores; the dominant HBM traffic:
//              a PU-Net patch occupies only ~2-3 % of a 32^3 grid)
//   6 gather : one wave per non-empty voxel, lane = channel: acc += feat[c, p] * (1/cnt) over the voxel's
//              points in ascending order, then out[c, v] = acc
// The point cloud of a patch is a 2-manifold, so a voxel that is occupied holds ~10 points (8192 points
// over ~800 voxels at r = 32): work is organised per occupied voxel, not per voxel.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vox_count_kernel(int n, int r, const int *__restrict__ coords,
                                                        int *__restrict__ ind, int *__restrict__ cnt) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int *c = coords + (size_t)b * 3 * n;
  const int v = c[i] * r * r + c[i + n] * r + c[i + 2 * n];
  ind[(size_t)b * n + i] = v;
  atomicAdd(cnt + (size_t)b * r * r * r + v, 1);
}

// block-wide exclusive scan of one int per thread (1024 threads); returns the exclusive prefix, total in *tot
__device__ __forceinline__ int block_exscan_1024(int x, int *wsum, int *tot) {
  const int t = threadIdx.x;
  int inc = x;
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(inc, d);
    if ((t & 63) >= d) inc += y;
  }
  __syncthreads();  // wsum may still be read from a previous call
  if ((t & 63) == 63) wsum[t >> 6] = inc;
  __syncthreads();
  int base = 0, all = 0;
  for (int w = 0; w < 16; ++w) {
    if (w < (t >> 6)) base += wsum[w];
    all += wsum[w];
  }
  *tot = all;
  return base + inc - x;
}

__global__ __launch_bounds__(1024) void vox_scan_kernel(int n, int r3, const int *__restrict__ cnt,
                                                        int *__restrict__ cur, int *__restrict__ occ,
                                                        int *__restrict__ nocc) {
  __shared__ int wsum[16];
  const int t = threadIdx.x;
  const int *c = cnt + (size_t)blockIdx.x * r3;
  int *o = cur + (size_t)blockIdx.x * r3;
  int *oc = occ + (size_t)blockIdx.x * n;
  const int per = (r3 + 1023) / 1024;
  const int beg = t * per, end = min(beg + per, r3);
  int tot;
  if (per == 32 && r3 == 32768) {  // r = 32: a thread's 32 counts in registers (eight 16-byte loads, issued together) -- the two
    // scalar passes of the general form were 64 dependent 4-byte loads at a 128-byte lane stride (55 us per launch)
    i32x4 x[8];
    const i32x4 *c4 = (const i32x4 *)(c + beg);
#pragma unroll
    for (int q = 0; q < 8; ++q) x[q] = c4[q];
    int s = 0, k = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s += x[q][i];
        k += x[q][i] > 0;
      }
    int run = block_exscan_1024(s, wsum, &tot);
    int kpos = block_exscan_1024(k, wsum, &tot);
    if (t == 0) nocc[blockIdx.x] = tot;
    i32x4 *o4 = (i32x4 *)(o + beg);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      i32x4 w;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        w[i] = run;
        run += x[q][i];
        if (x[q][i] > 0) oc[kpos++] = beg + 4 * q + i;
      }
      o4[q] = w;
    }
    return;
  }
  int s = 0, k = 0;
  for (int v = beg; v < end; ++v) {
    const int x = c[v];
    s += x;
    k += x > 0;
  }
  int run = block_exscan_1024(s, wsum, &tot);
  int kpos = block_exscan_1024(k, wsum, &tot);
  if (t == 0) nocc[blockIdx.x] = tot;
  for (int v = beg; v < end; ++v) {
    const int x = c[v];
    o[v] = run;
    run += x;
    if (x > 0) oc[kpos++] = v;
  }
}

__global__ __launch_bounds__(256) void vox_fill_kernel(int n, int r3, const int *__restrict__ ind,
                                                       int *__restrict__ cur, int *__restrict__ list) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int v = ind[(size_t)b * n + i];
  const int pos = atomicAdd(cur + (size_t)b * r3 + v, 1);
  list[(size_t)b * n + pos] = i;
}

// one wave per non-empty voxel: slist[start + rank(id)] = id, rank by counting (ids are distinct)
__global__ __launch_bounds__(256) void vox_sort_kernel(int n, int r3, const int *__restrict__ cnt,
                                                       const int *__restrict__ cur, const int *__restrict__ occ,
                                                       const int *__restrict__ nocc, const int *__restrict__ list,
                                                       int *__restrict__ slist) {
  const int b = blockIdx.y;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= nocc[b]) return;
  const int lane = lane_id();
  const int v = occ[(size_t)b * n + k];
  const int cn = cnt[(size_t)b * r3 + v];
  const int start = cur[(size_t)b * r3 + v] - cn;  // cur points at the segment end after the fill
  const int *seg = list + (size_t)b * n + start;
  int *dst = slist + (size_t)b * n + start;
  if (cn <= 64) {  // the usual case: the ids sit in the lanes, ranks through lane broadcasts (no load inside the loop)
    const int mine = lane < cn ? seg[lane] : 0x7fffffff;
    int rank = 0;
    for (int j = 0; j < cn; ++j) rank += __shfl(mine, j) < mine;
    if (lane < cn) dst[rank] = mine;
    return;
  }
  for (int l0 = 0; l0 < cn; l0 += 64) {
    const int l = l0 + lane;
    const int mine = l < cn ? seg[l] : 0x7fffffff;
    int rank = 0;
    for (int j = 0; j < cn; ++j) rank += seg[j] < mine;  // wave-uniform address: one broadcast load
    if (l < cn) dst[rank] = mine;
  }
}

extern "C" size_t p2pb_avg_voxelize_ws_bytes(int b, int n, int r) { return vox_ws_carve(nullptr, b, n, r * r * r, nullptr); }

// The coordinate-only half of the voxelisation (occupancy counts + per-voxel sorted point lists): it depends on
// the voxel coordinates alone, so the sampler runs it once per (level, resolution) on the geometry stream and every
// PVConv of that level reuses it. ws: p2pb_avg_voxelize_ws_bytes(b,n,r) bytes, consumed by the gathers of voxel_gather.hip.
extern "C" int p2pb_voxel_sort(int b, int n, int r, const int *coords, int *ind, int *cnt, void *ws, void *stream) {
  if (b <= 0 || n <= 0 || r <= 0 || !ws) return P2PB_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int r3 = r * r * r;
  VoxWs w;
  vox_ws_carve(ws, b, n, r3, &w);
  int e = p2pb_zero_async(cnt, sizeof(int) * (size_t)b * r3, s);
  if (e != 0) return e;
  hipLaunchKernelGGL(vox_count_kernel, dim3(cdiv(n, 256), b), dim3(256), 0, s, n, r, coords, ind, cnt);
  hipLaunchKernelGGL(vox_scan_kernel, dim3(b), dim3(1024), 0, s, n, r3, cnt, w.cur, w.occ, w.nocc);
  hipLaunchKernelGGL(vox_fill_kernel, dim3(cdiv(n, 256), b), dim3(256), 0, s, n, r3, ind, w.cur, w.list);
  const int maxocc = n < r3 ? n : r3;
  hipLaunchKernelGGL(vox_sort_kernel, dim3(cdiv(maxocc, 4), b), dim3(256), 0, s, n, r3, cnt, w.cur, w.occ, w.nocc, w.list,
                     w.slist);
  return p2pb_launch_status();
}
