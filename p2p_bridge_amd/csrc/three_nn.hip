// three_nn.hip -- three-nearest-neighbour search and interpolation of both operator families:
//   p2pb_three_nn, p2pb_three_nn_cells, p2pb_three_interpolate, p2pb_three_nn_interpolate_forward
//                                    (PN2/pvcnn_neighbor_interpolate_gpu.cu:20,96)  clouds f32[B,3,N], idx / weights [B,3,N]
//   p2pb_pn2_three_nn                (PN2/interpolate_gpu.cu:16)    clouds f32[B,N,3], dist2 / idx [B,N,3]
//   p2pb_pn2_three_interpolate       (PN2/interpolate_gpu.cu:84)    idx / weight [B,N,3]
//   p2pb_pn2_three_interpolate_grad  (PN2/interpolate_gpu.cu:127)   ADDS into its target
// (PN2 = third_party/openpoints/cpp/pointnet2_batch/src. The caller owns every output. The other classic operators:
// p2pb_pn2_ball_query in ball_query.hip, p2pb_pn2_fps in fps_ref.hip; group_points* / gather_points* have the layout and
// arithmetic of p2pb_grouping_* / p2pb_gather_features_* (neighbors.hip, scatter_grad.hip) and are routed there by the
// Python module. Backward of the PVCNN interpolation: scatter_grad.hip; the interpolation fused with the skip
// connection's add: three_interp_add_kernel, neighbors.hip.)
// The reference runs ONE thread block per cloud; here every kernel is spread over points x channels x batch.
// Squared distances are sqdist3 (common.h), as everywhere in the library.
#include "cloud_layout.h"

// sorted insertion of candidate (d, k) into the three bests, strict '<': among equal distances the earlier candidate
// ranks first. Six named scalars: as an array or a struct indexed at run time the bests become a scratch array.
__device__ __forceinline__ void nn3_insert(float d, int k, float &best0, float &best1, float &best2, int &i0, int &i1,
                                           int &i2) {
  if (d < best2) {
    best2 = d;
    i2 = k;
    if (d < best1) {
      best2 = best1;
      i2 = i1;
      best1 = d;
      i1 = k;
      if (d < best0) {
        best1 = best0;
        i1 = i0;
        best0 = d;
        i0 = k;
      }
    }
  }
}

// inverse-squared-distance weights of query j of a cloud of n: w f32[3][n], id i32[3][n] (this cloud's planes)
__device__ __forceinline__ void nn3_store_weights(float best0, float best1, float best2, int i0, int i1, int i2,
                                                  float *w, int *id, int j, int n) {
  best0 = fmaxf(fminf(1e10f, best0), 1e-10f);
  best1 = fmaxf(fminf(1e10f, best1), 1e-10f);
  best2 = fmaxf(fminf(1e10f, best2), 1e-10f);
  const float d0d1 = best0 * best1, d0d2 = best0 * best2, d1d2 = best1 * best2;
  const float inv = __fdiv_rn(1.0f, d0d1 + d0d2 + d1d2);
  w[j] = d1d2 * inv;
  id[j] = i0;
  w[j + n] = d0d2 * inv;
  id[j + n] = i1;
  w[j + 2 * n] = d0d1 * inv;
  id[j + 2 * n] = i2;
}

// ------------------------------------------------------------------------------------------------
// Brute force: one thread per query point, the centre coordinates are staged through LDS in tiles, as three planes, and
// read back as wave-wide broadcasts. Strict '<' in ascending k: among equal distances the lower index ranks first.
// The reference keeps its three bests as doubles initialised to 1e40 (never reached by an fp32 distance; its float
// store turns it into +inf): +inf in fp32 takes exactly the same branches and clamps to the same 1e10f.
//   WEIGHTS (PVCNN): out = weights f32[b,3,n], indices i32[b,3,n]
//   else (PN2):      out = dist2 f32[b,n,3], indices i32[b,n,3]; for m < 3 the unfilled slots are idx 0, dist2 +inf
// ------------------------------------------------------------------------------------------------
#define NN_TILE 2048
template <class Cloud, bool WEIGHTS>
__global__ __launch_bounds__(256) void three_nn_kernel(int n, int m, const float *__restrict__ points,
                                                       const float *__restrict__ centers, float *__restrict__ out,
                                                       int *__restrict__ indices) {
  __shared__ float sc[3][NN_TILE];
  const int b = blockIdx.y;
  const int j = blockIdx.x * 256 + threadIdx.x;
  const Cloud pts{points + (size_t)b * 3 * n, n}, ctr{centers + (size_t)b * 3 * m, m};
  const bool ok = j < n;
  float ux = 0.0f, uy = 0.0f, uz = 0.0f;
  if (ok) pts.load(j, ux, uy, uz);
  float best0 = INFINITY, best1 = INFINITY, best2 = INFINITY;
  int i0 = 0, i1 = 0, i2 = 0;
  for (int k0 = 0; k0 < m; k0 += NN_TILE) {
    const int kn = min(NN_TILE, m - k0);
    __syncthreads();
    ctr.stage_tile(&sc[0][0], NN_TILE, k0, kn, 256);
    __syncthreads();
    for (int k = 0; k < kn; ++k)
      nn3_insert(sqdist3(ux - sc[0][k], uy - sc[1][k], uz - sc[2][k]), k0 + k, best0, best1, best2, i0, i1, i2);
  }
  if (!ok) return;
  if (WEIGHTS) {
    nn3_store_weights(best0, best1, best2, i0, i1, i2, out + (size_t)b * 3 * n, indices + (size_t)b * 3 * n, j, n);
  } else {
    float *d = out + ((size_t)b * n + j) * 3;
    int *id = indices + ((size_t)b * n + j) * 3;
    d[0] = best0;
    d[1] = best1;
    d[2] = best2;
    id[0] = i0;
    id[1] = i1;
    id[2] = i2;
  }
}

// the search depends on coordinates only, so the sampler runs it on a side stream (geometry pipeline) while the feature
// path is still busy
extern "C" int p2pb_three_nn(int b, int m, int n, const float *points, const float *centers, int *idx, float *w,
                             void *stream) {
  if (b <= 0 || n <= 0 || m <= 0) return P2PB_EINVAL;
  hipLaunchKernelGGL((three_nn_kernel<ChannelMajor<float>, true>), dim3(cdiv(n, 256), b), dim3(256), 0,
                     (hipStream_t)stream, n, m, points, centers, w, idx);
  return p2pb_launch_status();
}

extern "C" int p2pb_pn2_three_nn(int b, int n, int m, const float *unknown, const float *known, float *dist2, int *idx,
                                 void *stream) {
  if (b <= 0 || b > 65535 || n <= 0 || m <= 0 || !unknown || !known || !dist2 || !idx) return P2PB_EINVAL;
  hipLaunchKernelGGL((three_nn_kernel<PointMajor<float>, false>), dim3(cdiv(n, 256), b), dim3(256), 0,
                     (hipStream_t)stream, n, m, unknown, known, dist2, idx);
  return p2pb_launch_status();
}

// ------------------------------------------------------------------------------------------------
// The same search through a uniform grid over the centres (exact): brute force evaluates n x m pairs (537 M per call
// at the first level; ~190 us of pure instruction issue, more beside the main stream), the grid ~50 per point.
//   nn_cells_build : one workgroup per cloud. Cubic cells of edge h = (largest bounding-box extent of the centres) /
//                    NNC_G; count (LDS atomics) -> exclusive scan -> fill -> every cell's short id list sorted
//                    ascending. cell_start i32[b][G^3 + 1], cell_ids i32[b][m], box f32[b][4] = (min x, y, z, h).
//   three_nn_cells : one thread per point, the cloud's records + cell table in LDS: visit the cells within Chebyshev
//                    radius rho of the point's (clamped) cell, rho = 1 (the 3x3x3 block), 2, ... (one more shell
//                    each); every centre outside is farther than rho * h, so the search stops as
//                    soon as three are held and the third distance is <= (rho h)^2. Candidates arrive out of index
//                    order, so ties are broken explicitly (smaller index first) -- what "first strict minimum in
//                    ascending index" gives the brute-force kernel. Same distances (sqdist3), same weights.
// ------------------------------------------------------------------------------------------------
#define NNC_G 16
#define NNC_CELLS (NNC_G * NNC_G * NNC_G)

__global__ __launch_bounds__(1024) void nn_cells_build_kernel(int m, const float *__restrict__ centers,
                                                              int *__restrict__ cell_start, int *__restrict__ cell_ids,
                                                              float4 *__restrict__ cell_rec, float *__restrict__ box) {
  __shared__ int cnt[NNC_CELLS];
  __shared__ int part[1024];
  __shared__ float red[6][16];
  __shared__ float sbox[4];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const float *ce = centers + (size_t)b * 3 * m;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int k = t; k < m; k += 1024)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float v = ce[k + a * m];
      lo[a] = fminf(lo[a], v);
      hi[a] = fmaxf(hi[a], v);
    }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo[a] = fminf(lo[a], __shfl_xor(lo[a], o));
      hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o));
    }
    if (lane == 0) {
      red[a][wave] = lo[a];
      red[3 + a][wave] = hi[a];
    }
  }
  for (int i = t; i < NNC_CELLS; i += 1024) cnt[i] = 0;
  __syncthreads();
  if (t == 0) {
    float mn[3], ext = 0.0f;
    for (int a = 0; a < 3; ++a) {
      float l = INFINITY, h = -INFINITY;
      for (int w = 0; w < 16; ++w) {
        l = fminf(l, red[a][w]);
        h = fmaxf(h, red[3 + a][w]);
      }
      mn[a] = l;
      ext = fmaxf(ext, h - l);
    }
    const float hcell = fmaxf(ext, 1e-12f) / NNC_G;
    for (int a = 0; a < 3; ++a) {
      sbox[a] = mn[a];
      box[(size_t)b * 4 + a] = mn[a];
    }
    sbox[3] = hcell;
    box[(size_t)b * 4 + 3] = hcell;
  }
  __syncthreads();
  const float inv = 1.0f / sbox[3];
  auto cell_of = [&](int k) {
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = min(max((int)floorf((ce[k + a * m] - sbox[a]) * inv), 0), NNC_G - 1);
    return (c[2] * NNC_G + c[1]) * NNC_G + c[0];
  };
  for (int k = t; k < m; k += 1024) atomicAdd(&cnt[cell_of(k)], 1);
  __syncthreads();
  // exclusive scan of the 4096 counts: thread t owns cells 4t .. 4t+3
  int c4[4], tot = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    c4[i] = cnt[4 * t + i];
    tot += c4[i];
  }
  part[t] = tot;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int v = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = part[t] - tot;
  int *cs = cell_start + (size_t)b * (NNC_CELLS + 1);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    cs[4 * t + i] = run;
    cnt[4 * t + i] = run;  // becomes the fill cursor
    run += c4[i];
  }
  if (t == 1023) cs[NNC_CELLS] = run;
  __syncthreads();
  int *ids = cell_ids + (size_t)b * m;
  for (int k = t; k < m; k += 1024) ids[atomicAdd(&cnt[cell_of(k)], 1)] = k;
  __syncthreads();
  // ascending ids inside every cell (insertion sort of a short list by the cell's owner thread)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int s0 = cs[4 * t + i], s1 = s0 + c4[i];
    for (int x = s0 + 1; x < s1; ++x) {
      const int v = ids[x];
      int y = x - 1;
      while (y >= s0 && ids[y] > v) {
        ids[y + 1] = ids[y];
        --y;
      }
      ids[y + 1] = v;
    }
    // the cell's centres as (x, y, z, id) records, contiguous: what the search streams through LDS
    float4 *rec = cell_rec + (size_t)b * m;
    for (int x = s0; x < s1; ++x) {
      const int k = ids[x];
      rec[x] = make_float4(ce[k], ce[k + m], ce[k + 2 * m], __int_as_float(k));
    }
  }
}

template <bool LDS_REC>  // false (m > NNC_MAX_M, PVDL's 12500-centre level): the records stay in global memory (L2-resident:
                         // 16 m bytes per cloud), only the cell table goes to LDS -- many workgroups per CU hide the L2 trips
__global__ __launch_bounds__(256) void three_nn_cells_kernel(int n, int m, const float *__restrict__ points,
                                                             const int *__restrict__ cell_start,
                                                             const float4 *__restrict__ cell_rec,
                                                             const float *__restrict__ box, float *__restrict__ weights,
                                                             int *__restrict__ indices) {
  // the cloud's cell table and sorted centre records, shared by the workgroup's 256 points (all of one cloud):
  // every candidate is then one 16-byte LDS read at an address known up front (no dependent global loads)
  extern __shared__ float4 nnc_lds[];
  const int b = blockIdx.y;
  const float4 *rec = LDS_REC ? (const float4 *)nnc_lds : cell_rec + (size_t)b * m;
  int *cs = (int *)(nnc_lds + (LDS_REC ? m : 0));
  if (LDS_REC)
    for (int i = threadIdx.x; i < m; i += 256) nnc_lds[i] = cell_rec[(size_t)b * m + i];
  for (int i = threadIdx.x; i <= NNC_CELLS; i += 256) cs[i] = cell_start[(size_t)b * (NNC_CELLS + 1) + i];
  __syncthreads();
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const float *p = points + (size_t)b * 3 * n;
  const float ux = p[j], uy = p[j + n], uz = p[j + 2 * n];
  const float h = box[(size_t)b * 4 + 3], inv = 1.0f / h;
  const int cx = min(max((int)floorf((ux - box[(size_t)b * 4]) * inv), 0), NNC_G - 1);
  const int cy = min(max((int)floorf((uy - box[(size_t)b * 4 + 1]) * inv), 0), NNC_G - 1);
  const int cz = min(max((int)floorf((uz - box[(size_t)b * 4 + 2]) * inv), 0), NNC_G - 1);
  float best0 = INFINITY, best1 = INFINITY, best2 = INFINITY;
  int i0 = 0, i1 = 0, i2 = 0;
  // (distance, index) lexicographic: what ascending-index brute force with strict '<' selects
  auto before = [](float d, int k, float bd, int bi) { return d < bd || (d == bd && k < bi); };
  // (always_inline: as an out-of-line call the by-reference captures -- the three bests -- would live in scratch)
  auto consider = [&](const float4 r) __attribute__((always_inline)) {
    const int k = __float_as_int(r.w);
    const float d = sqdist3(ux - r.x, uy - r.y, uz - r.z);
    if (d <= best2) {  // (one compare rejects almost every candidate)
      // sorted insertion as selects: written with nested ifs + shifts the compiler turned the three bests into a
      // dynamically indexed scratch array (8x slower)
      const bool c2 = before(d, k, best2, i2), c1 = before(d, k, best1, i1), c0 = before(d, k, best0, i0);
      const float n2 = c1 ? best1 : (c2 ? d : best2), n1 = c0 ? best0 : (c1 ? d : best1), n0 = c0 ? d : best0;
      const int m2 = c1 ? i1 : (c2 ? k : i2), m1 = c0 ? i0 : (c1 ? k : i1), m0 = c0 ? k : i0;
      best2 = n2;
      best1 = n1;
      best0 = n0;
      i2 = m2;
      i1 = m1;
      i0 = m0;
    }
  };
  auto visit_run = [&](int q0, int q1) __attribute__((always_inline)) {  // consecutive cells = consecutive records
    for (int q = q0; q < q1; q += 4) {  // four independent LDS reads in flight, candidates taken in order
      float4 r[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) r[u] = rec[min(q + u, q1 - 1)];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (q + u < q1) consider(r[u]);
    }
  };
  for (int rho = 1; rho < NNC_G; ++rho) {
    const int z0 = max(cz - rho, 0), z1 = min(cz + rho, NNC_G - 1);
    const int y0 = max(cy - rho, 0), y1 = min(cy + rho, NNC_G - 1);
    const int x0 = max(cx - rho, 0), x1 = min(cx + rho, NNC_G - 1);
    for (int z = z0; z <= z1; ++z)
      for (int y = y0; y <= y1; ++y) {
        const int row = (z * NNC_G + y) * NNC_G;  // the cells of one x-row are consecutive
        // rho = 1: the whole 3x3x3 block (ring 0 alone can never end the search); later: the shell of Chebyshev
        // radius rho -- full rows on its z / y faces, the two end cells on the interior rows
        const bool face = rho == 1 || z == cz - rho || z == cz + rho || y == cy - rho || y == cy + rho;
        if (face) {
          visit_run(cs[row + x0], cs[row + x1 + 1]);
        } else {
          if (cx - rho >= 0) visit_run(cs[row + cx - rho], cs[row + cx - rho + 1]);
          if (cx + rho <= NNC_G - 1) visit_run(cs[row + cx + rho], cs[row + cx + rho + 1]);
        }
      }
    // everything not visited yet is farther than rho * h (in at least one axis the cell index differs by > rho)
    const float bound = (float)rho * h;
    if (best2 <= bound * bound * 0.9999f && best2 < INFINITY) break;  // (margin: cell assignment rounds)
    if (x0 == 0 && y0 == 0 && z0 == 0 && x1 == NNC_G - 1 && y1 == NNC_G - 1 && z1 == NNC_G - 1) break;  // all cells seen
  }
  nn3_store_weights(best0, best1, best2, i0, i1, i2, weights + (size_t)b * 3 * n, indices + (size_t)b * 3 * n, j, n);
}

#define NNC_MAX_M 8192  // records + cell table in LDS: 16 m + 16.4 KB <= 148 KB

extern "C" size_t p2pb_three_nn_cells_ws_bytes(int b, int m) {
  return (size_t)b * m * 16 + ((size_t)b * (NNC_CELLS + 1) + (size_t)b * m) * sizeof(int) + (size_t)b * 4 * sizeof(float);
}

// p2pb_three_nn through a uniform grid over the centres: same idx / w. m >= 3 (records in LDS up to 8192 centres, in L2 above);
// ws: p2pb_three_nn_cells_ws_bytes(b, m) bytes, 16-byte aligned
extern "C" int p2pb_three_nn_cells(int b, int m, int n, const float *points, const float *centers, int *idx, float *w,
                                   void *ws, void *stream) {
  if (b <= 0 || n <= 0 || m < 3 || m > (1 << 24) || !ws || ((uintptr_t)ws & 15)) return P2PB_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  float4 *cell_rec = (float4 *)ws;
  int *cell_start = (int *)(cell_rec + (size_t)b * m);
  int *cell_ids = cell_start + (size_t)b * (NNC_CELLS + 1);
  float *box = (float *)(cell_ids + (size_t)b * m);
  const bool in_lds = m <= NNC_MAX_M;
  const size_t lds = (in_lds ? (size_t)m * 16 : 0) + (NNC_CELLS + 1) * sizeof(int) + 16;
  static bool once = false;
  if (!once) {
    (void)hipFuncSetAttribute((const void *)three_nn_cells_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    once = true;
  }
  hipLaunchKernelGGL(nn_cells_build_kernel, dim3(b), dim3(1024), 0, s, m, centers, cell_start, cell_ids, cell_rec, box);
  if (in_lds)
    hipLaunchKernelGGL(three_nn_cells_kernel<true>, dim3(cdiv(n, 256), b), dim3(256), lds, s, n, m, points, cell_start, cell_rec,
                       box, w, idx);
  else
    hipLaunchKernelGGL(three_nn_cells_kernel<false>, dim3(cdiv(n, 256), b), dim3(256), lds, s, n, m, points, cell_start, cell_rec,
                       box, w, idx);
  return p2pb_launch_status();
}

// ------------------------------------------------------------------------------------------------
// three-interpolate: out[b,l,j] = sum_k weight_k[b,j] * features[b,l,idx_k[b,j]], k = 0, 1, 2 left to right as one
// multiply and two fused multiply-adds. Lanes along n; a thread reads its three (idx, weight) pairs once -- [b,3,n]
// (ChannelMajor) or [b,n,3] (PointMajor) -- and walks TI_CC channels, so the writes go out lane-consecutive.
// GRAD (PN2 only) ADDS grad_out * weight_k into grad_features[b,l,idx_k] (global_atomic_add_f32): the caller's buffer is
// accumulated into, not zeroed (PN2/interpolate_gpu.cu:146-148; the layer passes zeros).
// ------------------------------------------------------------------------------------------------
#define TI_CC 16
template <template <class> class Layout, bool GRAD>
__global__ __launch_bounds__(256) void three_interp_kernel(int c, int m, int n, const float *__restrict__ src,
                                                           const int *__restrict__ indices,
                                                           const float *__restrict__ weights, float *dst) {
  const int b = blockIdx.z;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  int a0, a1, a2;
  float w0, w1, w2;
  Layout<int>{indices + (size_t)b * 3 * n, n}.load(j, a0, a1, a2);
  Layout<float>{weights + (size_t)b * 3 * n, n}.load(j, w0, w1, w2);
  const int c0 = blockIdx.y * TI_CC, c1 = min(c0 + TI_CC, c);
  for (int l = c0; l < c1; ++l) {
    if (GRAD) {  // src = grad_out f32[b,c,n], dst = grad_features f32[b,c,m]
      const float g = src[((size_t)b * c + l) * n + j];
      float *o = dst + ((size_t)b * c + l) * m;
      atomicAdd(o + a0, g * w0);
      atomicAdd(o + a1, g * w1);
      atomicAdd(o + a2, g * w2);
    } else {  // src = features f32[b,c,m], dst = out f32[b,c,n]
      const float *f = src + ((size_t)b * c + l) * m;
      dst[((size_t)b * c + l) * n + j] = __fmaf_rn(f[a2], w2, __fmaf_rn(f[a1], w1, f[a0] * w0));
    }
  }
}

template <template <class> class Layout, bool GRAD>
static int three_interp_launch(int b, int c, int m, int n, const float *src, const int *idx, const float *w, float *dst,
                               hipStream_t s) {
  hipLaunchKernelGGL((three_interp_kernel<Layout, GRAD>), dim3(cdiv(n, 256), cdiv(c, TI_CC), b), dim3(256), 0, s, c, m, n,
                     src, idx, w, dst);
  return p2pb_launch_status();
}

extern "C" int p2pb_three_interpolate(int b, int c, int m, int n, const float *cfeat, const int *idx, const float *w,
                                      float *out, void *stream) {
  if (b <= 0 || c <= 0 || n <= 0 || m <= 0) return P2PB_EINVAL;
  return three_interp_launch<ChannelMajor, false>(b, c, m, n, cfeat, idx, w, out, (hipStream_t)stream);
}

// search + interpolation in one call
extern "C" int p2pb_three_nn_interpolate_forward(int b, int c, int m, int n, const float *points,
                                                 const float *centers, const float *cfeat, int *idx, float *w,
                                                 float *out, void *stream) {
  if (b <= 0 || c <= 0 || n <= 0 || m <= 0) return P2PB_EINVAL;
  const int rc = p2pb_three_nn(b, m, n, points, centers, idx, w, stream);
  if (rc) return rc;
  return three_interp_launch<ChannelMajor, false>(b, c, m, n, cfeat, idx, w, out, (hipStream_t)stream);
}

extern "C" int p2pb_pn2_three_interpolate(int b, int c, int m, int n, const float *features, const int *idx,
                                          const float *weight, float *out, void *stream) {
  if (b <= 0 || b > 65535 || c <= 0 || m <= 0 || n <= 0 || !features || !idx || !weight || !out) return P2PB_EINVAL;
  return three_interp_launch<PointMajor, false>(b, c, m, n, features, idx, weight, out, (hipStream_t)stream);
}

// Global atomics in an order that is not fixed: refused in deterministic mode, as the library refuses every scatter it
// cannot run in a fixed order (scatter_grad.hip). The [b,n,3] index layout does not fit that file's LDS-row family.
extern "C" int p2pb_pn2_three_interpolate_grad(int b, int c, int n, int m, const float *grad_out, const int *idx,
                                               const float *weight, float *grad_features, void *stream) {
  if (b <= 0 || b > 65535 || c <= 0 || m <= 0 || n <= 0 || !grad_out || !idx || !weight || !grad_features) return P2PB_EINVAL;
  if (p2pb_deterministic()) return P2PB_EINVAL;
  return three_interp_launch<PointMajor, true>(b, c, m, n, grad_out, idx, weight, grad_features, (hipStream_t)stream);
}
