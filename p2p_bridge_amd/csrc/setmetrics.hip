// setmetrics.hip -- set-against-set generative metrics (metrics/evaluation_metrics_fast.py): the S x R matrices of Chamfer and
// approximate-EMD distances between every cloud of one set and every cloud of another, and the occupancy-grid counters behind
// the JSD. The reference fills a matrix row by row: it expands ONE cloud R times (expand().contiguous(), :215-216) and calls the
// batched extension on the copy (:219-231); here the pair (i, j) is an index inside the kernels and no copy exists.
//
// Chamfer (pw_nn_sum_kernel): one direction per launch, D[i, j] = sum_p min_q |A_ip - B_jq|^2. A workgroup stages ONE target
// cloud B_j in LDS as 16-byte records and walks a tile of `tq` query clouds over it, so a cloud comes from HBM once per tile of
// pairs. A thread holds 8 query points as 4 packed pairs: per LDS record (one broadcast ds_read_b128) it issues 4 x (3 v_pk_add
// + v_pk_mul + 2 v_pk_fma) + 8 v_min = 32 VALU instructions for 8 point pairs -- nm_distance_kernel's arithmetic (chamfer.hip:
// fma(dz, dz, fma(dy, dy, dx * dx)) on t - q) without the index bookkeeping. The minima are summed in fp64 in a fixed order
// (thread-sequential, then an LDS tree): no floating-point atomics, same bits every run.
//
// EMD: approxmatch only ever adds into match[l, k] and never reads it, and matchcost is linear in it, so
// cost = sum_levels sum_kl w_kl d_kl is accumulated level by level per point k and the n x m match matrix is never stored:
// the single-pass kernels of emd_sweep.h, which emd.hip runs too, with the pair (i, j) as their addressing. Pairs are
// processed in chunks bounded by the caller's workspace.
#include "emd_sweep.h"

typedef float smf2 __attribute__((ext_vector_type(2)));

#define SM_TILE 2048  // target points per LDS tile (32 KB: five workgroups per CU inside the 160 KB LDS)
#define SM_QP 4       // packed query pairs per thread: 8 points, 2048 per pass of a 256-thread workgroup

__global__ __launch_bounds__(256) void pw_nn_sum_kernel(int s, int r, int n, int m, int tq, const float *__restrict__ A,
                                                        const float *__restrict__ B, double *__restrict__ D) {
  __shared__ float4 buf[SM_TILE];
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const int j = blockIdx.x;
  const int i0 = blockIdx.y * tq, i1 = min(s, i0 + tq);
  const float *tg = B + (size_t)j * m * 3;
  const bool resident = m <= SM_TILE;  // the whole target cloud stays in LDS for every query cloud of the tile
  if (resident) {
    for (int e = tid; e < m; e += 256) buf[e] = make_float4(tg[e * 3], tg[e * 3 + 1], tg[e * 3 + 2], 0.0f);
    __syncthreads();
  }
  for (int i = i0; i < i1; ++i) {
    const float *qc = A + (size_t)i * n * 3;
    double acc = 0.0;
    for (int p0 = 0; p0 < n; p0 += 256 * 2 * SM_QP) {
      smf2 x[SM_QP], y[SM_QP], z[SM_QP];
      float best[2 * SM_QP];
#pragma unroll
      for (int u = 0; u < SM_QP; ++u) {
        const int pa = p0 + (2 * u) * 256 + tid, pb = pa + 256;
        const float *qa = qc + (size_t)(pa < n ? pa : 0) * 3, *qb = qc + (size_t)(pb < n ? pb : 0) * 3;
        x[u] = smf2{qa[0], qb[0]}, y[u] = smf2{qa[1], qb[1]}, z[u] = smf2{qa[2], qb[2]};
        best[2 * u] = INFINITY, best[2 * u + 1] = INFINITY;
      }
      for (int k0 = 0; k0 < m; k0 += SM_TILE) {
        const int kn = min(SM_TILE, m - k0);
        if (!resident) {
          __syncthreads();
          for (int e = tid; e < kn; e += 256) {
            const float *t = tg + (size_t)(k0 + e) * 3;
            buf[e] = make_float4(t[0], t[1], t[2], 0.0f);
          }
          __syncthreads();
        }
#pragma unroll 2
        for (int k = 0; k < kn; ++k) {
          const float4 t = buf[k];
#pragma unroll
          for (int u = 0; u < SM_QP; ++u) {
            const smf2 dx = smf2{t.x, t.x} - x[u], dy = smf2{t.y, t.y} - y[u], dz = smf2{t.z, t.z} - z[u];
            const smf2 d = __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, dx * dx));
            best[2 * u] = fminf(best[2 * u], d[0]);  // the VALUE of the strict-'<' minimum (a NaN distance never wins either way)
            best[2 * u + 1] = fminf(best[2 * u + 1], d[1]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 2 * SM_QP; ++u)
        if (p0 + u * 256 + tid < n) acc += (double)best[u];
    }
    red[tid] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (tid < w) red[tid] += red[tid + w];
      __syncthreads();
    }
    if (tid == 0) D[(size_t)i * r + j] = red[0];
    __syncthreads();
  }
}

// out[i, j] = fp32(D1[i, j] / n + D2[j, i] / m): the one rounding to fp32. (Symmetric case: D1 == D2, n == m, and the double
// addition commutes, so out equals its transpose bitwise.)
__global__ __launch_bounds__(256) void pw_chamfer_finish_kernel(int s, int r, int n, int m, const double *__restrict__ D1,
                                                                const double *__restrict__ D2, float *__restrict__ out) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)s * r) return;
  const int i = (int)(e / r), j = (int)(e % r);
  out[e] = (float)(D1[e] / (double)n + D2[(size_t)j * s + i] / (double)m);
}

static void pw_nn_sum(int s, int r, int n, int m, const float *A, const float *B, double *D, hipStream_t st) {
  int tq = 8;  // query clouds per workgroup: fewer when the tile grid alone cannot fill the chip
  while (tq > 1 && (long)r * cdiv(s, tq) < 2048) tq /= 2;
  // (blockIdx.y <= 65535: s / tq stays far below for any set that fits in memory; the entry point checks)
  hipLaunchKernelGGL(pw_nn_sum_kernel, dim3(r, cdiv(s, tq)), dim3(256), 0, st, s, r, n, m, tq, A, B, D);
}

extern "C" size_t p2pb_pairwise_chamfer_ws_bytes(int s, int r) {
  if (s <= 0 || r <= 0) return 0;
  return (size_t)s * r * 2 * sizeof(double);
}

extern "C" int p2pb_pairwise_chamfer(int s, int r, int n, int m, const float *A, const float *B, float *out, void *ws,
                                     void *stream) {
  if (s <= 0 || r <= 0 || n <= 0 || m <= 0 || !A || !B || !out || !ws || s > 65535 || r > 65535) return P2PB_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  double *D1 = (double *)ws, *D2 = D1 + (size_t)s * r;
  if (A == B && s == r && n == m) {
    pw_nn_sum(s, s, n, n, A, A, D1, st);
    D2 = D1;
  } else {
    pw_nn_sum(s, r, n, m, A, B, D1, st);
    pw_nn_sum(r, s, m, n, B, A, D2, st);
  }
  hipLaunchKernelGGL(pw_chamfer_finish_kernel, dim3(cdiv((long)s * r, 256)), dim3(256), 0, st, s, r, n, m, D1, D2, out);
  return p2pb_launch_status();
}

// ------------------------------------------------------------------------------------------------------------------
// approximate EMD for a chunk of pairs: emd_sweep.h on EmdPairwise's work arrays, then the mean of costk
// ------------------------------------------------------------------------------------------------------------------
#define EM_PAIRS_MAX 32768

// out[p] = fp32(sum_k costk_k / n): fp64, thread-sequential then an LDS tree (fixed order)
__global__ __launch_bounds__(256) void em_finish_kernel(EmdPairwise addr, int n, int m, float *__restrict__ out) {
  __shared__ double red[256];
  const EmdProblem e = addr(blockIdx.y, n, m);
  double acc = 0.0;
  for (int k = threadIdx.x; k < n; k += 256) acc += (double)e.costk[k];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[addr.p0 + blockIdx.y] = (float)(red[0] / (double)n);
}

static size_t em_pair_bytes(int n, int m) { return (3 * (size_t)n + 2 * (size_t)m) * sizeof(float); }

extern "C" size_t p2pb_pairwise_emd_ws_bytes(int s, int r, int n, int m) {
  if (s <= 0 || r <= 0 || n <= 0 || m <= 0) return 0;
  const size_t pairs = (size_t)s * r;
  return em_pair_bytes(n, m) * (pairs < 4096 ? pairs : 4096);  // 4096 pairs in flight fill the chip at any cloud size
}

extern "C" int p2pb_pairwise_emd(int s, int r, int n, int m, const float *A, const float *B, float *out, void *ws,
                                 size_t ws_bytes, void *stream) {
  if (s <= 0 || r <= 0 || n <= 0 || m <= 0 || !A || !B || !out || !ws) return P2PB_EINVAL;
  const size_t fit = ws_bytes / em_pair_bytes(n, m);
  if (fit == 0) return P2PB_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const long pairs = (long)s * r;
  const long chunk = (long)(fit < EM_PAIRS_MAX ? fit : EM_PAIRS_MAX);
  for (long p0 = 0; p0 < pairs; p0 += chunk) {
    const unsigned np = (unsigned)(pairs - p0 < chunk ? pairs - p0 : chunk);
    const EmdPairwise addr = {A, B, (float *)ws, (int)p0, r};
    emd_anneal(addr, (int)np, n, m, 1, st);
    hipLaunchKernelGGL(em_finish_kernel, dim3(1, np), dim3(256), 0, st, addr, n, m, out);
  }
  return p2pb_launch_status();
}

// ------------------------------------------------------------------------------------------------------------------
// Occupancy grid (entropy_of_occupancy_grid :587-600 on unit_cube_grid_point_cloud :534-552). Centres are
// fp32(i * spacing - 0.5) with spacing = 1 / (resolution - 1) in double, as numpy fills its float32 array; with clip_sphere a
// cell is kept when sqrt((x*x + y*y) + z*z) <= 0.5 in fp32 (numpy.linalg.norm on the float32 rows), indexed in row-major order.
// ------------------------------------------------------------------------------------------------------------------
#define OCC_RES_MAX 80  // the per-cloud "touched" bitmap (resolution^3 bits) lives in LDS: 64 KB

__host__ __device__ static inline float occ_centre(int i, double spacing) { return (float)((double)i * spacing - 0.5); }
__host__ __device__ static inline bool occ_kept(float x, float y, float z, int clip) {
  if (!clip) return true;
  const float s2 = (x * x + y * y) + z * z;
#ifdef __HIP_DEVICE_COMPILE__
  return __fsqrt_rn(s2) <= 0.5f;
#else
  return sqrtf(s2) <= 0.5f;
#endif
}

extern "C" int p2pb_occupancy_grid_cells(int resolution, int clip_sphere) {
  if (resolution < 2 || resolution > OCC_RES_MAX) return P2PB_EINVAL;
  const double spacing = 1.0 / (double)(resolution - 1);
  int g = 0;
  for (int i = 0; i < resolution; ++i)
    for (int j = 0; j < resolution; ++j)
      for (int k = 0; k < resolution; ++k)
        g += occ_kept(occ_centre(i, spacing), occ_centre(j, spacing), occ_centre(k, spacing), clip_sphere) ? 1 : 0;
  return g;
}

extern "C" size_t p2pb_occupancy_ws_bytes(int resolution) {
  if (resolution < 2 || resolution > OCC_RES_MAX) return 0;
  const size_t cells = (size_t)resolution * resolution * resolution;
  return cells * (sizeof(int) + sizeof(float4));  // kept centres float4[<= cells] | cell -> kept index int[cells]
}

// one workgroup: cellidx[cell] = index among the kept cells (row-major) or -1, centres[index] = (x, y, z, 0)
__global__ __launch_bounds__(1024) void occ_table_kernel(int res, int clip, float4 *__restrict__ centres,
                                                         int *__restrict__ cellidx) {
  __shared__ int cnt[1024];
  const int cells = res * res * res, per = (cells + 1023) / 1024;
  const double spacing = 1.0 / (double)(res - 1);
  const int c0 = min(cells, (int)threadIdx.x * per), c1 = min(cells, c0 + per);
  int mine = 0;
  for (int c = c0; c < c1; ++c)
    mine += occ_kept(occ_centre(c / (res * res), spacing), occ_centre(c / res % res, spacing), occ_centre(c % res, spacing), clip) ? 1 : 0;
  cnt[threadIdx.x] = mine;
  __syncthreads();
  int at = 0;
  for (int t = 0; t < (int)threadIdx.x; ++t) at += cnt[t];
  for (int c = c0; c < c1; ++c) {
    const float x = occ_centre(c / (res * res), spacing), y = occ_centre(c / res % res, spacing), z = occ_centre(c % res, spacing);
    if (occ_kept(x, y, z, clip)) {
      centres[at] = make_float4(x, y, z, 0.0f);
      cellidx[c] = at++;
    } else {
      cellidx[c] = -1;
    }
  }
}

// index of the centre nearest to v along one axis: the rounded one, corrected against its neighbours with the fp32 centres
// themselves (lowest index on a tie)
__device__ __forceinline__ int occ_axis(float v, int res, double spacing) {
  const float f = (v + 0.5f) * (float)(res - 1);
  int i = f >= 0.0f ? (f <= (float)(res - 1) ? (int)(f + 0.5f) : res - 1) : 0;  // (a NaN takes cell 0)
  i = min(max(i, 0), res - 1);
  int best = max(i - 1, 0);
  float bd = fabsf(v - occ_centre(best, spacing));
  for (int c = best + 1; c <= min(i + 1, res - 1); ++c) {
    const float d = fabsf(v - occ_centre(c, spacing));
    if (d < bd) bd = d, best = c;
  }
  return best;
}

// one workgroup per cloud; counters / bernoulli zeroed by the launcher
__global__ __launch_bounds__(256) void occ_count_kernel(int npts, int res, int G, const float *__restrict__ pts,
                                                        const float4 *__restrict__ centres, const int *__restrict__ cellidx,
                                                        int *__restrict__ counters, int *__restrict__ bernoulli) {
  extern __shared__ unsigned occ_touched[];  // G bits
  const int words = (G + 31) / 32;
  for (int w = threadIdx.x; w < words; w += 256) occ_touched[w] = 0u;
  __syncthreads();
  const double spacing = 1.0 / (double)(res - 1);
  const float *pc = pts + (size_t)blockIdx.x * npts * 3;
  const int lane = lane_id();
  for (int base = 0; base < npts; base += 256) {
    const int p = base + threadIdx.x;
    const bool ok = p < npts;
    const float *q = pc + (size_t)(ok ? p : 0) * 3;
    const float x = q[0], y = q[1], z = q[2];
    int cell = -1;
    if (ok) cell = cellidx[(occ_axis(x, res, spacing) * res + occ_axis(y, res, spacing)) * res + occ_axis(z, res, spacing)];
    // points whose rounded cell was clipped away: the whole wave searches the kept cells for one point at a time
    unsigned long long todo = __ballot(ok && cell < 0);
    while (todo) {
      const int src = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const float sx = __shfl(x, src), sy = __shfl(y, src), sz = __shfl(z, src);
      float bd = INFINITY;
      int bi = 0x7fffffff;
      for (int c = lane; c < G; c += 64) {  // ascending per lane with strict '<': the lane's lowest index wins its ties
        const float4 t = centres[c];
        const float d = sqdist3(t.x - sx, t.y - sy, t.z - sz);
        if (d < bd) bd = d, bi = c;
      }
      for (int off = 32; off > 0; off >>= 1) {
        const float od = __shfl_xor(bd, off);
        const int oi = __shfl_xor(bi, off);
        if (od < bd || (od == bd && oi < bi)) bd = od, bi = oi;
      }
      if (lane == src) cell = bi < G ? bi : 0;  // (all-NaN distances: cell 0, like the rounding path)
    }
    if (ok) {
      atomicAdd(counters + cell, 1);
      const unsigned bit = 1u << (cell & 31);
      if (!(atomicOr(occ_touched + (cell >> 5), bit) & bit)) atomicAdd(bernoulli + cell, 1);
    }
  }
}

extern "C" int p2pb_occupancy_counts(int clouds, int npts, int resolution, int clip_sphere, const float *pts, int *counters,
                                     int *bernoulli, void *ws, void *stream) {
  if (clouds <= 0 || npts <= 0 || resolution < 2 || resolution > OCC_RES_MAX || !pts || !counters || !bernoulli || !ws)
    return P2PB_EINVAL;
  const int G = p2pb_occupancy_grid_cells(resolution, clip_sphere);
  if (G <= 0) return P2PB_EINVAL;  // (resolution 2 with clip_sphere keeps no cell)
  hipStream_t st = (hipStream_t)stream;
  const size_t cells = (size_t)resolution * resolution * resolution;
  float4 *centres = (float4 *)ws;
  int *cellidx = (int *)(centres + cells);
  int e = p2pb_zero_async(counters, sizeof(int) * (size_t)G, st);
  if (e == 0) e = p2pb_zero_async(bernoulli, sizeof(int) * (size_t)G, st);
  if (e != 0) return e;
  hipLaunchKernelGGL(occ_table_kernel, dim3(1), dim3(1024), 0, st, resolution, clip_sphere ? 1 : 0, centres, cellidx);
  hipLaunchKernelGGL(occ_count_kernel, dim3(clouds), dim3(256), (size_t)((G + 31) / 32) * 4, st, npts, resolution, G, pts,
                     centres, cellidx, counters, bernoulli);
  return p2pb_launch_status();
}
