// pointnet2_legacy.hip -- the classic PointNet++ operators of the reference's extension, on its POINT-MAJOR clouds
// (xyz f32[B,N,3]; PN2 = third_party/openpoints/cpp/pointnet2_batch/src):
//   p2pb_pn2_ball_query              (PN2/ball_query_gpu.cu:15)
//   p2pb_pn2_three_nn                (PN2/interpolate_gpu.cu:16)
//   p2pb_pn2_three_interpolate       (PN2/interpolate_gpu.cu:84)
//   p2pb_pn2_three_interpolate_grad  (PN2/interpolate_gpu.cu:127)
// The caller owns every output; the gradient ADDS into its target. p2pb_pn2_fps of the same extension is in fps_ref.hip,
// with the pointops sampler it shares its kernels with; group_points* / gather_points* have the layout and arithmetic of
// p2pb_grouping_* / p2pb_gather_features_* (neighbors.hip, scatter_grad.hip) and are routed there by the Python module.
// Squared distances are sqdist3 (common.h), as everywhere in the library.
#include "common.h"

// ------------------------------------------------------------------------------------------------
// ball query: one wave per centre, ballot + mbcnt ordered slots as ball_query_lds_kernel (neighbors.hip), the cloud
// staged in LDS as three planes when it fits and there are enough centres to share it. What differs from the
// channel-major operator is the contract: a centre without a neighbour leaves its row as the caller filled it
// (PN2/ball_query_gpu.cu:40-49 writes on a hit only).
// ------------------------------------------------------------------------------------------------
#define PN2_BQ_UNROLL 4
template <bool LDS>
__global__ __launch_bounds__(1024) void pn2_ball_query_kernel(int n, int m, float r2, int u, int cpw,
                                                              const float *__restrict__ new_xyz,
                                                              const float *__restrict__ xyz, int *__restrict__ idx) {
  extern __shared__ float pn2_bq_pts[];  // [3][n] when LDS
  const int b = blockIdx.y;
  const int lane = lane_id(), wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const float *p = xyz + (size_t)b * 3 * n;
  const float *ce = new_xyz + (size_t)b * 3 * m;
  if (LDS) {
    for (int k = threadIdx.x; k < 3 * n; k += blockDim.x) pn2_bq_pts[(k % 3) * n + k / 3] = p[k];
    __syncthreads();
  }
  const int j0 = (blockIdx.x * nwaves + wave) * cpw;
  for (int j = j0; j < min(j0 + cpw, m); ++j) {
    int *o = idx + ((size_t)b * m + j) * u;
    const float cx = ce[3 * j], cy = ce[3 * j + 1], cz = ce[3 * j + 2];
    int cnt = 0, first = 0;
    for (int base = 0; base < n && cnt < u; base += 64 * PN2_BQ_UNROLL) {
      float px[PN2_BQ_UNROLL], py[PN2_BQ_UNROLL], pz[PN2_BQ_UNROLL];
#pragma unroll
      for (int q = 0; q < PN2_BQ_UNROLL; ++q) {
        const int k = min(base + q * 64 + lane, n - 1);
        if (LDS) {
          px[q] = pn2_bq_pts[k];
          py[q] = pn2_bq_pts[n + k];
          pz[q] = pn2_bq_pts[2 * n + k];
        } else {
          px[q] = p[(size_t)3 * k];
          py[q] = p[(size_t)3 * k + 1];
          pz[q] = p[(size_t)3 * k + 2];
        }
      }
#pragma unroll
      for (int q = 0; q < PN2_BQ_UNROLL; ++q) {
        const int k = base + q * 64 + lane;
        const float d2 = sqdist3(cx - px[q], cy - py[q], cz - pz[q]);
        const bool in = (k < n) && (d2 < r2);
        const unsigned long long mask = __ballot(in);
        if (mask) {
          const int slot = cnt + mbcnt(mask);
          if (in && slot < u) o[slot] = k;
          if (cnt == 0) first = base + q * 64 + (int)__builtin_ctzll(mask);
          cnt += (int)__builtin_popcountll(mask);
        }
      }
    }
    // the first hit fills every slot, later hits overwrite slots 1, 2, ...: slots >= cnt keep the first hit
    if (cnt > 0)
      for (int v = cnt + lane; v < u; v += 64) o[v] = first;
  }
}

#define PN2_BQ_LDS_MAX (144 * 1024)
extern "C" int p2pb_pn2_ball_query(int b, int n, int m, float radius, int nsample, const float *new_xyz, const float *xyz,
                                   int *idx, void *stream) {
  if (b <= 0 || b > 65535 || n <= 0 || m <= 0 || nsample <= 0 || !new_xyz || !xyz || !idx) return P2PB_EINVAL;
  const float r2 = radius * radius;  // the float product of PN2/ball_query_gpu.cu:29
  const size_t lds = (size_t)3 * n * sizeof(float);
  if (lds <= PN2_BQ_LDS_MAX && (long)m * b >= 2048) {  // enough centres to share the staged cloud (the bound of p2pb_ball_query)
    static bool once = false;
    if (!once) {
      (void)hipFuncSetAttribute((const void *)pn2_ball_query_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                160 * 1024);
      once = true;
    }
    // centres per wave: about two workgroups per CU over the whole launch, at least 1 (as p2pb_ball_query)
    int cpw = (int)(((long)m * b + 16L * 512 - 1) / (16L * 512));
    if (cpw < 1) cpw = 1;
    hipLaunchKernelGGL(pn2_ball_query_kernel<true>, dim3(cdiv(m, 16 * cpw), b), dim3(1024), lds, (hipStream_t)stream, n, m,
                       r2, nsample, cpw, new_xyz, xyz, idx);
    return p2pb_launch_status();
  }
  hipLaunchKernelGGL(pn2_ball_query_kernel<false>, dim3(cdiv(m, 4), b), dim3(256), 0, (hipStream_t)stream, n, m, r2,
                     nsample, 1, new_xyz, xyz, idx);
  return p2pb_launch_status();
}

// ------------------------------------------------------------------------------------------------
// three nearest known points of every unknown point: one lane per query, `known` tiled through LDS as planes and read
// back as wave-wide broadcasts (three_nn_kernel of neighbors.hip without the weights). Strict '<' in ascending k: among
// equal distances the lower index ranks first. The reference's bests start at 1e40 in double, which no fp32 distance
// reaches and which its float store turns into +inf: +inf in fp32 takes the same branches, so for m < 3 the unfilled
// slots are idx 0, dist2 +inf.
// ------------------------------------------------------------------------------------------------
#define PN2_NN_TILE 2048
__global__ __launch_bounds__(256) void pn2_three_nn_kernel(int n, int m, const float *__restrict__ unknown,
                                                           const float *__restrict__ known, float *__restrict__ dist2,
                                                           int *__restrict__ idx) {
  __shared__ float sc[3][PN2_NN_TILE];
  const int b = blockIdx.y;
  const int j = blockIdx.x * 256 + threadIdx.x;
  const float *un = unknown + (size_t)b * 3 * n;
  const float *kn = known + (size_t)b * 3 * m;
  const bool ok = j < n;
  const float ux = ok ? un[(size_t)3 * j] : 0.0f, uy = ok ? un[(size_t)3 * j + 1] : 0.0f, uz = ok ? un[(size_t)3 * j + 2] : 0.0f;
  float best0 = INFINITY, best1 = INFINITY, best2 = INFINITY;
  int i0 = 0, i1 = 0, i2 = 0;
  for (int k0 = 0; k0 < m; k0 += PN2_NN_TILE) {
    const int kn_ = min(PN2_NN_TILE, m - k0);
    __syncthreads();
    for (int k = threadIdx.x; k < 3 * kn_; k += 256) sc[k % 3][k / 3] = kn[(size_t)3 * k0 + k];
    __syncthreads();
    for (int k = 0; k < kn_; ++k) {
      const float d = sqdist3(ux - sc[0][k], uy - sc[1][k], uz - sc[2][k]);
      if (d < best2) {
        best2 = d;
        i2 = k0 + k;
        if (d < best1) {
          best2 = best1;
          i2 = i1;
          best1 = d;
          i1 = k0 + k;
          if (d < best0) {
            best1 = best0;
            i1 = i0;
            best0 = d;
            i0 = k0 + k;
          }
        }
      }
    }
  }
  if (!ok) return;
  float *d = dist2 + ((size_t)b * n + j) * 3;
  int *id = idx + ((size_t)b * n + j) * 3;
  d[0] = best0;
  d[1] = best1;
  d[2] = best2;
  id[0] = i0;
  id[1] = i1;
  id[2] = i2;
}

extern "C" int p2pb_pn2_three_nn(int b, int n, int m, const float *unknown, const float *known, float *dist2, int *idx,
                                 void *stream) {
  if (b <= 0 || b > 65535 || n <= 0 || m <= 0 || !unknown || !known || !dist2 || !idx) return P2PB_EINVAL;
  hipLaunchKernelGGL(pn2_three_nn_kernel, dim3(cdiv(n, 256), b), dim3(256), 0, (hipStream_t)stream, n, m, unknown, known,
                     dist2, idx);
  return p2pb_launch_status();
}

// ------------------------------------------------------------------------------------------------
// three-interpolate: out[b,l,j] = sum_k weight[b,j,k] * features[b,l,idx[b,j,k]], k = 0, 1, 2 left to right in the
// library's fused form (three_interp_kernel, neighbors.hip). Lanes along n; a thread reads its three (idx, weight)
// pairs once and walks CC channels, so the writes go out lane-consecutive.
// The gradient ADDS grad_out * weight_k into grad_features[b,l,idx_k] (global_atomic_add_f32): the caller's buffer is
// accumulated into, not zeroed (PN2/interpolate_gpu.cu:146-148; the layer passes zeros).
// ------------------------------------------------------------------------------------------------
#define PN2_TI_CC 16
template <bool GRAD>
__global__ __launch_bounds__(256) void pn2_three_interp_kernel(int c, int m, int n, const float *__restrict__ src,
                                                               const int *__restrict__ idx,
                                                               const float *__restrict__ weight, float *dst) {
  const int b = blockIdx.z;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int *id = idx + ((size_t)b * n + j) * 3;
  const float *w = weight + ((size_t)b * n + j) * 3;
  const int a0 = id[0], a1 = id[1], a2 = id[2];
  const float w0 = w[0], w1 = w[1], w2 = w[2];
  const int c0 = blockIdx.y * PN2_TI_CC, c1 = min(c0 + PN2_TI_CC, c);
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

extern "C" int p2pb_pn2_three_interpolate(int b, int c, int m, int n, const float *features, const int *idx,
                                          const float *weight, float *out, void *stream) {
  if (b <= 0 || b > 65535 || c <= 0 || m <= 0 || n <= 0 || !features || !idx || !weight || !out) return P2PB_EINVAL;
  hipLaunchKernelGGL(pn2_three_interp_kernel<false>, dim3(cdiv(n, 256), cdiv(c, PN2_TI_CC), b), dim3(256), 0,
                     (hipStream_t)stream, c, m, n, features, idx, weight, out);
  return p2pb_launch_status();
}

// Global atomics in an order that is not fixed: refused in deterministic mode, as the library refuses every scatter it
// cannot run in a fixed order (scatter_grad.hip). The [b,n,3] index layout does not fit that file's LDS-row family.
extern "C" int p2pb_pn2_three_interpolate_grad(int b, int c, int n, int m, const float *grad_out, const int *idx,
                                               const float *weight, float *grad_features, void *stream) {
  if (b <= 0 || b > 65535 || c <= 0 || m <= 0 || n <= 0 || !grad_out || !idx || !weight || !grad_features) return P2PB_EINVAL;
  if (p2pb_deterministic()) return P2PB_EINVAL;
  hipLaunchKernelGGL(pn2_three_interp_kernel<true>, dim3(cdiv(n, 256), cdiv(c, PN2_TI_CC), b), dim3(256), 0,
                     (hipStream_t)stream, c, m, n, grad_out, idx, weight, grad_features);
  return p2pb_launch_status();
}
