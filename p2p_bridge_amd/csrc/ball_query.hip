// ball_query.hip -- the ball query of both operator families, one scan and one launcher:
//   p2pb_ball_query      (PN2/pvcnn_ball_query_gpu.cu:19)  clouds f32[B,3,N] (ChannelMajor), a centre without a neighbour
//                                                          gets a row of zeros (pvcnn_ball_query.cpp:21)
//   p2pb_pn2_ball_query  (PN2/ball_query_gpu.cu:15)        clouds f32[B,N,3] (PointMajor), a centre without a neighbour
//                                                          leaves its row as the caller filled it (:40-49 writes on a hit only)
// (PN2 = third_party/openpoints/cpp/pointnet2_batch/src; the other classic operators: three_nn.hip, fps_ref.hip, and
// group_points* / gather_points*, which the Python module routes to p2pb_grouping_* / p2pb_gather_features_*.)
// The reference runs one thread block per cloud; here the centres are spread over waves x workgroups x batch.
// Squared distances are sqdist3 (common.h), as everywhere in the library.
#include "cloud_layout.h"

// ------------------------------------------------------------------------------------------------
// One 64-lane wave scans the cloud for one centre, 64 x 4 points at a time (lane-consecutive = coalesced reads), a wave
// ballot marks the in-radius lanes and the popcount of the lower lanes is the output slot, which reproduces the
// reference's "first u hits in ascending point index" order exactly; the scan stops as soon as u hits are found.
// On the first hit the reference sets every slot to it and later hits overwrite slots 0 .. cnt-1: slots >= cnt hold the
// first hit. Without a hit ZERO_FILL writes a row of zeros, the other contract nothing.
//
// Every wave walks `cpw` centres. LDS: the workgroup (16 waves) first copies the cloud into LDS as three planes. One wave
// per centre straight from global memory makes every wave re-read the cloud through L1/L2: 2048 centres x ~48 % of 8192
// points x 12 B x 32 samples = 3 GB of cache traffic per call at the sampler's first level. Alone the kernel is bound by
// instruction issue either way (190 us: ~25 instructions per 64-point step, mostly the ballot / slot bookkeeping -- packed
// fp32 for the distances changes nothing), but it runs on the geometry stream BESIDE the GEMMs and convolutions of the
// main stream, which need that cache bandwidth: with the cloud in LDS (3 x n floats, 96 KB at n = 8192) the sampler gains
// 0.9 % end to end. Same hit order, same outputs.
// (The scan is written out in the kernel, its point source chosen by type: as a function of its own it compiled to a
// rotated loop counter, two more instructions per 256 points, and the LDS arm measured 1 % slower. The two fills are
// worded apart for the same reason: with them the channel-major LDS kernel is the previous one but for the order of
// thirteen instructions before the loop.)
// ------------------------------------------------------------------------------------------------
#define BQ_UNROLL 4
template <class Cloud, bool LDS, bool ZERO_FILL>
__global__ __launch_bounds__(1024) void ball_query_kernel(int n, int m, float r2, int u, int cpw,
                                                          const float *__restrict__ centers,
                                                          const float *__restrict__ points, int *__restrict__ idx) {
  extern __shared__ float bq_planes[];  // [3][n] when LDS
  constexpr int NT = LDS ? 1024 : 256;  // the workgroup sizes of ball_query_launch
  using Source = std::conditional_t<LDS, ChannelMajor<float>, Cloud>;
  const int b = blockIdx.y;
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  const Cloud pts{points + (size_t)b * 3 * n, n}, ctr{centers + (size_t)b * 3 * m, m};
  if (LDS) {
    pts.stage(bq_planes, NT);
    __syncthreads();
  }
  const Source src{LDS ? bq_planes : pts.p, n};
  const int j0 = (blockIdx.x * (NT / 64) + wave) * cpw;
  for (int j = j0; j < min(j0 + cpw, m); ++j) {
    int *o = idx + ((size_t)b * m + j) * u;
    float cx, cy, cz;
    ctr.load(j, cx, cy, cz);
    int cnt = 0, first = 0;
    for (int base = 0; base < n && cnt < u; base += 64 * BQ_UNROLL) {
      float px[BQ_UNROLL], py[BQ_UNROLL], pz[BQ_UNROLL];
#pragma unroll
      for (int q = 0; q < BQ_UNROLL; ++q) src.load(min(base + q * 64 + lane, n - 1), px[q], py[q], pz[q]);
#pragma unroll
      for (int q = 0; q < BQ_UNROLL; ++q) {
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
    if (ZERO_FILL) {
      for (int v = lane; v < u; v += 64)
        if (v >= cnt) o[v] = cnt > 0 ? first : 0;
    } else if (cnt > 0) {
      for (int v = cnt + lane; v < u; v += 64) o[v] = first;
    }
  }
}

template <class Cloud, bool ZERO_FILL>
static int ball_query_launch(int b, int n, int m, float r2, int u, const float *centers, const float *points, int *idx,
                             hipStream_t s) {
  const size_t lds = (size_t)3 * n * sizeof(float);
  if (lds <= 144 * 1024 && (long)m * b >= 2048) {  // the cloud fits in LDS and there are enough centres to share it
    static bool once = false;
    if (!once) {
      (void)hipFuncSetAttribute((const void *)ball_query_kernel<Cloud, true, ZERO_FILL>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      once = true;
    }
    // centres per wave: about two workgroups per CU over the whole launch, at least 1
    int cpw = (int)(((long)m * b + 16L * 512 - 1) / (16L * 512));
    if (cpw < 1) cpw = 1;
    hipLaunchKernelGGL((ball_query_kernel<Cloud, true, ZERO_FILL>), dim3(cdiv(m, 16 * cpw), b), dim3(1024), lds, s, n, m,
                       r2, u, cpw, centers, points, idx);
    return p2pb_launch_status();
  }
  // from global memory: four waves per workgroup, one centre each
  hipLaunchKernelGGL((ball_query_kernel<Cloud, false, ZERO_FILL>), dim3(cdiv(m, 4), b), dim3(256), 0, s, n, m, r2, u, 1,
                     centers, points, idx);
  return p2pb_launch_status();
}

extern "C" int p2pb_ball_query(int b, int n, int m, float r2, int u, const float *centers, const float *points,
                               int *idx, void *stream) {
  if (b <= 0 || n <= 0 || m <= 0 || u <= 0) return P2PB_EINVAL;
  return ball_query_launch<ChannelMajor<float>, true>(b, n, m, r2, u, centers, points, idx, (hipStream_t)stream);
}

extern "C" int p2pb_pn2_ball_query(int b, int n, int m, float radius, int nsample, const float *new_xyz, const float *xyz,
                                   int *idx, void *stream) {
  if (b <= 0 || b > 65535 || n <= 0 || m <= 0 || nsample <= 0 || !new_xyz || !xyz || !idx) return P2PB_EINVAL;
  const float r2 = radius * radius;  // the float product of PN2/ball_query_gpu.cu:29
  return ball_query_launch<PointMajor<float>, false>(b, n, m, r2, nsample, new_xyz, xyz, idx, (hipStream_t)stream);
}
