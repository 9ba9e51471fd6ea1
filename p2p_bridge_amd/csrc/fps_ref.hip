// fps_ref.hip -- furthest point sampling in the order of the reference's two point-major samplers, one kernel family
// behind both entry points (include/p2pb_hip.h):
//   p2pb_pn2_fps                      (PN2/sampling_gpu.cu:101; PN2 = third_party/openpoints/cpp/pointnet2_batch/src)
//     b clouds xyz f32[b,n,3], m samples each, idx i32[b,m] local to the cloud
//   p2pb_pointops_furthestsampling    (PO/sampling/sampling_cuda_kernel.cu:15; PO = .../cpp/pointops/src)
//     one packed cloud xyz f32[n,3] with cumulative ends offset i32[b], samples new_offset i32[b], idx i32[m] global
// (The PVCNN sampler's own FPS, on channel-major clouds and with a 512-thread tie order, is sampling.hip.)
//
// Contract of both: temp / tmp f32, one per point, is the caller's running minima, read on entry (the layers fill it with
// 1e10) and written back once at the end, so it returns holding the minima over all samples but the last (the last pick
// starts no round); a segment asked for one sample leaves it untouched. The first sample is the segment's first point.
// Tie order: the reference's block has T = min(2^floor(log2 n), 1024) threads (PN2/cuda_utils.h:10; n is n_max on the
// packed entry), thread t scans k = t, t + T, ... keeping the first strict maximum, and its shared-memory tree keeps the
// lower thread on ties (PN2/sampling_gpu.cu:93-98): (minimum desc, k mod T asc, k asc) over the segment's LOCAL indices,
// the low word of fps_key_lt (fps_key.h).
//
// One workgroup per segment. A segment of up to THREADS * PPT points keeps coordinates and running minima in registers for
// the whole kernel, the winner's coordinates come from an LDS copy of the segment when the launch's longest one fits;
// above 16384 points the minima live in temp itself and the points are streamed from L2 every round.
#include "common.h"
#include "fps_key.h"
#include "po_segment.h"

// where a workgroup's segment lies: the two entry points differ in nothing else
struct FpsSegment {
  const float *c;  // its points [len][3]
  float *tp;       // their running minima
  int *out;        // its samples [ms]
  int len, ms;
  int first;  // added to the local indices written to out
};
template <bool PACKED>
__device__ __forceinline__ FpsSegment fps_segment(int n, int m, const float *__restrict__ xyz, const int *__restrict__ offset,
                                                  const int *__restrict__ new_offset, float *__restrict__ tmp,
                                                  int *__restrict__ idx) {
  const int s = blockIdx.x;
  FpsSegment g;
  if constexpr (PACKED) {  // ends clamped to [0, n] and [0, m], an end below its start is an empty segment
    int start_n, end_n;
    po_segment_points(s, n, offset, start_n, end_n);
    const int start_m = s ? po_clamp(new_offset[s - 1], 0, m) : 0;
    g.c = xyz + (size_t)3 * start_n;
    g.tp = tmp + start_n;
    g.out = idx + start_m;
    g.len = end_n - start_n;
    g.ms = po_clamp(new_offset[s], start_m, m) - start_m;
    g.first = start_n;
  } else {
    g.c = xyz + (size_t)s * 3 * n;
    g.tp = tmp + (size_t)s * n;
    g.out = idx + (size_t)s * m;
    g.len = n;
    g.ms = m;
    g.first = 0;
  }
  return g;
}

// the streaming body: minima in tp, points from L2
template <int THREADS>
__device__ __forceinline__ void fps_ref_stream(const FpsSegment &g, int lt, u64 *slots) {
  const int t = threadIdx.x, len = g.len;
  const float *__restrict__ c = g.c;
  float *__restrict__ tp = g.tp;
  int old = 0;
  for (int j = 1; j < g.ms; ++j) {
    const float x1 = c[(size_t)3 * old], y1 = c[(size_t)3 * old + 1], z1 = c[(size_t)3 * old + 2];
    float best = -1.0f;
    int bk = t;
    for (int k = t; k < len; k += THREADS) {  // (THREADS is a multiple of T: the thread's points share k mod T)
      const float d = sqdist3(c[(size_t)3 * k] - x1, c[(size_t)3 * k + 1] - y1, c[(size_t)3 * k + 2] - z1);
      const float d2 = fminf(d, tp[k]);
      tp[k] = d2;
      if (d2 > best) {
        best = d2;
        bk = k;
      }
    }
    // (a thread without points offers the identity, not an index: whatever temp holds, the winner is a point of the segment)
    u64 key = max_u64<true>(bk < len ? fps_key_lt(best, bk, lt) : 0);
    if (THREADS > 64) key = block_max(key, slots, j, t);
    old = fps_key_lt_index(key, lt);
    if (t == 0) g.out[j] = g.first + old;
  }
}

// PPT > 0, the register form: thread t owns k = t + i * THREADS. With PPT > 1 the launcher uses 1024 threads and n > 1024,
// so T = 1024: the thread's points share k mod T and are visited in ascending k, and "first strict maximum" inside the
// thread is the tie order. PPT == 0: the streaming form only.
// cap: the longest segment the register form takes -- THREADS * PPT, or the points the LDS copy was sized for. Only a
// packed launch can meet a longer one (an n_max that announces less than a segment holds); it STREAMS that segment, so
// the round loop below has no second source for the winner's coordinates and nothing longer than cap is copied to LDS.
template <int THREADS, int PPT, bool LDS_XYZ, bool PACKED>
__global__ __launch_bounds__(THREADS) void fps_ref_kernel(int n, int m, int lt, int cap, const float *__restrict__ xyz,
                                                          const int *__restrict__ offset,
                                                          const int *__restrict__ new_offset, float *__restrict__ tmp,
                                                          int *__restrict__ idx) {
  extern __shared__ __attribute__((aligned(16))) char fps_ref_smem[];
  u64 *slots = (u64 *)fps_ref_smem;                              // [2][16]
  float *sxyz = (float *)(fps_ref_smem + 2 * 16 * sizeof(u64));  // [cap][3] when LDS_XYZ
  const int t = threadIdx.x;
  const FpsSegment g = fps_segment<PACKED>(n, m, xyz, offset, new_offset, tmp, idx);
  const int len = g.len, ms = g.ms;
  if (len == 0 || ms == 0) return;  // (the whole workgroup)
  const float *__restrict__ c = g.c;
  float *__restrict__ tp = g.tp;
  if (t < 32) slots[t] = 0;
  if (t == 0) g.out[0] = g.first;
  if constexpr (PPT == 0) {
    __syncthreads();
    fps_ref_stream<THREADS>(g, lt, slots);
  } else {
    if (PACKED && len > cap) {
      __syncthreads();
      fps_ref_stream<THREADS>(g, lt, slots);
      return;
    }
    float x[PPT], y[PPT], z[PPT], dist[PPT];
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
      const int k = t + i * THREADS;
      const bool ok = k < len;
      x[i] = ok ? c[3 * k] : 0.0f;
      y[i] = ok ? c[3 * k + 1] : 0.0f;
      z[i] = ok ? c[3 * k + 2] : 0.0f;
      dist[i] = ok ? tp[k] : -1.0f;  // -1 = "no point here": stays -1, never selected
    }
    if (LDS_XYZ)
      for (int k = t; k < 3 * len; k += THREADS) sxyz[k] = c[k];
    __syncthreads();

    int old = 0;
    for (int j = 1; j < ms; ++j) {
      float x1, y1, z1;
      if (LDS_XYZ) {
        x1 = sxyz[3 * old];
        y1 = sxyz[3 * old + 1];
        z1 = sxyz[3 * old + 2];
      } else {
        x1 = c[3 * old];
        y1 = c[3 * old + 1];
        z1 = c[3 * old + 2];
      }
      float best = -1.0f;
      int bi = 0;
#pragma unroll
      for (int i = 0; i < PPT; ++i) {
        // (the bare v_min_f32, no canonicalising v_max_f32 in front: sampling.hip fps_kernel)
        const float d2 = vmin_raw(sqdist3(x[i] - x1, y[i] - y1, z[i] - z1), dist[i]);
        dist[i] = d2;
        if (d2 > best) {
          best = d2;
          bi = i;
        }
      }
      const int bk = t + bi * THREADS;
      u64 key = max_u64<true>(bk < len ? fps_key_lt(best, bk, lt) : 0);
      if (THREADS > 64) key = block_max(key, slots, j, t);
      old = fps_key_lt_index(key, lt);
      if (t == 0) g.out[j] = g.first + old;
    }
    if (ms > 1) {
#pragma unroll
      for (int i = 0; i < PPT; ++i) {
        const int k = t + i * THREADS;
        if (k < len) tp[k] = dist[i];
      }
    }
  }
}

// npts: n of the batched entry, n_max of the packed one; npts <= THREADS * PPT when PPT > 0
#define FPS_REF_LDS_MAX (160 * 1024)
template <int THREADS, int PPT, bool PACKED>
static void fps_ref_launch(int b, int n, int m, int npts, int lt, const float *xyz, const int *offset, const int *new_offset,
                           float *tmp, int *idx, hipStream_t s) {
  const size_t base = 2 * 16 * sizeof(u64), cloud = (size_t)3 * npts * sizeof(float);
  if constexpr (PPT > 0) {
    if (base + cloud <= FPS_REF_LDS_MAX) {
      // (on every such launch: the attribute belongs to the current device, and the call is cheap)
      if (base + cloud > 64 * 1024)
        (void)hipFuncSetAttribute((const void *)fps_ref_kernel<THREADS, PPT, true, PACKED>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, FPS_REF_LDS_MAX);
      hipLaunchKernelGGL((fps_ref_kernel<THREADS, PPT, true, PACKED>), dim3(b), dim3(THREADS), base + cloud, s, n, m, lt, npts,
                         xyz, offset, new_offset, tmp, idx);
      return;
    }
  }
  hipLaunchKernelGGL((fps_ref_kernel<THREADS, PPT, false, PACKED>), dim3(b), dim3(THREADS), base, s, n, m, lt, THREADS * PPT,
                     xyz, offset, new_offset, tmp, idx);
}

template <bool PACKED>
static void fps_ref_dispatch(int b, int n, int m, int npts, const float *xyz, const int *offset, const int *new_offset,
                             float *tmp, int *idx, hipStream_t s) {
  int lt = 0;  // log2 T(npts)
  while (lt < 10 && (2 << lt) <= npts) ++lt;
  if (npts <= 64) fps_ref_launch<64, 1, PACKED>(b, n, m, npts, lt, xyz, offset, new_offset, tmp, idx, s);
  else if (npts <= 256) fps_ref_launch<256, 1, PACKED>(b, n, m, npts, lt, xyz, offset, new_offset, tmp, idx, s);
  else if (npts <= 1024) fps_ref_launch<1024, 1, PACKED>(b, n, m, npts, lt, xyz, offset, new_offset, tmp, idx, s);
  else if (npts <= 2048) fps_ref_launch<1024, 2, PACKED>(b, n, m, npts, lt, xyz, offset, new_offset, tmp, idx, s);
  else if (npts <= 4096) fps_ref_launch<1024, 4, PACKED>(b, n, m, npts, lt, xyz, offset, new_offset, tmp, idx, s);
  else if (npts <= 8192) fps_ref_launch<1024, 8, PACKED>(b, n, m, npts, lt, xyz, offset, new_offset, tmp, idx, s);
  else if (npts <= 16384) fps_ref_launch<1024, 16, PACKED>(b, n, m, npts, lt, xyz, offset, new_offset, tmp, idx, s);
  else fps_ref_launch<1024, 0, PACKED>(b, n, m, npts, lt, xyz, offset, new_offset, tmp, idx, s);
}

extern "C" int p2pb_pn2_fps(int b, int n, int m, const float *xyz, float *temp, int *idx, void *stream) {
  if (b <= 0 || n <= 0 || m < 0) return P2PB_EINVAL;
  if (m == 0) return 0;  // (PN2/sampling_gpu.cu:108: nothing is written; idx i32[b,0] has no address)
  if (!xyz || !temp || !idx) return P2PB_EINVAL;
  fps_ref_dispatch<false>(b, n, m, n, xyz, nullptr, nullptr, temp, idx, (hipStream_t)stream);
  return p2pb_launch_status();
}

extern "C" int p2pb_pointops_furthestsampling(int b, int n, int m, int n_max, const float *xyz, const int *offset,
                                              const int *new_offset, float *tmp, int *idx, void *stream) {
  if (b < 0 || n < 0 || m < 0) return P2PB_EINVAL;
  if (b == 0 || n == 0 || m == 0) return 0;
  if (n_max < 1 || !xyz || !offset || !new_offset || !tmp || !idx) return P2PB_EINVAL;
  fps_ref_dispatch<true>(b, n, m, n_max, xyz, offset, new_offset, tmp, idx, (hipStream_t)stream);
  return p2pb_launch_status();
}
