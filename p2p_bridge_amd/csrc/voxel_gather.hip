// voxel_gather.hip -- the feature half of the point -> voxel kernels for gfx950: a voxel's mean over the sorted point
// lists of p2pb_voxel_sort (voxel_coords.hip).
//   p2pb_avg_voxelize_forward/backward      (PN2/vox_gpu.cu:18,50,92)
//   p2pb_avg_voxelize_cl_gather(_split)     the voxel-major forms of the fused inference branch
#include "voxel_common.h"

// a voxel's point ids (ascending), their number, and the reciprocal every gather multiplies by
struct VoxSeg {
  const int *seg;
  int cn;
  float div;
};

__device__ __forceinline__ VoxSeg vox_segment(const int *__restrict__ cnt, const int *__restrict__ cur,
                                              const int *__restrict__ slist, int b, int n, int r3, int v) {
  VoxSeg s;
  s.cn = cnt[(size_t)b * r3 + v];
  s.seg = slist + (size_t)b * n + (cur[(size_t)b * r3 + v] - s.cn);  // cur points at the segment end after the fill
  s.div = (float)(1.0 / (double)(float)s.cn);  // PN2/vox_gpu.cu:70 divides a double literal
  return s;
}

// one wave per non-empty voxel, lane = channel (steps 5 and 6 of the list in voxel_coords.hip)
__global__ __launch_bounds__(256) void vox_gather_kernel(int c, int n, int r3, const int *__restrict__ cnt,
                                                         const int *__restrict__ cur, const int *__restrict__ occ,
                                                         const int *__restrict__ nocc, const int *__restrict__ slist,
                                                         const float *__restrict__ feat, float *__restrict__ out) {
  const int b = blockIdx.y;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= nocc[b]) return;
  const int lane = lane_id();
  const int v = occ[(size_t)b * n + k];
  const VoxSeg s = vox_segment(cnt, cur, slist, b, n, r3, v);
  const float *f = feat + (size_t)b * c * n;
  float *o = out + (size_t)b * c * r3 + v;
  for (int c0 = 0; c0 < c; c0 += 64) {
    const int ch = c0 + lane;
    if (ch < c) {
      const float *fj = f + (size_t)ch * n;
      float acc = 0.0f;
      for (int q = 0; q < s.cn; ++q) acc += fj[s.seg[q]] * s.div;
      o[(size_t)ch * r3] = acc;
    }
  }
}

extern "C" int p2pb_avg_voxelize_forward(int b, int c, int n, int r, const int *coords, const float *feat, int *ind,
                                         int *cnt, float *out, void *ws, void *stream) {
  if (c <= 0) return P2PB_EINVAL;
  int e = p2pb_voxel_sort(b, n, r, coords, ind, cnt, ws, stream);
  if (e != 0) return e;
  hipStream_t s = (hipStream_t)stream;
  const int r3 = r * r * r;
  VoxWs w;
  vox_ws_carve(ws, b, n, r3, &w);
  e = p2pb_zero_async(out, sizeof(float) * (size_t)b * c * r3, s);
  if (e != 0) return e;
  const int maxocc = n < r3 ? n : r3;
  hipLaunchKernelGGL(vox_gather_kernel, dim3(cdiv(maxocc, 4), b), dim3(256), 0, s, c, n, r3, cnt, w.cur, w.occ, w.nocc,
                     w.slist, feat, out);
  return p2pb_launch_status();
}

// ------------------------------------------------------------------------------------------------
// Voxel-major variants for the fused inference branch (grid f32[b, r^3, c], a voxel's channels contiguous):
// the convolutions stage and store contiguous channel runs, and both ends of the branch become coalesced:
//   voxelize : features are first transposed to point-major [b, n, c] (LDS tile transpose), then one wave per
//              occupied voxel reads whole 4c-byte point rows (lane = channel) and writes one contiguous row --
//              the channel-major form reads and writes 4 bytes per 32-byte sector on both sides;
//   devoxelize (devoxelize.hip): lane = channel reads the 8 corner rows, results go through an LDS transpose so the
//              channel-major output [b, c, n] is written in 256-byte runs.
// Same arithmetic, same summation order as the reference-layout kernels (bit-identical values).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void transpose_cn_kernel(int c, int n, const float *__restrict__ in,
                                                           float *__restrict__ out) {
  __shared__ float t[32][33];
  const int b = blockIdx.z, n0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const float *src = in + (size_t)b * c * n;
  float *dst = out + (size_t)b * c * n;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int cc = c0 + ty + 8 * k, nn = n0 + tx;
    t[ty + 8 * k][tx] = (cc < c && nn < n) ? src[(size_t)cc * n + nn] : 0.0f;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int nn = n0 + ty + 8 * k, cc = c0 + tx;
    if (cc < c && nn < n) dst[(size_t)nn * c + cc] = t[tx][ty + 8 * k];
  }
}

// the whole grid in one pass: a thread owns V consecutive channels of one voxel -- zeros for an empty voxel, the
// ascending-order mean (same arithmetic as above) otherwise; replaces zero-fill + gather over the occupied list
// ALIGNED: c % 4 == 0, 16-byte loads / stores; else (e.g. the 3 + 32 channels of the first PVConv) a thread still owns
// four consecutive channels -- one occupancy lookup per quad -- but moves them as scalars and clips the last quad
template <bool ALIGNED>
__global__ __launch_bounds__(256) void vox_gather_cl_all_kernel(int c, int n, int r3, const int *__restrict__ cnt,
                                                                const int *__restrict__ cur,
                                                                const int *__restrict__ slist,
                                                                const float *__restrict__ feat_t,
                                                                float *__restrict__ out) {
  const int b = blockIdx.y, cv = (c + 3) / 4;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)r3 * cv) return;
  const int v = (int)(e / cv), ch = (int)(e % cv) * 4;
  const int nch = min(4, c - ch);
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (cnt[(size_t)b * r3 + v] > 0) {
    const VoxSeg s = vox_segment(cnt, cur, slist, b, n, r3, v);
    const float *f = feat_t + (size_t)b * n * c + ch;
    for (int q = 0; q < s.cn; ++q) {
      const float *fq = f + (size_t)s.seg[q] * c;
      if (ALIGNED) {
        const f32x4 x = *(const f32x4 *)fq;
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += x[i] * s.div;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i < nch) acc[i] += fq[i] * s.div;
      }
    }
  }
  float *o = out + ((size_t)b * r3 + v) * c + ch;
  if (ALIGNED) {
    *(f32x4 *)o = f32x4{acc[0], acc[1], acc[2], acc[3]};
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < nch) o[i] = acc[i];
  }
}

// Occupied voxels only, after a streaming zero-fill of the grid (p2pb_zero_async: 16 B per lane, 7 TB/s into the
// memory-side cache for the 134 MB level-0 grid of the bench; the one-pass kernels above visit every voxel and write the
// same bytes at 1 TB/s: 145 us against 18 + ~10). A thread owns one float of one occupied voxel's row; same arithmetic
// and summation order as the one-pass kernels.
__global__ __launch_bounds__(256) void vox_gather_cl_occ_kernel(int c, int n, int r3, const int *__restrict__ cnt,
                                                                const int *__restrict__ cur,
                                                                const int *__restrict__ occ,
                                                                const int *__restrict__ nocc,
                                                                const int *__restrict__ slist,
                                                                const float *__restrict__ feat_t,
                                                                float *__restrict__ out) {
  const int b = blockIdx.y;
  const size_t total = (size_t)nocc[b] * c;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int k = (int)(e / c), ch = (int)(e % c);
    const int v = occ[(size_t)b * n + k];
    const VoxSeg s = vox_segment(cnt, cur, slist, b, n, r3, v);
    const float *f = feat_t + (size_t)b * n * c + ch;
    float acc = 0.0f;
    for (int q = 0; q < s.cn; ++q) acc += f[(size_t)s.seg[q] * c] * s.div;
    out[((size_t)b * r3 + v) * c + ch] = acc;
  }
}

// The grid straight in the pre-split operand format of the voxel convolutions (conv3d_split.h "S format"): out
// u32x4[b][r^3][ceil(c/16)][2 planes][2 khalf], the fp16 pair (h0 | h1) of 4 x mean for channels chunk*16 + khalf*8 + i --
// 4 bytes per (voxel, channel) like the fp32 grid, channels padded with zeros to a multiple of 16. A thread owns 8
// consecutive channels (ch = 8 g .. 8 g + 7) of one voxel v; same means (ascending point order) as the kernels above, then
// the split the convolution's staging phase would apply -- the first convolution of a PVConv then stages with LDS-DMA alone.
// The thread is LATENCY-bound by its voxel's points: it adds them one after the other (ascending index: the reference's
// mean, bit for bit), and point by point every point was two dependent L2 round trips (list entry -> row: 150-170 us
// whatever the batch; profiles/r07_gather_wait_audit.txt). The list entries and rows of FOUR points are in flight before
// the first is added; the additions keep their order.
// ALL: the thread belongs to the one-pass form, whose voxel may be empty and whose 8 channels may lie past c (the padding of
// the last chunk): it then writes all-zero bits, and looks the segment up only behind the occupancy test (as
// vox_gather_cl_all_kernel does: an empty voxel costs one load). The occupied form never meets the first; for the second its
// masked loads give zeros and the sums stay +0.
template <bool ALIGNED, bool ALL>
__device__ __forceinline__ void vox_gather_split_thread(int c, int nchunk, int n, int r3, const int *__restrict__ cnt,
                                                        const int *__restrict__ cur, const int *__restrict__ slist,
                                                        const float *__restrict__ feat_t, u32x4 *__restrict__ out, int b, int v,
                                                        int g) {
  const int ch = g * 8;
  float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (!ALL || (cnt[(size_t)b * r3 + v] > 0 && ch < c)) {
    const VoxSeg s = vox_segment(cnt, cur, slist, b, n, r3, v);
    const float *f = feat_t + (size_t)b * n * c + ch;
    for (int q0 = 0; q0 < s.cn; q0 += 4) {
      int id[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) id[u] = s.seg[min(q0 + u, s.cn - 1)];
      float x[4][8];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float *fq = f + (size_t)id[u] * c;
        if (ALIGNED) {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            f32x4 y = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (ch + 4 * h < c) y = *(const f32x4 *)(fq + 4 * h);
#pragma unroll
            for (int i = 0; i < 4; ++i) x[u][4 * h + i] = y[i];
          }
        } else {
#pragma unroll
          for (int i = 0; i < 8; ++i) x[u][i] = ch + i < c ? fq[i] : 0.0f;
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (q0 + u < s.cn) {
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[i] += x[u][i] * s.div;
        }
    }
  }
  u32x4 p0, p1;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    unsigned a0, a1, a2;
    split_pair<SPLIT_F16X3>(acc[2 * i], acc[2 * i + 1], a0, a1, a2);
    p0[i] = a0;
    p1[i] = a1;
  }
  u32x4 *dst = out + (((size_t)b * r3 + v) * nchunk + (g >> 1)) * 4 + (g & 1);
  dst[0] = p0;
  dst[2] = p1;
}

// every voxel in one pass (zeros for the empty ones)
template <bool ALIGNED>
__global__ __launch_bounds__(256) void vox_gather_cl_split_kernel(int c, int nchunk, int n, int r3,
                                                                  const int *__restrict__ cnt, const int *__restrict__ cur,
                                                                  const int *__restrict__ slist,
                                                                  const float *__restrict__ feat_t, u32x4 *__restrict__ out) {
  const int b = blockIdx.y, ng = nchunk * 2;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)r3 * ng) return;
  vox_gather_split_thread<ALIGNED, true>(c, nchunk, n, r3, cnt, cur, slist, feat_t, out, b, (int)(e / ng), (int)(e % ng));
}

// Occupied voxels only, after a streaming zero-fill of the split grid (the fp16 pair of 0 is all-zero bits): the form for
// channel counts that are not a multiple of 4 (the 3 + 32 channels of the first PVConv: scalar point-row loads) and, since round 5,
// for every r = 32 grid (at most a quarter of the voxels is occupied: the one-pass kernel above wrote the 268 MB of the 64-channel
// level-0 grid at 1.2 TB/s, 226 us per 32 patches; the zero-fill streams at ~7 TB/s).
template <bool ALIGNED>
__global__ __launch_bounds__(256) void vox_gather_cl_occ_split_kernel(int c, int nchunk, int n, int r3,
                                                                      const int *__restrict__ cnt, const int *__restrict__ cur,
                                                                      const int *__restrict__ occ, const int *__restrict__ nocc,
                                                                      const int *__restrict__ slist,
                                                                      const float *__restrict__ feat_t, u32x4 *__restrict__ out) {
  const int b = blockIdx.y, ng = nchunk * 2;
  const size_t total = (size_t)nocc[b] * ng;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int k = (int)(e / ng), g = (int)(e % ng);
    vox_gather_split_thread<ALIGNED, false>(c, nchunk, n, r3, cnt, cur, slist, feat_t, out, b, occ[(size_t)b * n + k], g);
  }
}

// The feature half: out f32[b, r^3, c] (voxel-major) from feat f32[b,c,n] and the sort of p2pb_voxel_sort
// (cnt, ws); feat_t f32[b, n, c] scratch
extern "C" int p2pb_avg_voxelize_cl_gather(int b, int c, int n, int r, const float *feat, const int *cnt, const void *ws,
                                           float *out, float *feat_t, void *stream) {
  if (b <= 0 || c <= 0 || n <= 0 || r <= 0 || !ws || !feat_t) return P2PB_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int r3 = r * r * r;
  VoxWs w;
  vox_ws_carve(ws, b, n, r3, &w);
  const int maxocc = n < r3 ? n : r3;
  hipLaunchKernelGGL(transpose_cn_kernel, dim3(cdiv(n, 32), cdiv(c, 32), b), dim3(256), 0, s, c, n, feat, feat_t);
  // rows of whole 16-byte quads: one pass over every voxel (zeros for the empty ones). Other channel counts (the 3 + 32
  // channels of the first PVConv): zero-fill + the occupied voxels only -- measured 181 vs 234 us for the whole
  // voxelisation at the bench's level-0 shape; for aligned rows the one-pass form is as fast or faster (tools/exp_voxelize.py)
  static const int onepass = (int)p2pb_experiment_long("vox_onepass", -1);  // (A/B switch: 0 / 1 force)
  if (onepass == 0 || (onepass < 0 && (c & 3) != 0)) {
    const int e = p2pb_zero_async(out, (size_t)b * r3 * c * sizeof(float), s);
    if (e != 0) return e;
    const size_t nwg = cdiv((size_t)maxocc * c, 256);
    hipLaunchKernelGGL(vox_gather_cl_occ_kernel, dim3((unsigned)(nwg > 65536 ? 65536 : nwg), b), dim3(256), 0, s, c, n, r3,
                       cnt, w.cur, w.occ, w.nocc, w.slist, feat_t, out);
    return p2pb_launch_status();
  }
  const dim3 grid((unsigned)cdiv((size_t)r3 * ((c + 3) / 4), 256), b);
  if ((c & 3) == 0)
    hipLaunchKernelGGL(vox_gather_cl_all_kernel<true>, grid, dim3(256), 0, s, c, n, r3, cnt, w.cur, w.slist, feat_t, out);
  else
    hipLaunchKernelGGL(vox_gather_cl_all_kernel<false>, grid, dim3(256), 0, s, c, n, r3, cnt, w.cur, w.slist, feat_t, out);
  return p2pb_launch_status();
}

// The feature half, straight into the pre-split operand format (S format) of the voxel convolutions:
// out_split b * r^3 * ceil(c/16) * 64 bytes; feat_t f32[b, n, c] scratch
extern "C" int p2pb_avg_voxelize_cl_gather_split(int b, int c, int n, int r, const float *feat, const int *cnt, const void *ws,
                                                 void *out_split, float *feat_t, void *stream) {
  if (b <= 0 || c <= 0 || n <= 0 || r <= 0 || !ws || !feat_t || !out_split) return P2PB_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int r3 = r * r * r, nchunk = (c + 15) / 16;
  VoxWs w;
  vox_ws_carve(ws, b, n, r3, &w);
  hipLaunchKernelGGL(transpose_cn_kernel, dim3(cdiv(n, 32), cdiv(c, 32), b), dim3(256), 0, s, c, n, feat, feat_t);
  static const int onepass = (int)p2pb_experiment_long("vox_onepass", -1);  // (A/B switch: 0 / 1 force)
  // zero-fill + occupied voxels only: ragged rows (the rule of p2pb_avg_voxelize_cl_gather) and every grid with at least four
  // voxels per point (r = 32 at 8192 points: <= 25 % occupied)
  if (onepass == 0 || (onepass < 0 && ((c & 3) != 0 || (size_t)r3 >= 4 * (size_t)n))) {
    const int maxocc = n < r3 ? n : r3;
    const int e = p2pb_zero_async(out_split, (size_t)b * r3 * nchunk * 64, s);
    if (e != 0) return e;
    const size_t nwg = cdiv((size_t)maxocc * nchunk * 2, 256);
    const dim3 g((unsigned)(nwg > 65536 ? 65536 : nwg), b);
    if ((c & 3) == 0)
      hipLaunchKernelGGL(vox_gather_cl_occ_split_kernel<true>, g, dim3(256), 0, s, c, nchunk, n, r3, cnt, w.cur, w.occ, w.nocc,
                         w.slist, feat_t, (u32x4 *)out_split);
    else
      hipLaunchKernelGGL(vox_gather_cl_occ_split_kernel<false>, g, dim3(256), 0, s, c, nchunk, n, r3, cnt, w.cur, w.occ, w.nocc,
                         w.slist, feat_t, (u32x4 *)out_split);
    return p2pb_launch_status();
  }
  const dim3 grid((unsigned)cdiv((size_t)r3 * nchunk * 2, 256), b);
  if ((c & 3) == 0)
    hipLaunchKernelGGL(vox_gather_cl_split_kernel<true>, grid, dim3(256), 0, s, c, nchunk, n, r3, cnt, w.cur, w.slist, feat_t,
                       (u32x4 *)out_split);
  else
    hipLaunchKernelGGL(vox_gather_cl_split_kernel<false>, grid, dim3(256), 0, s, c, nchunk, n, r3, cnt, w.cur, w.slist, feat_t,
                       (u32x4 *)out_split);
  return p2pb_launch_status();
}

// both halves: out f32[b, r^3, c] (voxel-major); feat_t f32[b, n, c] scratch; everything else as p2pb_avg_voxelize_forward
extern "C" int p2pb_avg_voxelize_cl_forward(int b, int c, int n, int r, const int *coords, const float *feat, int *ind,
                                            int *cnt, float *out, float *feat_t, void *ws, void *stream) {
  const int e = p2pb_voxel_sort(b, n, r, coords, ind, cnt, ws, stream);
  if (e != 0) return e;
  return p2pb_avg_voxelize_cl_gather(b, c, n, r, feat, cnt, ws, out, feat_t, stream);
}

template <int CC>
__global__ __launch_bounds__(256) void vox_grad_kernel(int c, int n, int r3, const int *__restrict__ ind,
                                                       const int *__restrict__ cnt, const float *__restrict__ gy,
                                                       float *__restrict__ gx) {
  const int b = blockIdx.z;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c0 = blockIdx.y * CC, c1 = min(c0 + CC, c);
  const int pos = ind[(size_t)b * n + i];
  const int cn = cnt[(size_t)b * r3 + pos];
  const float div = cn > 0 ? (float)(1.0 / (double)(float)cn) : 0.0f;
  const float *g = gy + (size_t)b * c * r3 + pos;
  float *o = gx + (size_t)b * c * n + i;
  for (int j = c0; j < c1; ++j) o[(size_t)j * n] = cn > 0 ? g[(size_t)j * r3] * div : 0.0f;
}

extern "C" int p2pb_avg_voxelize_backward(int b, int c, int n, int r3, const int *ind, const int *cnt,
                                          const float *grad_y, float *grad_x, void *stream) {
  if (b <= 0 || c <= 0 || n <= 0 || r3 <= 0) return P2PB_EINVAL;
  constexpr int CC = 16;
  hipLaunchKernelGGL(vox_grad_kernel<CC>, dim3(cdiv(n, 256), cdiv(c, CC), b), dim3(256), 0, (hipStream_t)stream, c, n,
                     r3, ind, cnt, grad_y, grad_x);
  return p2pb_launch_status();
}
