// neighbors.hip -- grouping / gather kernels of the set abstraction and feature propagation for gfx950.
//   p2pb_grouping_forward            (PN2/pvcnn_grouping_gpu.cu:18)
//   p2pb_gather_features_forward     (PN2/pvcnn_sampling_gpu.cu:17)
//   p2pb_group_concat, p2pb_group_sub, p2pb_group_sub_stats, p2pb_three_interpolate_add: the fused forms of the sampler
// (their backward passes: scatter_grad.hip; the searches that produce the indices: ball_query.hip, three_nn.hip, which also
// holds the plain three-interpolate)
// The reference runs ONE thread block per cloud for each of these; here every kernel is spread over
// (points or centres) x channels x batch so a B=32 launch covers all 256 CUs.
#include "common.h"

// ------------------------------------------------------------------------------------------------
// grouping: out[b,c,j,k] = feat[b,c,idx[b,j,k]] . One thread per (j,k) slot, looping a chunk of
// channels: the index is read once, the 32x write amplification goes out as lane-consecutive stores.
// ------------------------------------------------------------------------------------------------
template <int CC>
__global__ __launch_bounds__(256) void grouping_kernel(int c, int n, int mu, const float *__restrict__ feat,
                                                       const int *__restrict__ idx, float *__restrict__ out) {
  const int b = blockIdx.z;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= mu) return;
  const int id = idx[(size_t)b * mu + q];
  const int c0 = blockIdx.y * CC, c1 = min(c0 + CC, c);
  for (int l = c0; l < c1; ++l) out[((size_t)b * c + l) * mu + q] = feat[((size_t)b * c + l) * n + id];
}

extern "C" int p2pb_grouping_forward(int b, int c, int n, int m, int u, const float *feat, const int *idx, float *out,
                                     void *stream) {
  if (b <= 0 || c <= 0 || n <= 0 || m <= 0 || u <= 0) return P2PB_EINVAL;
  constexpr int CC = 8;
  hipLaunchKernelGGL(grouping_kernel<CC>, dim3(cdiv((long)m * u, 256), cdiv(c, CC), b), dim3(256), 0,
                     (hipStream_t)stream, c, n, m * u, feat, idx, out);
  return p2pb_launch_status();
}

// set-abstraction operand in one pass: out[b, 0:3, j, k] = coords[b, :, idx] - centers[b, :, j] (relative
// neighbour coordinates, models/pvcnn.py:117-118) and out[b, 3:, j, k] = feat[b, :, idx] (:124-126), i.e.
// grouping x2 + subtract + concat of the unfused graph without the two intermediate tensors
template <int CC>
__global__ __launch_bounds__(256) void group_concat_kernel(int c, int n, int m, int u,
                                                           const float *__restrict__ coords,
                                                           const float *__restrict__ centers,
                                                           const float *__restrict__ feat, const int *__restrict__ idx,
                                                           float *__restrict__ out) {
  const int b = blockIdx.z;
  const int mu = m * u;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= mu) return;
  const int id = idx[(size_t)b * mu + q];
  const int j = q / u;
  const int ct = 3 + c;
  const int c0 = blockIdx.y * CC, c1 = min(c0 + CC, ct);
  for (int l = c0; l < c1; ++l) {
    float v;
    if (l < 3) v = coords[((size_t)b * 3 + l) * n + id] - centers[((size_t)b * 3 + l) * m + j];
    else v = feat[((size_t)b * c + (l - 3)) * n + id];
    out[((size_t)b * ct + l) * mu + q] = v;
  }
}

extern "C" int p2pb_group_concat(int b, int c, int n, int m, int u, const float *coords, const float *centers,
                                 const float *feat, const int *idx, float *out, void *stream) {
  if (b <= 0 || c < 0 || n <= 0 || m <= 0 || u <= 0) return P2PB_EINVAL;
  constexpr int CC = 8;
  hipLaunchKernelGGL(group_concat_kernel<CC>, dim3(cdiv((long)m * u, 256), cdiv(3 + c, CC), b), dim3(256), 0,
                     (hipStream_t)stream, c, n, m, u, coords, centers, feat, idx, out);
  return p2pb_launch_status();
}

// ------------------------------------------------------------------------------------------------
// First layer of a set-abstraction MLP applied BEFORE the grouping (inference): a 1x1 convolution is linear, so
//   W [xyz[idx] - centre ; f[idx]] + bias  =  Z[:, idx] - Cx[:, centre],   Z = W [xyz ; f] + bias (N points),
//                                                                          Cx = W_xyz centre (M centres),
// i.e. the GEMM runs on the N points instead of the M*U grouped positions (4x .. 32x fewer) and the
// (3+C)-channel grouped tensor of models/pvcnn.py:117-126 is never built. This kernel gathers the C1-channel
// result, subtracts the centre term and emits the {sum, sum of squares} partials of the GroupNorm that follows
// (one slot per half-wave = 32 positions; reduced in fixed order by gn_affine_kernel).
//   z f32[b,c,n], cx f32[b,c,m] (or NULL), idx i32[b,m,u] -> out f32[b,c,m*u], stats f32[b, nslots, c, 2]
// ------------------------------------------------------------------------------------------------
// [b, c, n] -> [b, n, c] (32 x 32 LDS tiles)
__global__ __launch_bounds__(256) void nb_transpose_kernel(int c, int n, const float *__restrict__ in,
                                                           float *__restrict__ out) {
  __shared__ float t[32][33];
  const int b = blockIdx.z, n0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
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

// Gathers run on POINT-MAJOR copies (zt f32[b,n,c], cxt f32[b,m,c]): lane = channel reads one contiguous row per
// neighbour (a channel-major gather touches 4 bytes per 64-byte line), 64 positions per workgroup go through an LDS
// transpose so the channel-major output is written in 256-byte runs; a wave then owns whole channel rows of the
// tile, and the statistics are two half-wave sums per row (slot = 32 positions).
__global__ __launch_bounds__(256) void group_sub_kernel(int c, int n, int m, int u, int nslots,
                                                        const float *__restrict__ zt, const float *__restrict__ cxt,
                                                        const int *__restrict__ idx, float *__restrict__ out,
                                                        float *__restrict__ stats) {
  __shared__ float tile[64][65];  // [channel][position]
  const int b = blockIdx.z, p0 = blockIdx.x * 64, t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int mu = m * u;
  // the wave's 16 neighbour indices (and centre rows) are fetched once, by lanes 0..15
  const int qmine = p0 + wave * 16 + (lane & 15);
  const int id_mine = qmine < mu ? idx[(size_t)b * mu + qmine] : -1;
  // narrow layers (c <= 32) gather two positions per step, one per half-wave
  const int cpl = c <= 32 ? 32 : 64, pps = 64 / cpl;
  const int sub = lane / cpl, chl = lane % cpl;
  {
    const int c0 = blockIdx.y * cpl;  // one channel chunk per workgroup (more workgroups on the small levels)
    const int ch = c0 + chl;
    // Loads are issued eight steps at a time, from clamped addresses, and the masking is a select afterwards: a load inside a
    // per-step branch is waited for (vmcnt(0)) before the next step issues its own, one L2 round trip per step
    // (profiles/r07_gather_wait_audit.txt). The centre index is advanced, not divided out per step.
    const float *zb = zt + (size_t)b * n * c + min(ch, c - 1);
    const float *cb = cxt ? cxt + (size_t)b * m * c + min(ch, c - 1) : nullptr;
    int cj = (p0 + wave * 16 + sub) / u, cr = (p0 + wave * 16 + sub) - cj * u;  // centre of the lane's first position, offset in it
    for (int it0 = 0; it0 < 16 / pps; it0 += 8) {
      int id[8];
      float zv[8], cv[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        id[k] = __shfl(id_mine, (it0 + k) * pps + sub);
        zv[k] = zb[(size_t)max(id[k], 0) * c];
        cv[k] = cb ? cb[(size_t)min(cj, m - 1) * c] : 0.0f;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const bool wrap = q < pps && cr + 1 == u;
          cr = wrap ? 0 : (q < pps ? cr + 1 : cr);
          cj += wrap ? 1 : 0;
        }
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int pl = wave * 16 + (it0 + k) * pps + sub;
        float v = zv[k];
        if (cb) v -= cv[k];
        tile[chl][pl] = (id[k] >= 0 && ch < c) ? v : 0.0f;
      }
    }
    __syncthreads();
    const int pt = lane;
    // a wave owns rows wave, wave + 4, ... (four waves write four adjacent output rows at a time: measured 15 % faster
    // than consecutive rows per wave)
    const int per = cpl / 4;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int cr = wave + 4 * k;
      const float v = tile[cr & 63][pt];  // zero outside the tensor: statistics unaffected
      if (k < per && c0 + cr < c) {
        if (out && p0 + pt < mu) out[((size_t)b * c + c0 + cr) * mu + p0 + pt] = v;  // (out == NULL: statistics only)
        const float s1 = halfwave_sum_to_last(v), s2 = halfwave_sum_to_last(v * v);
        if ((lane & 31) == 31) {
          float *p = stats + (((size_t)b * nslots + blockIdx.x * 2 + (lane >> 5)) * c + c0 + cr) * 2;
          p[0] = s1;
          p[1] = s2;
        }
      }
    }
    __syncthreads();
  }
}

// STATISTICS ONLY (the two-layer set abstractions: the consumer, pw_wide_kernel<GATHER>, gathers the grouped operand itself and
// only the GroupNorm partials of the grouped tensor are needed first). Round 5: this used to be group_sub_kernel with out == NULL --
// the LDS transpose that exists for the output's sake and ten DPP steps per channel row, 114 us for the first level of the bench;
// here a lane IS a channel: a wave walks its 128 positions, every lane adds its own {v, v * v} (v = z[idx] - cx, group_sub's
// arithmetic) in position order, and the partial of (sample, slot = wave, channel) is one store -- no LDS, no cross-lane step
// (two positions per step for c <= 32: the half-waves' sums are added once at the end). Slots of 128 positions: a quarter of the
// partials gn_affine has to reduce afterwards.
#define GST_PW 128
// Round 7: the loads of GST_NB steps are issued together, from clamped addresses, and the masking is a select on the two sums
// afterwards (same additions, same order): with `if (id >= 0 && chok) { load; load; add }` per step every step sat in its own
// exec-masked branch and its loads were waited for (vmcnt(0)) before the next step issued any -- a wave walked its slot as 64 or
// 128 dependent L2 round trips (profiles/r07_gather_wait_audit.txt). The neighbour index comes by v_readlane (uniform lane
// number: a scalar row base for c > 32) instead of ds_bpermute, the centre index is advanced instead of divided out per step.
#define GST_NB 16
template <int CPL, bool CX>
__global__ __launch_bounds__(256) void group_stats_kernel(int c, int n, int m, int u, int nslots, const float *__restrict__ zt,
                                                          const float *__restrict__ cxt, const int *__restrict__ idx,
                                                          float *__restrict__ stats) {
  constexpr int PPS = 64 / CPL;  // positions per step
  const int b = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = blockIdx.x * 4 + wave;
  if (slot >= nslots) return;
  const int mu = m * u, p0 = slot * GST_PW;
  const int sub = lane / CPL, ch = blockIdx.y * CPL + lane % CPL;
  // the wave's 128 neighbour indices: two per lane, handed round by lane reads
  const int ia = p0 + lane < mu ? idx[(size_t)b * mu + p0 + lane] : -1;
  const int ib = p0 + 64 + lane < mu ? idx[(size_t)b * mu + p0 + 64 + lane] : -1;
  const bool chok = ch < c;
  const float *zb = zt + (size_t)b * n * c + min(ch, c - 1);
  const float *cb = CX ? cxt + (size_t)b * m * c + min(ch, c - 1) : nullptr;
  int cj = (p0 + sub) / u, cr = (p0 + sub) - cj * u;  // centre of the lane's first position, offset inside its neighbourhood
  float s1 = 0.0f, s2 = 0.0f;
#pragma unroll 1
  for (int pb = 0; pb < GST_PW; pb += GST_NB * PPS) {  // (a batch lies in one half of the slot: ia or ib)
    const int src = pb < 64 ? ia : ib;
    int id[GST_NB];
    float zv[GST_NB], cv[GST_NB];
#pragma unroll
    for (int k = 0; k < GST_NB; ++k) {
      const int l = (pb & 63) + k * PPS;
      id[k] = __builtin_amdgcn_readlane(src, l);
      if (PPS == 2) id[k] = sub ? __builtin_amdgcn_readlane(src, l + 1) : id[k];
      zv[k] = zb[(size_t)max(id[k], 0) * c];
      if (CX) {
        cv[k] = cb[(size_t)min(cj, m - 1) * c];
#pragma unroll
        for (int q = 0; q < PPS; ++q) {
          const bool wrap = cr + 1 == u;
          cr = wrap ? 0 : cr + 1;
          cj += wrap ? 1 : 0;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < GST_NB; ++k) {  // ascending positions: the chain every lane has always run
      float v = zv[k];
      if (CX) v -= cv[k];
      const bool ok = id[k] >= 0 && chok;
      const float t1 = s1 + v, t2 = s2 + v * v;
      s1 = ok ? t1 : s1;
      s2 = ok ? t2 : s2;
    }
  }
  if (PPS == 2) {
    s1 += __shfl_xor(s1, 32);
    s2 += __shfl_xor(s2, 32);
  }
  if (chok && sub == 0) {
    float *q = stats + (((size_t)b * nslots + slot) * c + ch) * 2;
    q[0] = s1;
    q[1] = s2;
  }
}

template <int CPL>
static void group_stats_launch(int b, int c, int n, int m, int u, int nslots, const float *zt, const float *cxt, const int *idx,
                               float *stats_part, hipStream_t s) {
  const dim3 grid(cdiv(nslots, 4), cdiv(c, CPL), b);
  if (cxt) hipLaunchKernelGGL((group_stats_kernel<CPL, true>), grid, dim3(256), 0, s, c, n, m, u, nslots, zt, cxt, idx, stats_part);
  else hipLaunchKernelGGL((group_stats_kernel<CPL, false>), grid, dim3(256), 0, s, c, n, m, u, nslots, zt, cxt, idx, stats_part);
}

extern "C" int p2pb_group_sub_stats_slots(int m, int u) { return (int)(((long)m * u + GST_PW - 1) / GST_PW); }
// zt f32[b,n,c], cxt f32[b,m,c] | NULL (point-major), idx i32[b,m,u] -> stats_part f32[b, p2pb_group_sub_stats_slots(m,u), c, 2]
extern "C" int p2pb_group_sub_stats(int b, int c, int n, int m, int u, const float *zt, const float *cxt, const int *idx,
                                    float *stats_part, void *stream) {
  if (b <= 0 || c <= 0 || n <= 0 || m <= 0 || u <= 0 || !zt || !idx || !stats_part || (long)m * u > 0x7fffffffL) return P2PB_EINVAL;
  const int nslots = p2pb_group_sub_stats_slots(m, u);
  hipStream_t s = (hipStream_t)stream;
  if (c <= 32) group_stats_launch<32>(b, c, n, m, u, nslots, zt, cxt, idx, stats_part, s);
  else group_stats_launch<64>(b, c, n, m, u, nslots, zt, cxt, idx, stats_part, s);
  return p2pb_launch_status();
}

extern "C" size_t p2pb_group_sub_stats_floats(int b, int c, int m, int u) {
  return (size_t)b * (((size_t)m * u + 63) / 64 * 2) * c * 2;
}

// ws: f32[b*(n+m)*c] scratch for the point-major copies
extern "C" int p2pb_group_sub(int b, int c, int n, int m, int u, const float *z, const float *cx, const int *idx,
                              float *out, float *stats_part, float *ws, void *stream) {
  if (b <= 0 || c <= 0 || n <= 0 || m <= 0 || u <= 0 || !stats_part) return P2PB_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const float *zt = z, *cxt = cx;  // ws == NULL: z f32[b,n,c] and cx f32[b,m,c] are point-major already
  if (ws) {
    float *zw = ws, *cw = ws + (size_t)b * n * c;
    hipLaunchKernelGGL(nb_transpose_kernel, dim3(cdiv(n, 32), cdiv(c, 32), b), dim3(256), 0, s, c, n, z, zw);
    if (cx) hipLaunchKernelGGL(nb_transpose_kernel, dim3(cdiv(m, 32), cdiv(c, 32), b), dim3(256), 0, s, c, m, cx, cw);
    zt = zw;
    cxt = cx ? cw : nullptr;
  }
  const int nblk = (int)(((long)m * u + 63) / 64);
  hipLaunchKernelGGL(group_sub_kernel, dim3(nblk, cdiv(c, c <= 32 ? 32 : 64), b), dim3(256), 0, s, c, n, m, u, nblk * 2,
                     zt, cxt, idx, out, stats_part);
  return p2pb_launch_status();
}

// ------------------------------------------------------------------------------------------------
// gather: out[b,c,j] = feat[b,c,idx[b,j]]
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gather_kernel(int c, int n, int m, const float *__restrict__ feat,
                                                     const int *__restrict__ idx, float *__restrict__ out) {
  const int b = blockIdx.z, l = blockIdx.y;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  out[((size_t)b * c + l) * m + j] = feat[((size_t)b * c + l) * n + idx[(size_t)b * m + j]];
}

extern "C" int p2pb_gather_features_forward(int b, int c, int n, int m, const float *feat, const int *idx, float *out,
                                            void *stream) {
  if (b <= 0 || c <= 0 || n <= 0 || m <= 0) return P2PB_EINVAL;
  hipLaunchKernelGGL(gather_kernel, dim3(cdiv(m, 256), c, b), dim3(256), 0, (hipStream_t)stream, c, n, m, feat, idx,
                     out);
  return p2pb_launch_status();
}

// Feature propagation with the first 1x1 convolution applied before the interpolation (inference): interpolation and
// convolution are both linear, so W [interp(g) ; skip] + bias = interp(W_g g) + (W_s skip + bias): the GEMM on the
// interpolated channels runs on the m coarse points instead of the n fine ones and the concatenated tensor of
// models/pvcnn.py:457-461 is never built.  out[b,c,j] = sum_k w_k * cz[b,c,idx_k] + add[b,c,j] (+ bias[c]), plus the
// {sum, sum of squares} partials of the GroupNorm that follows (one slot per half-wave, as group_sub_kernel).
__global__ __launch_bounds__(256) void three_interp_add_kernel(int c, int m, int n, int nslots,
                                                               const float *__restrict__ czt,
                                                               const int *__restrict__ indices,
                                                               const float *__restrict__ weights,
                                                               const float *__restrict__ add,
                                                               const float *__restrict__ bias, float *__restrict__ out,
                                                               float *__restrict__ stats) {
  __shared__ float tile[64][65];  // [channel][position]
  __shared__ int sid[64][3];
  __shared__ float sw[64][3];
  const int b = blockIdx.z, p0 = blockIdx.x * 64, t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  if (t < 64) {
    const int j = min(p0 + t, n - 1);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      sid[t][k] = indices[((size_t)b * 3 + k) * n + j];
      sw[t][k] = weights[((size_t)b * 3 + k) * n + j];
    }
  }
  __syncthreads();
  {
    const int c0 = blockIdx.y * 64;  // one 64-channel chunk per workgroup
    const int ch = c0 + lane;
    if (ch < c) {
      const float *f = czt + (size_t)b * m * c + ch;  // point-major coarse features: one contiguous row per neighbour
      // (eight positions' rows per batch: left to the unroller, two positions' six loads were waited for together, eight round
      // trips for the wave's sixteen positions)
      for (int pl0 = wave * 16; pl0 < wave * 16 + 16; pl0 += 8) {
        float g[8][3];
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
          for (int q = 0; q < 3; ++q) g[k][q] = f[(size_t)sid[pl0 + k][q] * c];
#pragma unroll
        for (int k = 0; k < 8; ++k)
          tile[lane][pl0 + k] = __fmaf_rn(g[k][2], sw[pl0 + k][2], __fmaf_rn(g[k][1], sw[pl0 + k][1], g[k][0] * sw[pl0 + k][0]));
      }
    }
    const int pt = lane;
    const bool pok = p0 + pt < n;
    // The `add` and `bias` values of the thread's 16 rows are loaded here, all at once and from clamped addresses (rows >= c,
    // positions >= n), while the waves meet at the barrier: loaded inside the row loop's branches each was waited for
    // (vmcnt(0)) before the next was issued, 32 L2 round trips in a row (profiles/r07_gather_wait_audit.txt).
    float av[16], bv[16];
    if (add) {
#pragma unroll
      for (int k = 0; k < 16; ++k) av[k] = add[((size_t)b * c + min(c0 + wave + 4 * k, c - 1)) * n + min(p0 + pt, n - 1)];
    }
    if (bias) {
#pragma unroll
      for (int k = 0; k < 16; ++k) bv[k] = bias[min(c0 + wave + 4 * k, c - 1)];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int cr = wave + 4 * k;  // (see group_sub_kernel)
      if (c0 + cr < c) {
        float v = tile[cr][pt];
        if (add) v += av[k];
        if (bias) v += bv[k];
        v = pok ? v : 0.0f;
        if (pok) out[((size_t)b * c + c0 + cr) * n + p0 + pt] = v;
        const float s1 = halfwave_sum_to_last(v), s2 = halfwave_sum_to_last(v * v);
        if ((lane & 31) == 31) {
          float *p = stats + (((size_t)b * nslots + blockIdx.x * 2 + (lane >> 5)) * c + c0 + cr) * 2;
          p[0] = s1;
          p[1] = s2;
        }
      }
    }
    __syncthreads();
  }
}

// stats_part: f32[p2pb_group_sub_stats_floats(b, c, n, 1)]; ws: f32[b*m*c] scratch (point-major copy of cz)
extern "C" int p2pb_three_interpolate_add(int b, int c, int m, int n, const float *cz, const int *idx, const float *w,
                                          const float *add, const float *bias, float *out, float *stats_part,
                                          float *ws, void *stream) {
  if (b <= 0 || c <= 0 || n <= 0 || m <= 0 || !stats_part) return P2PB_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const float *czt = cz;  // ws == NULL: cz f32[b,m,c] is point-major already
  if (ws) {
    hipLaunchKernelGGL(nb_transpose_kernel, dim3(cdiv(m, 32), cdiv(c, 32), b), dim3(256), 0, s, c, m, cz, ws);
    czt = ws;
  }
  const int nblk = (n + 63) / 64;
  hipLaunchKernelGGL(three_interp_add_kernel, dim3(nblk, cdiv(c, 64), b), dim3(256), 0, s, c, m, n, nblk * 2, czt, idx, w,
                     add, bias, out, stats_part);
  return p2pb_launch_status();
}
