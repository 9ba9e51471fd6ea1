// pointwise_act.hip -- the small kernels around the 1x1-convolution GEMMs of the other pointwise*.hip:
//   minmax_act      max(act(scale*min + shift), act(scale*max + shift)) from the {min, max} a GEMM's pooling epilogue left
//   linear_rows     nn.Linear on a handful of rows without BLAS
//   affine_act      y = swish(x*scale[b,c] + shift[b,c]) (+ residual)           (last layer of a chain)
//   affine_act_max  y[b,c,m] = max_u swish(x[b,c,m,u]*scale + shift)            (set-abstraction pooling)
#include "pw_common.h"

// y = max(act(scale*min + shift), act(scale*max + shift)):
//   nslots == 0: minmax f32[b, c, m, 2] -> y f32[b, c, m]      (set-abstraction neighbour max)
//   nslots  > 0: minmax f32[b, nslots, c, 2] -> y f32[b, c]    (global max-pool; partials reduced first)
__global__ __launch_bounds__(256) void minmax_act_kernel(int c, int m, int nslots, const float *__restrict__ mm,
                                                         const float *__restrict__ scale,
                                                         const float *__restrict__ shift, int swish,
                                                         float *__restrict__ y, size_t total) {
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    float mn, mx;
    size_t bc;
    if (nslots == 0) {
      bc = e / m;
      const float2 v = *(const float2 *)(mm + e * 2);
      mn = v.x;
      mx = v.y;
    } else {
      bc = e;
      const size_t b = e / c, ch = e % c;
      mn = INFINITY;
      mx = -INFINITY;
      for (int sl = 0; sl < nslots; ++sl) {
        const float2 v = *(const float2 *)(mm + ((b * nslots + sl) * c + ch) * 2);
        mn = fminf(mn, v.x);
        mx = fmaxf(mx, v.y);
      }
    }
    const float sc = scale[bc], sh = shift[bc];
    float lo = mn * sc + sh, hi = mx * sc + sh;
    if (swish) {
      lo = swishf(lo);
      hi = swishf(hi);
    }
    y[e] = fmaxf(lo, hi);
  }
}

// global pool (nslots > 0) with the slot loop spread over 8 waves: 32 channels x 8 slot classes per workgroup, min / max
// combined through LDS (exact, order-free) -- one thread per (sample, channel) walked 128+ slots serially: 69 us for the
// 1024-channel embedding of the bench
// part != NULL (round 5): the GroupNorm that precedes the activation is folded here too -- the workgroup finishes the groups its
// 32 channels belong to from the producing GEMM's statistics partials (gn_finish_group: gn_affine_kernel's bits), WRITES
// scale / shift (fin.scale / fin.shift: the next GEMM applies them to the same tensor on load) and pools with them; the
// gn_affine launch between the GEMM and this kernel is gone.
__global__ __launch_bounds__(256) void minmax_act_pool_kernel(int c, int nslots, const float *__restrict__ mm,
                                                              const float *__restrict__ scale,
                                                              const float *__restrict__ shift, int swish,
                                                              float *__restrict__ y, const float *__restrict__ part, int nslots_st,
                                                              GnFinish fin) {
  __shared__ float smn[8][32], smx[8][32];
  __shared__ double gl[4 * 256];
  extern __shared__ float mmp_tab[];  // folded form: scale[c] | shift[c] of this sample
  const int b = blockIdx.y, ch = blockIdx.x * 32 + (threadIdx.x & 31), part_i = threadIdx.x >> 5;
  float mn = INFINITY, mx = -INFINITY;
  if (ch < c)
    for (int sl = part_i; sl < nslots; sl += 8) {
      const float2 v = *(const float2 *)(mm + (((size_t)b * nslots + sl) * c + ch) * 2);
      mn = fminf(mn, v.x);
      mx = fmaxf(mx, v.y);
    }
  smn[part_i][threadIdx.x & 31] = mn;
  smx[part_i][threadIdx.x & 31] = mx;
  if (part != nullptr) {
    const int cg = c / fin.groups, c0 = blockIdx.x * 32, c1 = min(c0 + 32, c) - 1;
    for (int g = c0 / cg; g <= c1 / cg; ++g)
      gn_finish_group_v(c, nslots_st, part, fin, b, g, gl, (int)threadIdx.x, true, nullptr, mmp_tab, mmp_tab + c);
  }
  __syncthreads();
  if (part_i != 0 || ch >= c) return;
#pragma unroll
  for (int p = 1; p < 8; ++p) {
    mn = fminf(mn, smn[p][threadIdx.x]);
    mx = fmaxf(mx, smx[p][threadIdx.x]);
  }
  const float sc = part ? mmp_tab[ch] : scale[(size_t)b * c + ch], sh = part ? mmp_tab[c + ch] : shift[(size_t)b * c + ch];
  float lo = mn * sc + sh, hi = mx * sc + sh;
  if (swish) {
    lo = swishf(lo);
    hi = swishf(hi);
  }
  y[(size_t)b * c + ch] = fmaxf(lo, hi);
}

extern "C" int p2pb_minmax_act(int b, int c, int m, int nslots, const float *minmax, const float *scale,
                               const float *shift, int swish, float *y, void *stream) {
  if (b <= 0 || c <= 0 || m <= 0 || nslots < 0) return P2PB_EINVAL;
  if (nslots >= 16) {
    hipLaunchKernelGGL(minmax_act_pool_kernel, dim3((c + 31) / 32, b), dim3(256), 0, (hipStream_t)stream, c, nslots, minmax,
                       scale, shift, swish, y, (const float *)nullptr, 0, GnFinish());
    return p2pb_launch_status();
  }
  const size_t total = nslots == 0 ? (size_t)b * c * m : (size_t)b * c;
  const unsigned blocks = (unsigned)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
  hipLaunchKernelGGL(minmax_act_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, c, m, nslots, minmax, scale,
                     shift, swish, y, total);
  return p2pb_launch_status();
}
// the global max-pool (minmax f32[b, nslots, c, 2] -> y f32[b, c]) with the GroupNorm in front of the activation folded in: part
// f32[b, nslots_st, c, 2] = the producing GEMM's statistics partials; scale / shift f32[b, c] are OUTPUTS (p2pb_gn_affine_params'
// values, same bits). Replaces MyGroupNorm + Swish + the max-pool of models/pvcnn.py:905-932 behind a Pnet2Stage GEMM.
extern "C" int p2pb_minmax_act_pool_gn(int b, int c, int nslots, const float *minmax, const float *part, int nslots_st,
                                       double count_per_channel, int groups, const float *gamma, const float *beta,
                                       const float *style, int style_stride, float eps, int swish, float *scale, float *shift,
                                       float *y, void *stream) {
  if (b <= 0 || c <= 0 || nslots <= 0 || !minmax || !part || nslots_st <= 0 || !scale || !shift || !y || groups <= 0 ||
      c % groups != 0 || c / groups > 256 || (style && style_stride < 2 * c) || (size_t)c * 8 > 32 * 1024)
    return P2PB_EINVAL;
  GnFinish f = {};
  f.gamma = gamma, f.beta = beta, f.style = style, f.scale = scale, f.shift = shift, f.style_stride = style_stride, f.groups = groups;
  f.eps = eps, f.count_per_channel = count_per_channel;
  hipLaunchKernelGGL(minmax_act_pool_kernel, dim3((c + 31) / 32, b), dim3(256), (size_t)c * 8, (hipStream_t)stream, c, nslots, minmax,
                     (const float *)nullptr, (const float *)nullptr, swish, y, part, nslots_st, f);
  return p2pb_launch_status();
}

// ------------------------------------------------------------------------------------------------
// nn.Linear on a handful of rows: out[b, co] = bias[co] + sum_ci w[co, ci] x[b, ci]   (b <= a few dozen)
// The per-evaluation Linears of the network -- every AdaGN's style Linear on the global embedding (concatenated: 1024 ->
// 13184 for PVDS, models/modules.py:337-345), the time embedding's two (models/unet_pvc.py:108-112), the global embedding's
// per-sample bias (models/pvcnn.py:926) -- are weight-streaming GEMVs (54 MB of weights for the styles). They used to go
// through torch's BLAS, whose per-stream WORKSPACE a captured graph bakes in: two sampler chains replaying their graphs side
// by side then shared one workspace and corrupted each other's GEMMs (round 4, tests/test_full_size_parity_gpu.py::
// test_c2_bench_dispatch_two_chains_b32 -- the corruption found there turned out to be the devoxelisation's, devoxelize.hip; the
// workspace sharing is real all the same).
// This kernel needs no scratch: the exact-fp32 matrix instruction (v_mfma_f32_32x32x2_f32: fp32 products, fp32 accumulate) with
// M = 32 weight rows, N = the batch rows (<= 16 per chunk, x staged in LDS with a 4-float row pad: conflict-free 16-byte reads),
// K split over the four waves of a workgroup and summed through LDS in a fixed order (deterministic). A lane's weight operand is
// one 16-byte load W[row][k0 + 4 h .. + 3] feeding four MFMAs (k pairs (4 h + i) of both half-waves), so the weights stream
// through once, 32 contiguous bytes per row and step, every 128-byte line consumed by the same wave within four steps.
#define LR_BC 16
__global__ __launch_bounds__(256) void linear_rows_kernel(int B, int cin, int cout, const float *__restrict__ x, long xs,
                                                          const float *__restrict__ w, long ws,
                                                          const float *__restrict__ bias, float *__restrict__ out, long os,
                                                          int bc) {
  extern __shared__ float lr_x[];  // [bc][cin + 4]; reused for the cross-wave sum [4][32][17]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int row0 = blockIdx.x * 32;
  const int xp = cin + 4;
  const int wrow = min(row0 + l31, cout - 1);  // (clamped rows multiply garbage that is never stored)
  // this wave's K range: whole 8-steps, dealt round-robin to the four waves
  const int nk8 = (cin + 7) / 8;
  for (int b0 = 0; b0 < B; b0 += bc) {
    const int nb = min(bc, B - b0);
    __syncthreads();
    for (int e = tid * 4; e < nb * cin; e += 1024) {
      const int bb = e / cin, c = e - bb * cin;
      *(f32x4 *)(lr_x + bb * xp + c) = *(const f32x4 *)(x + (size_t)(b0 + bb) * xs + c);
    }
    __syncthreads();
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const float *wp_ = w + (size_t)wrow * ws + 4 * h;
    const float *xq = lr_x + min(l31, nb - 1) * xp + 4 * h;
    // weights: EIGHT 16-byte loads per lane in flight (round 5: with four the 54 MB of style weights streamed at 0.7-0.9 TB/s --
    // 8 waves x 4 KB per CU in flight against an HBM latency of microseconds; the multiply is 16 us of matrix time at most)
    const int nit = (nk8 - wave + 3) / 4;
    for (int it0 = 0; it0 < nit; it0 += 8) {
      f32x4 wv[8], xv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int k = (wave + 4 * (it0 + u)) * 8;
        wv[u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (it0 + u < nit && k + 4 * h < cin) wv[u] = *(const f32x4 *)(wp_ + k);  // (cin % 4 == 0: a quad is inside or outside)
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int k = (wave + 4 * (it0 + u)) * 8;
        xv[u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (it0 + u < nit && k + 4 * h < cin) xv[u] = *(const f32x4 *)(xq + k);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[u][i], xv[u][i], acc, 0, 0, 0);
    }
    __syncthreads();  // everyone is done with x
    float *red = lr_x;  // [4 waves][32 rows][17]
    if (l31 < nb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) red[(wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * 17 + l31] = acc[r];
    }
    __syncthreads();
    for (int e = tid; e < 32 * nb; e += 256) {
      const int r = e / nb, bb = e - r * nb;
      if (row0 + r < cout) {
        const float v = (red[(0 * 32 + r) * 17 + bb] + red[(1 * 32 + r) * 17 + bb]) + (red[(2 * 32 + r) * 17 + bb] + red[(3 * 32 + r) * 17 + bb]);
        out[(size_t)(b0 + bb) * os + row0 + r] = v + (bias ? bias[row0 + r] : 0.0f);
      }
    }
  }
}

// x f32[b, cin] (row pitch x_stride floats), w f32[cout, cin] (row pitch w_stride: a column slice of a wider matrix is fine),
// bias f32[cout] or NULL -> out f32[b, cout] (row pitch out_stride). cin % 4 == 0, 16-byte aligned rows.
extern "C" int p2pb_linear_rows(int b, int cin, int cout, const float *x, long x_stride, const float *w, long w_stride,
                                const float *bias, float *out, long out_stride, void *stream) {
  if (b <= 0 || cin <= 0 || cout <= 0 || !x || !w || !out || (cin & 3) || (x_stride & 3) || (w_stride & 3) ||
      (((uintptr_t)x | (uintptr_t)w) & 15) || x_stride < cin || w_stride < cin || out_stride < cout)
    return P2PB_EINVAL;
  int bc = (int)(65536 / ((long)(cin + 4) * 4));  // batch rows per LDS chunk (64 KB: two workgroups per CU)
  if (bc < 1) return P2PB_EINVAL;           // (cin > 16384)
  if (bc > LR_BC) bc = LR_BC;
  if (bc > b) bc = b;
  size_t lr_lds = (size_t)bc * (cin + 4) * 4;
  if (lr_lds < 4 * 32 * 17 * 4) lr_lds = 4 * 32 * 17 * 4;  // (the cross-wave sum's table)
  hipLaunchKernelGGL(linear_rows_kernel, dim3(cdiv(cout, 32)), dim3(256), lr_lds, (hipStream_t)stream, b, cin,
                     cout, x, x_stride, w, w_stride, bias, out, out_stride, bc);
  return p2pb_launch_status();
}

// ------------------------------------------------------------------------------------------------
// y = act(x*scale[b,c] + shift[b,c]) (+ residual)   over [b, c, P]
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void affine_act_kernel(int c, int P, const float *__restrict__ x,
                                                         const float *__restrict__ scale,
                                                         const float *__restrict__ shift, int swish,
                                                         const float *__restrict__ residual, float *__restrict__ y) {
  const int bc = blockIdx.y;  // b*c + ch
  const float sc = scale[bc], sh = shift[bc];
  const float *xr = x + (size_t)bc * P;
  const float *rr = residual ? residual + (size_t)bc * P : nullptr;
  float *yr = y + (size_t)bc * P;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < P; p += gridDim.x * 256) {
    float v = xr[p] * sc + sh;
    if (swish) v = swishf(v);
    if (rr) v = rr[p] + v;
    yr[p] = v;
  }
}

// 16-byte form (rows of whole, aligned quads): a pure streaming pass, HBM-bound
__global__ __launch_bounds__(256) void affine_act4_kernel(int c, int P4, const f32x4 *__restrict__ x,
                                                          const float *__restrict__ scale,
                                                          const float *__restrict__ shift, int swish,
                                                          const f32x4 *__restrict__ residual, f32x4 *__restrict__ y) {
  const int bc = blockIdx.y;
  const float sc = scale[bc], sh = shift[bc];
  const f32x4 *xr = x + (size_t)bc * P4;
  const f32x4 *rr = residual ? residual + (size_t)bc * P4 : nullptr;
  f32x4 *yr = y + (size_t)bc * P4;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < P4; p += gridDim.x * 256) {
    f32x4 v = xr[p];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float t = v[i] * sc + sh;
      if (swish) t = swishf(t);
      v[i] = t;
    }
    if (rr) v += rr[p];
    yr[p] = v;
  }
}

extern "C" int p2pb_affine_act(int b, int c, int npos, const float *x, const float *scale, const float *shift,
                               int swish, const float *residual, float *y, void *stream) {
  if (b <= 0 || c <= 0 || npos <= 0) return P2PB_EINVAL;
  if (npos % 4 == 0 && (((uintptr_t)x | (uintptr_t)y | (uintptr_t)residual) & 15) == 0) {
    const int p4 = npos / 4;
    const unsigned gx = (unsigned)((p4 + 255) / 256 > 64 ? 64 : (p4 + 255) / 256);
    hipLaunchKernelGGL(affine_act4_kernel, dim3(gx, b * c), dim3(256), 0, (hipStream_t)stream, c, p4, (const f32x4 *)x,
                       scale, shift, swish, (const f32x4 *)residual, (f32x4 *)y);
    return p2pb_launch_status();
  }
  const unsigned gx = (unsigned)((npos + 255) / 256 > 64 ? 64 : (npos + 255) / 256);
  hipLaunchKernelGGL(affine_act_kernel, dim3(gx, b * c), dim3(256), 0, (hipStream_t)stream, c, npos, x, scale, shift,
                     swish, residual, y);
  return p2pb_launch_status();
}

// ------------------------------------------------------------------------------------------------
// y[b,c,m] = max_{u < U} act(x[b,c,m,u]*scale + shift), U a power of two <= 64 (32 in every config):
// lanes read the [m,u] plane contiguously, the max runs over aligned groups of U lanes.
// U == 0 selects "max over the whole row" (Pnet2Stage's global max-pool): y[b,c] = max_p act(...).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void affine_act_max_kernel(int M, int U, const float *__restrict__ x,
                                                             const float *__restrict__ scale,
                                                             const float *__restrict__ shift, int swish,
                                                             float *__restrict__ y) {
  const int bc = blockIdx.y;
  const float sc = scale[bc], sh = shift[bc];
  const float *xr = x + (size_t)bc * M * U;
  float *yr = y + (size_t)bc * M;
  const int total = M * U;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {  // total % 64 == 0 by construction
    float v = xr[e] * sc + sh;
    if (swish) v = swishf(v);
    for (int off = U >> 1; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    if ((e & (U - 1)) == 0) yr[e / U] = v;
  }
}

__global__ __launch_bounds__(256) void affine_act_rowmax_kernel(int P, const float *__restrict__ x,
                                                                const float *__restrict__ scale,
                                                                const float *__restrict__ shift, int swish,
                                                                float *__restrict__ y) {
  __shared__ float red[256];
  const int bc = blockIdx.x;
  const float sc = scale[bc], sh = shift[bc];
  const float *xr = x + (size_t)bc * P;
  float mx = -INFINITY;
  for (int p = threadIdx.x; p < P; p += 256) {
    float v = xr[p] * sc + sh;
    if (swish) v = swishf(v);
    mx = fmaxf(mx, v);
  }
  red[threadIdx.x] = mx;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x == 0) y[bc] = red[0];
}

extern "C" int p2pb_affine_act_max(int b, int c, int m, int u, const float *x, const float *scale, const float *shift,
                                   int swish, float *y, void *stream) {
  if (b <= 0 || c <= 0 || m <= 0 || u < 0) return P2PB_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (u == 0) {
    hipLaunchKernelGGL(affine_act_rowmax_kernel, dim3(b * c), dim3(256), 0, s, m, x, scale, shift, swish, y);
    return p2pb_launch_status();
  }
  if ((u & (u - 1)) != 0 || u > 64 || ((long)m * u) % 64 != 0) return P2PB_EINVAL;
  const long total = (long)m * u;
  const unsigned gx = (unsigned)((total + 255) / 256 > 64 ? 64 : (total + 255) / 256);
  hipLaunchKernelGGL(affine_act_max_kernel, dim3(gx, b * c), dim3(256), 0, s, m, u, x, scale, shift, swish, y);
  return p2pb_launch_status();
}
