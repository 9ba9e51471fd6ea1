// conv3d_farfield.hip -- the constants of the "sparsity by linearity" form of a PVConv's second convolution (conv3d_common.h):
// a[b, ci], the value of its operand where the first convolution saw only zeros, and K[b, class, co], the convolution of that
// constant field, per boundary class. Summed from the exact-fp32 weight pack (conv3d_fp32.hip).
#include "conv3d_common.h"

// far-field constants of a folded operand transform: a[b,c] = xf(base[c]) with the SAME device function the
// staging code uses (bit-identical), i.e. the value of swish(affine(conv0 output)) where conv0 saw only zeros
static __global__ void far_value_kernel(int c, const float *__restrict__ base, const float *__restrict__ scale,
                                 const float *__restrict__ shift, int swish, float *__restrict__ a) {
  const int b = blockIdx.y, ch = blockIdx.x * 256 + threadIdx.x;
  if (ch >= c) return;
  a[(size_t)b * c + ch] = xf_apply(base[ch], scale[(size_t)b * c + ch], shift[(size_t)b * c + ch], swish);
}

// T[b, tap, co] = sum_ci W[tap][ci][co] * a[b,ci]  (one thread per output channel, weights read coalesced)
static __global__ __launch_bounds__(256) void tap_sum_kernel(int cin, int cout, int nchunk, int cout_pad,
                                                      const float *__restrict__ wt, const float *__restrict__ a,
                                                      float *__restrict__ tsum) {
  const int tap = blockIdx.y, b = blockIdx.z;
  const int co = blockIdx.x * 256 + threadIdx.x;
  if (co >= cout) return;
  float acc = 0.0f;
  for (int ci = 0; ci < cin; ++ci) {
    const size_t idx = ((((size_t)tap * nchunk + (ci >> 3)) * 2 + (ci & 1)) * cout_pad + co) * 4 + ((ci & 7) >> 1);
    acc = __fmaf_rn(wt[idx], a[(size_t)b * cin + ci], acc);
  }
  tsum[((size_t)b * 27 + tap) * cout + co] = acc;
}

// K[b, class, co] = bias[co] + sum over the taps that stay inside the grid for that boundary class of T[b,tap,co]
// (the convolution of the constant field a with zero padding)
static __global__ __launch_bounds__(256) void class_bias_kernel(int cout, const float *__restrict__ tsum,
                                                         const float *__restrict__ bias, float *__restrict__ k_out) {
  const int cls = blockIdx.y, b = blockIdx.z;
  const int co = blockIdx.x * 256 + threadIdx.x;
  if (co >= cout) return;
  const int cd = cls / 9, ch = (cls / 3) % 3, cw = cls % 3;
  float acc = 0.0f;
  for (int tap = 0; tap < 27; ++tap) {
    const int kd = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
    // class 0 = low face: the tap reading index -1 is outside; class 2 = high face: the tap reading R is outside
    if ((cd == 0 && kd == 0) || (cd == 2 && kd == 2) || (ch == 0 && kh == 0) || (ch == 2 && kh == 2) ||
        (cw == 0 && kw == 0) || (cw == 2 && kw == 2))
      continue;
    acc += tsum[((size_t)b * 27 + tap) * cout + co];
  }
  k_out[((size_t)b * 27 + cls) * cout + co] = acc + bias[co];
}

// The three steps above in ONE launch (round 4: 15 -> 5 launches per network evaluation): workgroup (FF_CO output channels, sample):
// every thread evaluates a[ci] into LDS (the first channel block also stores it), thread (c, tap) sums ITS tap for channel c over the
// input channels, then the 27 class sums from the LDS table. Same operations in the same order per output as far_value / tap_sum /
// class_bias: bit-identical.
// Round 5 (profiles/r05_overlap.txt: 52-79 us per launch on 32-64 workgroups, 290 us of every chain-evaluation): 32 channels x 27
// taps per workgroup instead of 64 channels x 16 tap groups of two (twice the workgroups, half the serial length per thread), and
// the weights as the 16-byte groups the pack holds -- [tap][ci / 8][ci & 1][co][(ci & 7) >> 1]: one float4 = input channels
// h, h + 2, h + 4, h + 6 of a chunk -- so a chunk of 8 input channels is two coalesced 16-byte loads (512 contiguous bytes per 32
// lanes) instead of eight 4-byte loads at a 16-byte stride; the fused multiply-adds stay in ascending input-channel order.
// part != NULL: the GroupNorm(+AdaGN) between the two convolutions is folded HERE as well -- `scale` / `shift` are then OUTPUTS
// (fin.scale / fin.shift, f32[b, cin], written by the first channel block for the kernels that stage the operand) and the
// gn_affine launch between the first convolution and this kernel is gone (round 5; gn_finish_sample: the same bits).
constexpr int FF_CO = 32;
static __global__ __launch_bounds__(1024) void far_field_kernel(int cin, int cout, int nchunk, int cout_pad,
                                                        const float *__restrict__ base, const float *__restrict__ scale,
                                                        const float *__restrict__ shift, int swish,
                                                        const float *__restrict__ wt, const float *__restrict__ bias,
                                                        float *__restrict__ a_out, float *__restrict__ k_out,
                                                        const float *__restrict__ part, int nslots, GnFinish fin) {
  extern __shared__ double ff_sm_d[];  // [scale[cin] | shift[cin]] (folded form) | union { 4 x 1024 doubles, a[cin] | T[27][FF_CO] }
  float *ff_sm = (float *)ff_sm_d;
  const int b = blockIdx.y, t = threadIdx.x, c = t & (FF_CO - 1), tap = t / FF_CO;
  const int co = blockIdx.x * FF_CO + c;
  float *a, *T;
  if (part != nullptr) {
    float *tsc = ff_sm, *tsh = ff_sm + cin;
    double *gl = ff_sm_d + (2 * cin + 1) / 2;
    GnFinish f = fin;
    if (blockIdx.x != 0) f.scale = f.shift = nullptr;  // (every channel block computes the values, one writes them)
    gn_finish_sample<4>(cin, nslots, part, f, b, gl, tsc, tsh);
    a = (float *)gl, T = a + nchunk * 8;
    for (int ch = t; ch < cin; ch += 1024) {
      const float v = xf_apply(base[ch], tsc[ch], tsh[ch], swish);
      a[ch] = v;
      if (blockIdx.x == 0) a_out[(size_t)b * cin + ch] = v;
    }
  } else {
    a = ff_sm, T = ff_sm + nchunk * 8;
    for (int ch = t; ch < cin; ch += 1024) {
      const float v = xf_apply(base[ch], scale[(size_t)b * cin + ch], shift[(size_t)b * cin + ch], swish);
      a[ch] = v;
      if (blockIdx.x == 0) a_out[(size_t)b * cin + ch] = v;
    }
  }
  __syncthreads();
  if (tap < 27) {
    float acc = 0.0f;
    if (co < cout) {
      const float4 *w4 = (const float4 *)wt + ((size_t)tap * nchunk * 2) * cout_pad + co;
      // Whole chunks four at a time, their eight weight loads issued together: with the ragged-chunk tests inside the loop every
      // chunk's two loads were waited for (vmcnt(0)) before the next chunk's were issued, one L2 round trip per eight input
      // channels (profiles/r07_gather_wait_audit.txt). Same fused multiply-adds in the same ascending input-channel order.
      int k8 = 0;
      for (; k8 + 4 <= cin / 8; k8 += 4) {
        float4 h[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) h[q] = w4[(size_t)(2 * k8 + q) * cout_pad];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 h0 = h[2 * q], h1 = h[2 * q + 1];
          const float *av = a + (k8 + q) * 8;
          acc = __fmaf_rn(h0.x, av[0], acc);
          acc = __fmaf_rn(h1.x, av[1], acc);
          acc = __fmaf_rn(h0.y, av[2], acc);
          acc = __fmaf_rn(h1.y, av[3], acc);
          acc = __fmaf_rn(h0.z, av[4], acc);
          acc = __fmaf_rn(h1.z, av[5], acc);
          acc = __fmaf_rn(h0.w, av[6], acc);
          acc = __fmaf_rn(h1.w, av[7], acc);
        }
      }
      for (; k8 < nchunk; ++k8) {
        const float4 h0 = w4[(size_t)(2 * k8) * cout_pad], h1 = w4[(size_t)(2 * k8 + 1) * cout_pad];
        const float *av = a + k8 * 8;
        const int left = cin - k8 * 8;  // (a ragged last chunk: the channels that exist, in order)
        if (left > 0) acc = __fmaf_rn(h0.x, av[0], acc);
        if (left > 1) acc = __fmaf_rn(h1.x, av[1], acc);
        if (left > 2) acc = __fmaf_rn(h0.y, av[2], acc);
        if (left > 3) acc = __fmaf_rn(h1.y, av[3], acc);
        if (left > 4) acc = __fmaf_rn(h0.z, av[4], acc);
        if (left > 5) acc = __fmaf_rn(h1.z, av[5], acc);
        if (left > 6) acc = __fmaf_rn(h0.w, av[6], acc);
        if (left > 7) acc = __fmaf_rn(h1.w, av[7], acc);
      }
    }
    T[tap * FF_CO + c] = acc;
  }
  __syncthreads();
  if (co >= cout || tap >= 27) return;
  {
    const int cls = tap;
    const int cd = cls / 9, ch = (cls / 3) % 3, cw = cls % 3;
    float acc = 0.0f;
    for (int tp = 0; tp < 27; ++tp) {
      const int kd = tp / 9, kh = (tp / 3) % 3, kw = tp % 3;
      if ((cd == 0 && kd == 0) || (cd == 2 && kd == 2) || (ch == 0 && kh == 0) || (ch == 2 && kh == 2) ||
          (cw == 0 && kw == 0) || (cw == 2 && kw == 2))
        continue;
      acc += T[tp * FF_CO + c];
    }
    k_out[((size_t)b * 27 + cls) * cout + co] = acc + bias[co];
  }
}

// a f32[b,cin] = far-field operand constants, k_out f32[b,27,cout] = per-boundary-class output constants,
// tap_ws f32[b,27,cout] scratch
static int far_field_launch(int b, int cin, int cout, const float *prev_bias, const float *in_scale, const float *in_shift,
                            int in_swish, const float *wt_packed, const float *bias, float *a, float *k_out, float *tap_ws,
                            const float *part, int nslots, const GnFinish &fin, hipStream_t s) {
  const int nchunk = (cin + CONV_CK - 1) / CONV_CK, cout_pad = (cout + 63) / 64 * 64;
  const size_t body = (size_t)(nchunk * 8 + 27 * FF_CO) * 4;
  const size_t lds = part ? (size_t)((2 * cin + 1) / 2) * 8 + (body > 32768 ? body : 32768) : body;
  if (lds <= 48 * 1024) {  // (tap_ws unused in this form)
    hipLaunchKernelGGL(far_field_kernel, dim3(cdiv(cout, FF_CO), b), dim3(1024), lds, s, cin, cout, nchunk, cout_pad, prev_bias,
                       in_scale, in_shift, in_swish, wt_packed, bias, a, k_out, part, nslots, fin);
    return p2pb_launch_status();
  }
  if (part) {  // (very wide layers: the norm as its own launch)
    const int e = p2pb_gn_affine_launch(b, cin, nslots, part, fin, s);
    if (e != 0) return e;
    in_scale = fin.scale, in_shift = fin.shift;
  }
  hipLaunchKernelGGL(far_value_kernel, dim3(cdiv(cin, 256), b), dim3(256), 0, s, cin, prev_bias, in_scale, in_shift,
                     in_swish, a);
  hipLaunchKernelGGL(tap_sum_kernel, dim3(cdiv(cout, 256), 27, b), dim3(256), 0, s, cin, cout, nchunk, cout_pad,
                     wt_packed, a, tap_ws);
  hipLaunchKernelGGL(class_bias_kernel, dim3(cdiv(cout, 256), 27, b), dim3(256), 0, s, cout, tap_ws, bias, k_out);
  return p2pb_launch_status();
}
extern "C" int p2pb_conv3d_k3_far_field(int b, int cin, int cout, const float *prev_bias, const float *in_scale,
                                        const float *in_shift, int in_swish, const float *wt_packed,
                                        const float *bias, float *a, float *k_out, float *tap_ws, void *stream) {
  if (b <= 0 || cin <= 0 || cout <= 0 || !in_scale || !in_shift) return P2PB_EINVAL;
  return far_field_launch(b, cin, cout, prev_bias, in_scale, in_shift, in_swish, wt_packed, bias, a, k_out, tap_ws, nullptr, 0,
                          GnFinish(), (hipStream_t)stream);
}
// the same with the GroupNorm(+AdaGN) of the operand folded in: part f32[b, nslots, cin, 2] = the first convolution's statistics
// partials; scale / shift f32[b, cin] are OUTPUTS (what p2pb_gn_affine_params would have written, same bits)
extern "C" int p2pb_conv3d_k3_far_field_gn(int b, int cin, int cout, const float *prev_bias, const float *part, int nslots,
                                           double count_per_channel, int groups, const float *gamma, const float *beta,
                                           const float *style, int style_stride, float eps, int in_swish,
                                           const float *wt_packed, const float *bias, float *scale, float *shift, float *a,
                                           float *k_out, float *tap_ws, void *stream) {
  if (b <= 0 || cin <= 0 || cout <= 0 || !part || nslots <= 0 || !scale || !shift || !gn_shape_ok(cin, groups, style, style_stride))
    return P2PB_EINVAL;
  GnFinish f = {};
  f.gamma = gamma, f.beta = beta, f.style = style, f.scale = scale, f.shift = shift, f.chmean = nullptr;
  f.count_per_channel = count_per_channel, f.style_stride = style_stride, f.groups = groups, f.eps = eps;
  return far_field_launch(b, cin, cout, prev_bias, nullptr, nullptr, in_swish, wt_packed, bias, a, k_out, tap_ws, part, nslots, f,
                          (hipStream_t)stream);
}
