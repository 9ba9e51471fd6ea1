// pointwise.hip -- entry points of the shared point MLPs (1x1 convolutions + AdaGN/GroupNorm + Swish (+ neighbour max)) of
// models/pvcnn.py:162-205 (SharedMLP), :388-424 (set abstraction), :446-467 (feature propagation), :905-932 (Pnet2Stage):
//   out[b,co,p] = bias[co] (+ bias_b[b,co]) + sum_ci W[co,ci] * xf(in[b,ci,p])
//   xf = identity, or the PREVIOUS layer's norm+activation folded to a per-(b,ci) affine + Swish applied while the operand is
//   staged; the epilogue emits the {sum, sumsq} partials the NEXT GroupNorm needs (and the {min, max} a max-pool is taken from).
//   So a chain conv-norm-act-conv-norm-act touches each activation tensor exactly twice (one write, one read) instead of ~8 times.
// Here: the two weight packs (each is read by kernels of more than one object), the validation of the arguments, the choice of
// the kernel form (recorded for p2pb_debug_pointwise_form) and the GroupNorm finisher behind the launch. The GEMM kernels are in
// pointwise_fp32.hip (exact-fp32 MFMA: P2PB_CONV_MATH=fp32, unaligned rows), pointwise_f16.hip and pointwise_split.hip (f16x3, the
// default: register-tiled for the narrow, HBM-bound layers -- 8 FLOP/B at C = 32..64 --, LDS-tiled for the matrix-bound ones).
#include "pw_common.h"
#include "absmax.h"

// w element (co, ci) at w[co * s_co + ci * s_ci]: (cin, 1) for a layer's own weight [cout][cin], (1, cout) for the adjoint
// (data-gradient) operator of a layer whose weight is [cin][cout] -- no transposed copy of the weight is ever made
__global__ void pw_pack_kernel(int cout, int cin, int cin_pad, int cout_pad, const float *__restrict__ w,
                               float *__restrict__ wp, long s_co, long s_ci) {
  const size_t total = (size_t)cin_pad * cout_pad;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int kk = (int)(e & 3);
    const int co = (int)((e >> 2) % cout_pad);
    const int kh = (int)((e / ((size_t)4 * cout_pad)) & 1);
    const int chunk = (int)(e / ((size_t)8 * cout_pad));
    const int ci = chunk * 8 + 2 * kk + kh;
    wp[e] = (co < cout && ci < cin) ? w[(size_t)co * s_co + (size_t)ci * s_ci] : 0.0f;
  }
}

extern "C" size_t p2pb_pointwise_packed_floats(int cout, int cin) {
  return (size_t)pw_cin_pad(cin) * pw_cout_pad(cout);
}

static int pw_pack(int cout, int cin, const float *w, float *wp, bool adjoint, void *stream) {
  if (cout <= 0 || cin <= 0) return P2PB_EINVAL;
  const size_t total = p2pb_pointwise_packed_floats(cout, cin);
  hipLaunchKernelGGL(pw_pack_kernel, dim3((unsigned)((total + 255) / 256 > 2048 ? 2048 : (total + 255) / 256)), dim3(256),
                     0, (hipStream_t)stream, cout, cin, pw_cin_pad(cin), pw_cout_pad(cout), w, wp, adjoint ? 1L : (long)cin,
                     adjoint ? (long)cout : 1L);
  return p2pb_launch_status();
}
extern "C" int p2pb_pointwise_pack_weights(int cout, int cin, const float *w, float *wp, void *stream) {
  return pw_pack(cout, cin, w, wp, false, stream);
}
extern "C" int p2pb_pointwise_pack_weights_adjoint(int cout, int cin, const float *w_forward, float *wp, void *stream) {
  return pw_pack(cout, cin, w_forward, wp, true, stream);
}

// split pack: wp[chunk32][cout block of 128][kstep 2][split 3][khalf 2][128 co][8 bf16],
// channel = chunk*32 + kstep*16 + khalf*8 + idx
// mode SPLIT_F16X3: planes 0, 1 hold the fp16 pair of w * S_w (plane 2 unused); trailer = {max|w| bits, 1 / (S_x S_w)}
__global__ void pw_pack_split_kernel(int cout, int cin, int nchunk, int ncoblk, const float *__restrict__ w,
                                     unsigned short *__restrict__ wp, int mode, float *__restrict__ trailer, long s_co, long s_ci,
                                     const unsigned *__restrict__ amax) {
  const size_t total = (size_t)nchunk * ncoblk * 2 * 2 * 128 * 8;  // (chunk, coblk, kstep, khalf, co, idx)
  const bool x2w = (mode & SPLIT_X2W_FLAG) != 0;  // (pricing experiment, common.h: a zero low plane)
  mode &= 0xff;
  const float wmax = amax ? __builtin_bit_cast(float, *amax) : trailer[0];  // (conv3d_pack_split_kernel: same convention)
  const float sw = mode == SPLIT_F16X3 ? f16_weight_scale(wmax) : 1.0f;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    trailer[1] = mode == SPLIT_F16X3 ? 1.0f / (SPLIT_F16_SX * sw) : 1.0f;
    if (amax) trailer[0] = wmax, trailer[2] = trailer[3] = 0.0f;  // (the whole trailer, as the zero fill of the other path)
  }
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int idx = (int)(e & 7);
    size_t q = e >> 3;
    const int col = (int)(q & 127);
    q >>= 7;
    const int kh = (int)(q & 1);
    q >>= 1;
    const int ks = (int)(q & 1);
    q >>= 1;
    const int cb = (int)(q % ncoblk), chunk = (int)(q / ncoblk);
    const int co = cb * 128 + col, ci = chunk * PWS_CK + ks * 16 + kh * 8 + idx;
    const float x = (co < cout && ci < cin) ? w[(size_t)co * s_co + (size_t)ci * s_ci] : 0.0f;
    unsigned p0, p1, p2;
    if (mode == SPLIT_F16X3) {
      split2h(x * sw, 0.0f, p0, p1);
      if (x2w) p1 = 0u;
      p2 = 0u;
    } else {
      split3(x, 0.0f, p0, p1, p2);
    }
    const unsigned pp[3] = {p0, p1, p2};
    for (int s = 0; s < 3; ++s)
      wp[((((((size_t)chunk * ncoblk + cb) * 2 + ks) * 3 + s) * 2 + kh) * 128 + col) * 8 + idx] = (unsigned short)(pp[s] & 0xffff);
  }
}

extern "C" size_t p2pb_pointwise_split_packed_bytes(int cout, int cin) {
  const size_t nchunk = (cin + PWS_CK - 1) / PWS_CK, ncoblk = (cout + 127) / 128;
  return nchunk * ncoblk * (2 * 3 * 2 * 128) * 16 + 16;  // + trailer {max|w| bits, output scale, -, -} (fp16 mode)
}

static int pw_pack_split(int cout, int cin, const float *w, void *wp, bool adjoint, void *stream, const unsigned *amax = nullptr) {
  if (cout <= 0 || cin <= 0) return P2PB_EINVAL;
  const int nchunk = (cin + PWS_CK - 1) / PWS_CK, ncoblk = (cout + 127) / 128;
  const size_t total = (size_t)nchunk * ncoblk * 2 * 2 * 128 * 8;
  // the pack is made for the arithmetic selected NOW (p2pb_set_split_terms); callers re-pack after a switch
  float *trailer = (float *)((char *)wp + (size_t)nchunk * ncoblk * PWS_TILE * 16);
  static const long x2w = p2pb_experiment_long("x2w", 0);
  const int mode = p2pb_g_split_terms;
  if (mode == SPLIT_F16X3 && !amax) {
    const int rc = p2pb_zero_async(trailer, 16, (hipStream_t)stream);
    if (rc) return rc;
    hipLaunchKernelGGL(absmax_bits_kernel, dim3(absmax_blocks((size_t)cout * cin)), dim3(256), 0, (hipStream_t)stream, w, (size_t)cout * cin,
                       (unsigned *)trailer);
  }
  hipLaunchKernelGGL(pw_pack_split_kernel, dim3((unsigned)((total + 255) / 256 > 2048 ? 2048 : (total + 255) / 256)),
                     dim3(256), 0, (hipStream_t)stream, cout, cin, nchunk, ncoblk, w, (unsigned short *)wp,
                     mode | ((x2w && mode == SPLIT_F16X3 && !adjoint) ? SPLIT_X2W_FLAG : 0), trailer,
                     adjoint ? 1L : (long)cin, adjoint ? (long)cout : 1L, mode == SPLIT_F16X3 ? amax : nullptr);
  return p2pb_launch_status();
}
extern "C" int p2pb_pointwise_pack_weights_split(int cout, int cin, const float *w, void *wp, void *stream) {
  return pw_pack_split(cout, cin, w, wp, false, stream);
}
extern "C" int p2pb_pointwise_pack_weights_split_adjoint(int cout, int cin, const float *w_forward, void *wp, void *stream) {
  return pw_pack_split(cout, cin, w_forward, wp, true, stream);
}
extern "C" int p2pb_pointwise_pack_weights_split_amax(int cout, int cin, const float *w, void *wp, const unsigned *amax_bits,
                                                      void *stream) {
  return amax_bits ? pw_pack_split(cout, cin, w, wp, false, stream, amax_bits) : P2PB_EINVAL;
}

// The GroupNorm(+AdaGN) that follows the layer (the fin_* arguments of the three statistics-producing entry points below, common.h
// GnFinish; scale == NULL: none). An entry point checks it BEFORE launching anything (pw_fin_ok) and puts gn_affine_kernel behind
// its producer, in stream order (pw_finish_behind).
static GnFinish pw_fin(double count_per_channel, int groups, const float *gamma, const float *beta, const float *style,
                       int style_stride, float eps, float *scale, float *shift, float *chmean) {
  GnFinish f = {};
  f.gamma = gamma, f.beta = beta, f.style = style, f.scale = scale, f.shift = shift, f.chmean = chmean;
  f.count_per_channel = count_per_channel, f.style_stride = style_stride, f.groups = groups, f.eps = eps;
  return f;
}
// (gn_shape_ok, ADVICE r4: a MyGroupNorm(32, cout) with cout % 32 != 0, or cout / groups > 256, ran gn_finish_group with a
//  truncated group / past its 256-entry LDS table and read gamma out of bounds)
static bool pw_fin_ok(const GnFinish &f, int cout, const float *stats_part) {
  return !f.scale || (stats_part && f.shift && f.count_per_channel > 0.0 && gn_shape_ok(cout, f.groups, f.style, f.style_stride));
}
static int pw_finish_behind(int rc, int b, int cout, int P, const float *stats_part, const GnFinish &f, hipStream_t s) {
  if (rc != 0 || !f.scale) return rc;
  return p2pb_gn_affine_launch(b, cout, (P + 255) / 256 * 4, stats_part, f, s);
}

// The LDS-tiled forms of a layer on the split pack, in the arithmetic selected now.
static int pw_run_split(const PwArgs &a) {
  const int mode = p2pb_g_split_terms;
  // 256-channel workgroups when the grid still holds >= 4 of them per CU (P2PB_EXPERIMENT pw_wm=2 / 4 overrides: A/B timing)
  static const int wm_env = (int)p2pb_experiment_long("pw_wm", 0);
  const bool wm4 = !a.out_pm && (wm_env ? wm_env == 4
                                         : (a.cout >= 512 && (long)((a.P + 127) / 128) * ((a.cout + 255) / 256) * a.b >= 1024));
  // bf16x3, the training data gradient's arithmetic: plain operand, no pooling, channel-major output
  if (mode == SPLIT_BF16X3 && (a.in_scale || a.minmax || a.out_pm)) return P2PB_EINVAL;
  // The layers that qualify for 256-channel workgroups AND come in whole 512-channel blocks with an even number of
  // 32-channel stages run the ping-pong kernel (pw_pp512.h: one 8-wave workgroup per CU on 512 channels x 128 positions, all
  // 160 KB of LDS, weight tiles by LDS-DMA, the two waves of a SIMD in opposite phase; any position count).
  // P2PB_EXPERIMENT pw_pp=0 keeps pw_split_kernel (A/B timing).
  static const int pp_env = (int)p2pb_experiment_long("pw_pp", 1);
  if (pp_env && wm4 && mode == SPLIT_F16X3 && a.cin % 64 == 0 && a.cout % 512 == 0 && (!a.minmax || a.pool_u == 0) &&
      (size_t)a.cin * a.P * 4 < (1ull << 31)) {  // (its operand descriptor holds one sample: 32-bit byte offsets)
    p2pb_note_pointwise_form(a.cin, a.cout, a.P, P2PB_FORM_PW_PINGPONG);
    return pw_pp512_launch(a);
  }
  p2pb_note_pointwise_form(a.cin, a.cout, a.P, wm4 ? P2PB_FORM_PW_SPLIT256 : P2PB_FORM_PW_SPLIT128);
  return pw_split_launch(a, mode, wm4);
}

// Which kernel runs the layer. 16-byte rows = pw_wide_ok: every form but pw_conv_kernel needs them.
static int pw_run(const PwArgs &a, int flags) {
  const bool rows16 = pw_wide_ok(a.P, a.in, a.out);
  if ((flags & PW_SPLIT_PACK) && (flags & PW_WIDE_TILING)) {  // narrow layer on the split pack: the wide tiling with f16x3 products
    if (!rows16 || p2pb_g_split_terms != SPLIT_F16X3) return P2PB_EINVAL;
    p2pb_note_pointwise_form(a.cin, a.cout, a.P, P2PB_FORM_PW_WIDE_F16);
    return pw_wide_f16_launch(a);
  }
  if (flags & PW_SPLIT_PACK) return rows16 ? pw_run_split(a) : P2PB_EINVAL;
  if (rows16) {
    p2pb_note_pointwise_form(a.cin, a.cout, a.P, P2PB_FORM_PW_WIDE_FP32);
    return pw_wide_fp32_launch(a);
  }
  if (a.minmax || a.out_pm) return P2PB_EINVAL;  // (the unaligned fallback: plain form only)
  p2pb_note_pointwise_form(a.cin, a.cout, a.P, P2PB_FORM_PW_FP32);
  return pw_conv_launch(a);
}

extern "C" size_t p2pb_pointwise_stats_floats(int b, int cout, int npos) {
  return (size_t)b * ((npos + 255) / 256) * 4 * cout * 2;
}

extern "C" int p2pb_pointwise_conv_forward(int b, int cin, int cout, int npos, const float *in, const void *wp_any,
                                           const float *bias, const float *bias_b, const float *in_scale,
                                           const float *in_shift, int in_swish, int flags, float *out,
                                           float *stats_part, double fin_count_per_channel, int fin_groups,
                                           const float *fin_gamma, const float *fin_beta, const float *fin_style,
                                           int fin_style_stride, float fin_eps, float *fin_scale, float *fin_shift,
                                           float *fin_chmean, void *stream) {
  const GnFinish f = pw_fin(fin_count_per_channel, fin_groups, fin_gamma, fin_beta, fin_style, fin_style_stride, fin_eps, fin_scale,
                            fin_shift, fin_chmean);
  if (!pw_fin_ok(f, cout, stats_part)) return P2PB_EINVAL;
  if (b <= 0 || cin <= 0 || cout <= 0 || npos <= 0 || !out) return P2PB_EINVAL;
  const int out_pm = (flags & PW_OUT_POINT_MAJOR) != 0;
  if (out_pm && stats_part) return P2PB_EINVAL;
  const PwArgs a = {b,   cin,        cout,    npos, in,     wp_any, bias, bias_b, in_scale, in_shift, in_swish,
                    out, stats_part, nullptr, 0,    out_pm, (hipStream_t)stream};
  return pw_finish_behind(pw_run(a, flags), b, cout, npos, stats_part, f, a.s);
}

extern "C" int p2pb_pointwise_pool_supported(int npos, int pool_u) {
  const bool uok = pool_u == 0 || pool_u == 4 || pool_u == 8 || pool_u == 16 || pool_u == 32 || pool_u == 64;
  return npos > 0 && npos % 4 == 0 && uok && (pool_u == 0 || npos % pool_u == 0);
}

extern "C" size_t p2pb_pointwise_minmax_floats(int b, int cout, int npos, int pool_u, int flags) {
  const bool split_tiling = (flags & PW_SPLIT_PACK) && !(flags & PW_WIDE_TILING);
  if (pool_u == 0) return (size_t)b * (split_tiling ? (npos + 127) / 128 * 2 : (npos + 511) / 512 * 4) * cout * 2;
  return (size_t)b * cout * (npos / pool_u) * 2;
}

extern "C" int p2pb_pointwise_conv_pool_forward(int b, int cin, int cout, int npos, const float *in,
                                                const void *wp_any, const float *bias, const float *bias_b,
                                                const float *in_scale, const float *in_shift, int in_swish, int flags,
                                                float *out, float *stats_part, int pool_u, float *minmax,
                                                double fin_count_per_channel, int fin_groups, const float *fin_gamma,
                                                const float *fin_beta, const float *fin_style, int fin_style_stride,
                                                float fin_eps, float *fin_scale, float *fin_shift, float *fin_chmean,
                                                void *stream) {
  const GnFinish f = pw_fin(fin_count_per_channel, fin_groups, fin_gamma, fin_beta, fin_style, fin_style_stride, fin_eps, fin_scale,
                            fin_shift, fin_chmean);
  if (!pw_fin_ok(f, cout, stats_part)) return P2PB_EINVAL;
  if (b <= 0 || cin <= 0 || cout <= 0 || npos <= 0 || !minmax || !stats_part) return P2PB_EINVAL;
  if (!p2pb_pointwise_pool_supported(npos, pool_u) || !pw_wide_ok(npos, in, out)) return P2PB_EINVAL;
  const PwArgs a = {b,   cin,        cout,   npos,   in, wp_any, bias, bias_b, in_scale, in_shift, in_swish,
                    out, stats_part, minmax, pool_u, 0,  (hipStream_t)stream};
  return pw_finish_behind(pw_run(a, flags), b, cout, npos, stats_part, f, a.s);
}

// The last layer of a set abstraction's MLP on the GROUPED tensor without building it (pw_wide_kernel<GATHER>):
//   operand[ci, (mi, ui)] = zt[b, idx[b, mi, ui], ci] - cxt[b, mi, ci]   (zt f32[b,n,cin], cxt f32[b,m,cin] point-major,
//   idx i32[b,m,u]: what p2pb_group_sub writes out as f32[b,cin,m*u]), folded norm + Swish applied on load, then the
//   1x1 convolution with the statistics + neighbourhood {min, max} epilogue of p2pb_pointwise_conv_pool_forward (output
//   never stored). wp_split = the split pack; f16x3 arithmetic; cin % 8 == 0, u in {4, 8, 16, 32, 64}.
extern "C" int p2pb_pointwise_conv_pool_gather(int b, int cin, int cout, int n, int m, int u, const float *zt,
                                               const float *cxt, const int *idx, const void *wp_split, const float *bias,
                                               const float *in_scale, const float *in_shift, int in_swish,
                                               float *stats_part, float *minmax, double fin_count_per_channel,
                                               int fin_groups, const float *fin_gamma, const float *fin_beta,
                                               const float *fin_style, int fin_style_stride, float fin_eps, float *fin_scale,
                                               float *fin_shift, float *fin_chmean, void *stream) {
  const GnFinish f = pw_fin(fin_count_per_channel, fin_groups, fin_gamma, fin_beta, fin_style, fin_style_stride, fin_eps, fin_scale,
                            fin_shift, fin_chmean);
  const long npos = (long)m * u;
  if (b <= 0 || cin <= 0 || cout <= 0 || n <= 0 || m <= 0 || !zt || !idx || !wp_split || !in_scale || !in_shift ||
      !stats_part || !minmax || (cin & 7) || npos > 0x7fffffffL || !p2pb_pointwise_pool_supported((int)npos, u) || u == 0 ||
      p2pb_g_split_terms != SPLIT_F16X3 || (((uintptr_t)zt | (uintptr_t)cxt) & 15) || !pw_fin_ok(f, cout, stats_part))
    return P2PB_EINVAL;
  const PwArgs a = {b,       cin,        cout,   (int)npos, zt, wp_split, bias, nullptr, in_scale, in_shift, in_swish,
                    nullptr, stats_part, minmax, u,         0,  (hipStream_t)stream};
  p2pb_note_pointwise_form(cin, cout, a.P, P2PB_FORM_PW_GATHER);
  return pw_finish_behind(pw_gather_launch(a, PwGather{cxt, idx, n, u}), b, cout, a.P, stats_part, f, a.s);
}
