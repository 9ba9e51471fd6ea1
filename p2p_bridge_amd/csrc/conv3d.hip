// conv3d.hip -- the voxel convolution's C entry points (forward, list-driven sparse, compact, compact on a pre-split grid), the
// f16x3 instantiations of the split-operand kernels (conv3d_split.h, conv3d_compact.h: the default arithmetic), the weight packs
// of the split form and the pre-split operand grid. conv3d_common.h has the map of the other files.
#include "conv3d_compact.h"
#include "absmax.h"

#ifdef CONV_TIMELINE  // experiment builds only (tools/exp_conv_timeline.py): where the stamps of this object's kernels go
extern "C" int p2pb_conv_timeline_set(void *p) {
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(conv_tl_buf), &p, sizeof(p));
}
#endif

// packed weights: wt[tap][chunk16][split 3][khalf 2][cout_pad][8 bf16]; element idx = channel chunk*16 + khalf*8 + idx
// mode SPLIT_F16X3 (common.h): planes 0, 1 = the fp16 pair of w * S_w, plane 2 unused; trailer = {max|w| bits, 1 / (S_x S_w)}
// w element (co, ci, tap) at w[co * s_co + ci * s_ci + (flip ? 26 - tap : tap)]: (cin * 27, 27, no flip) for a layer's own
// weight; (27, cout * 27, flip) packs the ADJOINT (data-gradient) operator straight from the forward weight [cin][cout][27]
// -- a correlation's adjoint is the correlation with the point-reflected kernel and the channel roles swapped
static __global__ void conv3d_pack_split_kernel(int cout, int cin, int nchunk, int cout_pad, const float *__restrict__ w,
                                        unsigned short *__restrict__ wt, int mode, float *__restrict__ trailer, long s_co,
                                        long s_ci, int flip, const unsigned *__restrict__ amax) {
  const size_t total = (size_t)27 * nchunk * 2 * cout_pad * 8;  // one thread per (tap, chunk, khalf, co, idx)
  // max |w| (bits): from the caller's slot (amax: the optimiser keeps it per tensor, csrc/optim.hip) or from the reduction
  // launched in front of this kernel (trailer[0])
  const bool x2w = (mode & SPLIT_X2W_FLAG) != 0;  // (pricing experiment, common.h: a zero low plane)
  mode &= 0xff;
  const float wmax = amax ? __builtin_bit_cast(float, *amax) : trailer[0];
  const float sw = mode == SPLIT_F16X3 ? f16_weight_scale(wmax) : 1.0f;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    trailer[1] = mode == SPLIT_F16X3 ? 1.0f / (SPLIT_F16_SX * sw) : 1.0f;
    if (amax) trailer[0] = wmax, trailer[2] = trailer[3] = 0.0f;  // (the whole trailer, as the zero fill of the other path)
  }
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int idx = (int)(e & 7);
    size_t q = e >> 3;
    const int co = (int)(q % cout_pad);
    q /= cout_pad;
    const int kh = (int)(q & 1);
    q >>= 1;
    const int chunk = (int)(q % nchunk), tap = (int)(q / nchunk);
    const int ci = chunk * CONV_SCK + kh * 8 + idx;
    const float x = (co < cout && ci < cin) ? w[(size_t)co * s_co + (size_t)ci * s_ci + (flip ? 26 - tap : tap)] : 0.0f;
    unsigned p0, p1, p2;
    if (mode == SPLIT_F16X3) {
      split2h(x * sw, 0.0f, p0, p1);
      if (x2w) p1 = 0u;
      p2 = 0u;
    } else {
      split3(x, 0.0f, p0, p1, p2);
    }
    const unsigned p[3] = {p0, p1, p2};
    for (int s = 0; s < 3; ++s)
      wt[((((size_t)(tap * nchunk + chunk) * 3 + s) * 2 + kh) * cout_pad + co) * 8 + idx] = (unsigned short)(p[s] & 0xffff);
  }
}

extern "C" size_t p2pb_conv3d_k3_split_packed_bytes(int cout, int cin) {
  const int nchunk = (cin + CONV_SCK - 1) / CONV_SCK, cout_pad = (cout + 63) / 64 * 64;
  return (size_t)27 * nchunk * 3 * 2 * cout_pad * 8 * sizeof(unsigned short) + 16;  // + trailer (fp16 mode's scales)
}

static int conv_pack_split(int cout, int cin, const float *w, void *wt_split, bool adjoint, void *stream,
                           const unsigned *amax = nullptr) {
  if (cout <= 0 || cin <= 0) return P2PB_EINVAL;
  const int nchunk = (cin + CONV_SCK - 1) / CONV_SCK, cout_pad = (cout + 63) / 64 * 64;
  const size_t total = (size_t)27 * nchunk * 2 * cout_pad * 8;
  // the pack is made for the arithmetic selected NOW (p2pb_set_split_terms); callers re-pack after a switch to / from 16
  float *trailer = (float *)((char *)wt_split + conv_split_trailer_bytes(nchunk, cout_pad));
  static const long x2w = p2pb_experiment_long("x2w", 0);
  const int mode = p2pb_g_split_terms;
  if (mode == SPLIT_F16X3 && !amax) {
    const int rc = p2pb_zero_async(trailer, 16, (hipStream_t)stream);
    if (rc) return rc;
    hipLaunchKernelGGL(absmax_bits_kernel, dim3(absmax_blocks((size_t)cout * cin * 27)), dim3(256), 0, (hipStream_t)stream, w, (size_t)cout * cin * 27,
                       (unsigned *)trailer);
  }
  hipLaunchKernelGGL(conv3d_pack_split_kernel, dim3((unsigned)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256)),
                     dim3(256), 0, (hipStream_t)stream, cout, cin, nchunk, cout_pad, w, (unsigned short *)wt_split,
                     mode | ((x2w && mode == SPLIT_F16X3 && !adjoint) ? SPLIT_X2W_FLAG : 0), trailer, adjoint ? 27L : (long)cin * 27, adjoint ? (long)cout * 27 : 27L, adjoint ? 1 : 0,
                     mode == SPLIT_F16X3 ? amax : nullptr);
  return p2pb_launch_status();
}
extern "C" int p2pb_conv3d_k3_pack_weights_split(int cout, int cin, const float *w, void *wt_split, void *stream) {
  return conv_pack_split(cout, cin, w, wt_split, false, stream);
}
extern "C" int p2pb_conv3d_k3_pack_weights_split_adjoint(int cout, int cin, const float *w_forward, void *wt_split, void *stream) {
  return conv_pack_split(cout, cin, w_forward, wt_split, true, stream);
}
extern "C" int p2pb_conv3d_k3_pack_weights_split_amax(int cout, int cin, const float *w, void *wt_split, const unsigned *amax_bits,
                                                      void *stream) {
  return amax_bits ? conv_pack_split(cout, cin, w, wt_split, false, stream, amax_bits) : P2PB_EINVAL;
}

extern "C" size_t p2pb_conv3d_k3_stats_floats(int b, int cout, int r) {
  return (size_t)b * conv_bricks(r) * 4 * cout * 2;
}

// the split kernels in the arithmetic selected NOW (p2pb_set_split_terms): f16x3 here, the others behind their bridge functions
static int conv_split(int r, int mt, const ConvArgs &a) {
  const int terms = p2pb_g_split_terms;
  if (terms == SPLIT_BF16X6) {
    if (a.pre) return P2PB_EINVAL;  // (the S format is the f16x3 arithmetic's)
    return conv3d_bf16x6_split(r, mt, a);
  }
  if (terms == SPLIT_BF16X3) {  // the training data gradient's form only: plain operand, channel-major
    if (a.pre || a.in_scale || a.in_sub || a.cl || a.brick_list) return P2PB_EINVAL;
    return conv3d_bf16x3_split(r, mt, a);
  }
  return conv_split_launch<SPLIT_F16X3>(r, mt, a);
}
static int conv_compact(int r, const ConvArgs &a) {
  const int terms = p2pb_g_split_terms;
  if (terms == SPLIT_BF16X3) return P2PB_EINVAL;  // (the data gradient's arithmetic: dense form only)
  if (a.pre && (terms == SPLIT_BF16X6 || a.in_scale || a.in_sub)) return P2PB_EINVAL;
  if (terms == SPLIT_BF16X6) return conv3d_bf16x6_compact(r, a);
  return conv_compact_launch<SPLIT_F16X3>(r, a);
}

// out[b,cout,r,r,r] = conv3d(xf(in[b,cin,r,r,r]), W) + bias, where xf(x) = x (in_scale == NULL) or
// swish?(x*in_scale[b,ci] + in_shift[b,ci]) - in_sub[b,ci]; out_class (optional, f32[b,27,cout]) replaces
// bias per boundary class; stats_part (optional) receives per-(b, slot, cout) {sum, sum of squares} of the
// output. flags: bit 0 = skip all-zero operand tiles (exact), bit 1 = compact 4x8x8 bricks, bit 2 = wt_packed is
// the split pack (p2pb_conv3d_k3_pack_weights_split) -> split-operand kernel. r in {4,8,16,32}.
extern "C" int p2pb_conv3d_k3_forward(int b, int cin, int cout, int r, const float *in, const float *wt_packed,
                                      const float *bias, const float *in_scale, const float *in_shift, int in_swish,
                                      float *out, float *stats_part, void *stream) {
  return p2pb_conv3d_k3_forward_ex(b, cin, cout, r, in, wt_packed, bias, nullptr, in_scale, in_shift, in_swish, nullptr,
                                   0, out, stats_part, stream);
}

extern "C" int p2pb_conv3d_k3_forward_ex(int b, int cin, int cout, int r, const float *in, const void *wt_packed,
                                         const float *bias, const float *out_class, const float *in_scale,
                                         const float *in_shift, int in_swish, const float *in_sub, int flags,
                                         float *out, float *stats_part, void *stream) {
  if (b <= 0 || cin <= 0 || cout <= 0) return P2PB_EINVAL;
  const bool compact = (flags & 2) != 0;
  const bool pre = (flags & 16) != 0;  // `in` is the pre-split operand grid (p2pb_conv3d_presplit / ..._cl_gather_split)
  if (pre && (flags & 12) != 12) return P2PB_EINVAL;
  ConvArgs a = {};
  a.b = b, a.cin = cin, a.cout = cout, a.in = in, a.wt = wt_packed, a.bias = bias, a.out_class = out_class;
  a.in_scale = in_scale, a.in_shift = in_shift, a.in_swish = in_swish, a.in_sub = in_sub, a.skip_zero = flags & 1;
  a.out = out, a.stats_part = stats_part, a.pre = pre, a.s = (hipStream_t)stream;
  a.cl = (flags & 8) != 0;  // voxel-major tensors in[b,r,r,r,cin], out[b,r,r,r,cout]
  if (flags & 4) {  // wt_packed is the split pack; always the compact tiling (same results, same slots)
    // 64 output channels per workgroup, unless that leaves under one workgroup per CU (small grids x small batches:
    // the 8^3 grids of a training batch of 8): 32 channels then double the workgroup count
    static const long wide_min = p2pb_experiment_long("conv_wide_min", 256);  // (A/B switch)
    const bool wide = cout > 32 && (long)conv_bricks(r) * ((cout + 63) / 64) * b >= wide_min;
    return conv_split(r, wide ? 2 : 1, a);
  }
  // 64 output channels per workgroup unless that leaves fewer than 2 workgroups per CU (small grids)
  const bool wide = cout > 32 && (long)conv_bricks(r) * ((cout + 63) / 64) * b >= 512;
  return conv3d_fp32_launch(r, compact, wide ? 2 : 1, a);
}

// list-driven sparse form: MFMA workgroups only for the `active` (sample, brick) pairs, constants for the
// `inactive` ones (lists from p2pb_conv3d_brick_lists). Compact geometry; r in {16, 32}.
extern "C" int p2pb_conv3d_k3_forward_sparse(int b, int cin, int cout, int r, const float *in, const void *wt_packed,
                                             const float *bias, const float *out_class, const float *in_scale,
                                             const float *in_shift, int in_swish, const float *in_sub, int flags,
                                             const int *active_list, const int *active_count,
                                             const int *inactive_list, const int *inactive_count, float *out,
                                             float *stats_part, void *stream) {
  if (b <= 0 || cin <= 0 || cout <= 0 || (r != 16 && r != 32) || !active_list || !inactive_list) return P2PB_EINVAL;
  if ((flags & 32) && !stats_part) return P2PB_EINVAL;  // (bit 5: the inactive bricks' statistics only -- there must be statistics)
  const bool pre = (flags & 16) != 0;  // `in` is the pre-split operand grid
  if (pre && (flags & 12) != 12) return P2PB_EINVAL;
  ConvArgs a = {};
  a.b = b, a.cin = cin, a.cout = cout, a.in = in, a.wt = wt_packed, a.bias = bias, a.out_class = out_class;
  a.in_scale = in_scale, a.in_shift = in_shift, a.in_swish = in_swish, a.in_sub = in_sub, a.skip_zero = 1;
  a.brick_list = active_list, a.brick_count = active_count, a.out = out, a.stats_part = stats_part;
  a.cl = (flags & 8) != 0, a.pre = pre, a.s = (hipStream_t)stream;
  conv3d_fill_launch(r, a, inactive_list, inactive_count, (flags & 32) != 0);
  const int mt = cout > 32 ? 2 : 1;
  return (flags & 4) ? conv_split(r, mt, a) : conv3d_fp32_launch(r, true, mt, a);
}

// compact form (conv3d_compact.h): alist / acount = ONE set of p2pb_conv3d_active_lists; flags bit 5 = listed outputs only
extern "C" int p2pb_conv3d_k3_forward_compact(int b, int cin, int cout, int r, const float *in, const void *wt_split,
                                              const float *bias, const float *out_class, const float *in_scale,
                                              const float *in_shift, int in_swish, const float *in_sub,
                                              const unsigned char *alist, const int *acount, float *out,
                                              float *stats_part, int flags, void *stream) {
  if (b <= 0 || cin <= 0 || cout <= 0 || !alist || !acount || (r != 8 && r != 16 && r != 32) || (flags & ~32)) return P2PB_EINVAL;
  ConvArgs a = {};
  a.b = b, a.cin = cin, a.cout = cout, a.in = in, a.wt = wt_split, a.bias = bias, a.out_class = out_class;
  a.in_scale = in_scale, a.in_shift = in_shift, a.in_swish = in_swish, a.in_sub = in_sub;
  a.skip_zero = 1 | ((flags & 32) ? 2 : 0);
  a.alist = alist, a.acount = acount, a.out = out, a.stats_part = stats_part, a.s = (hipStream_t)stream;
  return conv_compact(r, a);
}

// the compact form on a pre-split operand grid (S format, see PreStage): in_split u32x4[b][r^3][ceil(cin/16)][4]
extern "C" int p2pb_conv3d_k3_forward_compact_pre(int b, int cin, int cout, int r, const void *in_split,
                                                  const void *wt_split, const float *bias, const float *out_class,
                                                  const unsigned char *alist, const int *acount, float *out,
                                                  float *stats_part, int flags, void *stream) {
  if (b <= 0 || cin <= 0 || cout <= 0 || !in_split || !alist || !acount || (r != 8 && r != 16 && r != 32) || (flags & ~32))
    return P2PB_EINVAL;
  ConvArgs a = {};
  a.b = b, a.cin = cin, a.cout = cout, a.in = (const float *)in_split, a.wt = wt_split, a.bias = bias, a.out_class = out_class;
  a.skip_zero = (flags & 32) ? 2 : 0;  // (a pre-split stage is brought in whole: no zero-tile test)
  a.alist = alist, a.acount = acount, a.out = out, a.stats_part = stats_part, a.pre = true, a.s = (hipStream_t)stream;
  return conv_compact(r, a);
}

// y f32[b][nvox][c] (voxel-major) -> S format u32x4[b][nvox][ceil(c/16)][2 planes][2 khalf]: the operand transform of
// the split kernels' staging phase (folded norm + Swish - far-field value, then the fp16-pair split of 4 x value), once
// per element.
#define PRESPLIT_VT 128  // voxels per workgroup
static __global__ __launch_bounds__(256) void conv3d_presplit_kernel(int c, int nchunk, int nvox, const float *__restrict__ y,
                                                                     const float *__restrict__ in_scale,
                                                                     const float *__restrict__ in_shift, int in_swish,
                                                                     const float *__restrict__ in_sub,
                                                                     u32x4 *__restrict__ out) {
  // a thread keeps ONE group of 8 channels (its scale / shift / far-field value in registers) and walks the voxels of the
  // workgroup's tile: 256 / ng voxels per pass, a voxel's row read and written by ng neighbouring lanes (coalesced)
  const int b = blockIdx.y, ng = nchunk * 2, vpp = 256 / ng;
  const int g = threadIdx.x % ng, vl = threadIdx.x / ng, c0 = g * 8;
  if (vl >= vpp) return;
  float sc[8], sh[8], sub[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int ch = c0 + i;
    const bool ok = ch < c && in_scale != nullptr;
    sc[i] = ok ? in_scale[b * c + ch] : 1.0f;
    sh[i] = ok ? in_shift[b * c + ch] : 0.0f;
    sub[i] = (ok && in_sub) ? in_sub[b * c + ch] : 0.0f;
  }
  const int v0 = blockIdx.x * PRESPLIT_VT, v1 = min(v0 + PRESPLIT_VT, nvox);
  const bool quad = (c & 3) == 0;
  for (int v = v0 + vl; v < v1; v += vpp) {
    const float *src = y + ((size_t)b * nvox + v) * c + c0;
    float x[8];
    if (quad) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        f32x4 t = {0.0f, 0.0f, 0.0f, 0.0f};
        if (c0 + 4 * q < c) t = *(const f32x4 *)(src + 4 * q);
#pragma unroll
        for (int i = 0; i < 4; ++i) x[4 * q + i] = t[i];
      }
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) x[i] = c0 + i < c ? src[i] : 0.0f;
    }
    if (in_scale) {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (c0 + i < c) x[i] = xf_apply(x[i], sc[i], sh[i], in_swish) - sub[i];
    }
    u32x4 p0, p1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      unsigned a0, a1, a2;
      split_pair<SPLIT_F16X3>(x[2 * i], x[2 * i + 1], a0, a1, a2);
      p0[i] = a0;
      p1[i] = a1;
    }
    u32x4 *dst = out + (((size_t)b * nvox + v) * nchunk + (g >> 1)) * 4 + (g & 1);
    dst[0] = p0;
    dst[2] = p1;
  }
}

// y f32[b, nvox, c] -> out_split (S format, b * nvox * ceil(c/16) * 64 bytes); in_scale / in_shift / in_sub f32[b,c] or NULL
extern "C" int p2pb_conv3d_presplit(int b, int c, long nvox, const float *y, const float *in_scale, const float *in_shift,
                                    int in_swish, const float *in_sub, void *out_split, void *stream) {
  if (b <= 0 || c <= 0 || nvox <= 0 || nvox > 0x7fffffffL / 64 || !y || !out_split || (in_scale && !in_shift)) return P2PB_EINVAL;
  const int nchunk = (c + CONV_SCK - 1) / CONV_SCK;
  if (nchunk * 2 > 256) return P2PB_EINVAL;  // (<= 2048 channels)
  const dim3 grid(cdiv(nvox, PRESPLIT_VT), b);
  hipLaunchKernelGGL(conv3d_presplit_kernel, grid, dim3(256), 0, (hipStream_t)stream, c, nchunk, (int)nvox, y, in_scale,
                     in_shift, in_swish, in_sub, (u32x4 *)out_split);
  return p2pb_launch_status();
}
