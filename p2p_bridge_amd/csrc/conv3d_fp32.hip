// conv3d_fp32.hip -- the voxel convolution (conv3d_common.h) on the gfx950 matrix cores in exact fp32: conv_math = fp32.
//
// The reference calls cuDNN (TF32 on NVIDIA); CDNA4 has no TF32 but has an exact-fp32 MFMA (v_mfma_f32_32x32x2_f32,
// 157 TFLOP/s dense): every product is rounded once and accumulated in fp32, like an fmaf chain. It was the first form and is
// the yardstick the split-operand kernels (conv3d_split.h, the default: the same values at 1/3 of the matrix cycles) are pinned
// against; its pack is also what the far-field constants are summed from (conv3d_farfield.hip).
//
// Workgroup = 256 threads (4 waves) -> one brick of 256 voxels (8 N-tiles of 32) x NC output channels of
// one sample. Per chunk of CK input channels the workgroup stages the zero-padded halo brick
// [CK][TD+2][TH+2][TW+2] into LDS once (optional per-channel affine + Swish applied on the way in: that is
// how the preceding AdaGN + Swish is fused away), then every wave walks the 27 taps reading its B
// fragments from LDS at constant offsets; A fragments (packed weights) are 16-byte L1/L2 loads.
// Epilogue: + bias, store, and per-(sample, brick, wave, channel) {sum, sum of squares} partials for the
// GroupNorm that follows (reduced deterministically by gn_affine_kernel).
#include "conv3d_common.h"

// MT = 32-row output-channel tiles per workgroup (NC = 32*MT), XF = apply affine(+swish)(-sub) to the input
template <int R, bool COMPACT, int MT, bool XF, bool CL>
__global__ __launch_bounds__(256) void conv3d_k3_kernel(int cin, int cout, int nchunk, int cout_pad,
                                                        const float *__restrict__ in, const float *__restrict__ wt,
                                                        const float *__restrict__ bias,
                                                        const float *__restrict__ out_class,
                                                        const float *__restrict__ in_scale,
                                                        const float *__restrict__ in_shift, int in_swish,
                                                        const float *__restrict__ in_sub, int skip_zero,
                                                        const int *__restrict__ brick_list,
                                                        const int *__restrict__ brick_count,
                                                        float *__restrict__ out, float *__restrict__ stats_part) {
  using G = ConvGeom<R, COMPACT>;
  constexpr int HD = G::TD + 2, HH = G::TH + 2, HW = G::TW + 2;
  constexpr int PLANE = HD * HH * HW;
  constexpr int NTILES = (G::TD * G::TH * G::TW) / 32;  // N-tiles in the brick (8, or 2 for R=4)
  constexpr int BH = R / G::TH, BW = R / G::TW;          // bricks per sample along h, w
  constexpr int R3 = R * R * R;
  __shared__ float tile[CONV_CK * PLANE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, khalf = lane >> 5;
  // blockIdx.x -> brick. Workgroups are dealt to the 8 XCDs round-robin (id mod 8); with the zero-tile skip
  // the active bricks hug the surface, and a linear map would park a whole (h,w) column of bricks -- i.e.
  // all of the surface or none of it -- on one XCD. The compact geometry therefore uses a diagonal hash:
  // d-index = (x mod BD) - (3*bh + 5*bw), so consecutive ids walk diagonally through the grid.
  constexpr int BD = R / G::TD;
  constexpr int NBRICK = BD * BH * BW;
  int bd, bh, bw, b = blockIdx.z;
  if (brick_list) {  // compacted list of ACTIVE (sample, brick) pairs; the rest is written by conv3d_fill_kernel
    if ((int)blockIdx.x >= *brick_count) return;
    const int entry = brick_list[blockIdx.x];
    b = entry / NBRICK;
    const int bk = entry % NBRICK;
    bd = bk / (BH * BW);
    bh = (bk / BW) % BH;
    bw = bk % BW;
  } else if (COMPACT) {
    const int hi = blockIdx.x / BD, lo = blockIdx.x % BD;
    bh = hi / BW;
    bw = hi % BW;
    bd = (lo + 8 * BD - (3 * bh + 5 * bw)) % BD;
  } else {
    bd = blockIdx.x / (BH * BW);
    bh = (blockIdx.x / BW) % BH;
    bw = blockIdx.x % BW;
  }
  const int brick = (bd * BH + bh) * BW + bw;
  const int d0 = bd * G::TD, h0 = bh * G::TH, w0 = bw * G::TW;
  const int co0 = blockIdx.y * (32 * MT);

  // this wave's two N-tiles: tile index t = 2*wave + s ; origin of an N-tile inside the brick
  int nbase[2];
  bool nact[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int t = 2 * wave + s;
    nact[s] = t < NTILES;
    constexpr int HB = G::TH / G::NH;
    const int td = (t / HB) * G::ND, th = (t % HB) * G::NH;
    const int jw = l31 % G::TW, jr = l31 / G::TW;  // lane's voxel inside the N-tile
    const int jh = jr % G::NH, jd = jr / G::NH;
    nbase[s] = ((td + jd) * HH + (th + jh)) * HW + jw;
  }

  // staging map, fixed for the whole kernel: this thread stages halo positions tid, tid+256, ... of EVERY
  // channel of a chunk (channel-outer order keeps the folded scale/shift wave-uniform, i.e. scalar loads,
  // and needs only NP offsets instead of one per staged element)
  constexpr int NP = (PLANE + 255) / 256;
  int soff[NP];  // offset inside a channel's r^3 grid, or -1 outside the grid / beyond the halo
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int e = tid + j * 256;
    const int dz = e / (HH * HW), hy = (e / HW) % HH, wx = e % HW;
    const int d = d0 - 1 + dz, h = h0 - 1 + hy, w = w0 - 1 + wx;
    const bool ok = e < PLANE && (unsigned)d < (unsigned)R && (unsigned)h < (unsigned)R && (unsigned)w < (unsigned)R;
    soff[j] = ok ? (d * R + h) * R + w : -1;
  }

  f32x16 acc[MT][2];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][s][r] = 0.0f;

  const float *inb = in + (size_t)b * cin * R3;
  float stg[CONV_CK][NP];
  // unpredicated loads through scalar descriptors; halo positions outside the grid carry an out-of-range offset
  // and read the hardware's zero. Channel-major (reference) layout: one descriptor per channel row (rows past cin
  // are clamped and zeroed at staging time). Voxel-major layout (CL): a staged voxel's channels are contiguous,
  // 32 bytes per stage = 16-byte loads when cin % 4 == 0 (quads past cin are zeroed at staging time).
  unsigned voff[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j)
    voff[j] = soff[j] >= 0 ? (unsigned)soff[j] * (CL ? (unsigned)cin * 4u : 4u) : 0x80000000u;
  auto stage_load = [&](int ci0) {
    if (CL) {
      auto rs = __builtin_amdgcn_make_buffer_rsrc((void *)inb, 0, R3 * cin * 4, 0x00020000);
      if ((cin & 3) == 0) {
#pragma unroll
        for (int j = 0; j < NP; ++j)
#pragma unroll
          for (int q = 0; q < CONV_CK / 4; ++q) {
            const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff[j] + (unsigned)(ci0 + 4 * q) * 4u, 0, 0));
#pragma unroll
            for (int i = 0; i < 4; ++i) stg[4 * q + i][j] = v[i];
          }
      } else {
#pragma unroll
        for (int j = 0; j < NP; ++j)
#pragma unroll
          for (int c = 0; c < CONV_CK; ++c)
            stg[c][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, voff[j] + (unsigned)(ci0 + c) * 4u, 0, 0));
      }
    } else {
#pragma unroll
      for (int c = 0; c < CONV_CK; ++c) {
        auto rs = __builtin_amdgcn_make_buffer_rsrc((void *)(inb + (size_t)min(ci0 + c, cin - 1) * R3), 0, R3 * 4, 0x00020000);
#pragma unroll
        for (int j = 0; j < NP; ++j) stg[c][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, voff[j], 0, 0));
      }
    }
  };
  stage_load(0);

  for (int ci0 = 0; ci0 < cin; ci0 += CONV_CK) {
    __syncthreads();  // everyone is done reading the previous chunk's tile
    int nonzero = 0;
#pragma unroll
    for (int c = 0; c < CONV_CK; ++c) {
      float sc = 1.0f, sh = 0.0f, sub = 0.0f;
      const bool cok = ci0 + c < cin;
      if (XF && cok) {
        sc = in_scale[b * cin + ci0 + c];
        sh = in_shift[b * cin + ci0 + c];
        if (in_sub) sub = in_sub[b * cin + ci0 + c];
      }
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        float v = cok ? stg[c][j] : 0.0f;
        if (XF && cok && soff[j] >= 0) v = xf_apply(v, sc, sh, in_swish) - sub;
        nonzero |= (v != 0.0f);
        if (tid + j * 256 < PLANE) tile[c * PLANE + tid + j * 256] = v;
      }
    }
    // barrier + "is any staged value non-zero" in one; an all-zero tile contributes exactly +0
    const int any = skip_zero ? __syncthreads_or(nonzero) : (__syncthreads(), 1);
    if (ci0 + CONV_CK < cin) {  // next chunk's loads fly during the MFMAs
      int nxt = ci0 + CONV_CK;
      asm volatile("" : "+s"(nxt));  // opaque: unpredicated loads would otherwise be hoisted above the staging phase
      stage_load(nxt);
    }
    if (!any) continue;

    // ---- 27 taps x CK/2 k-pairs of MFMAs; A fragments: one 16-byte load per (tap, M-tile), next tap
    //      prefetched while the current one is multiplied
    const float *wchunk = wt + ((((size_t)(ci0 / CONV_CK)) * 2 + khalf) * cout_pad + co0 + l31) * 4;
    const size_t wtap_stride = (size_t)nchunk * 2 * cout_pad * 4;
    f32x4 a_cur[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) a_cur[m] = *(const f32x4 *)(wchunk + (size_t)m * 32 * 4);
    // B fragments are read one k-pair ahead, A fragments one tap ahead; the scheduling barriers pin both
    // prefetches (left alone, the scheduler sinks every load to just before its first use, so each group of
    // MFMAs would start with an exposed LDS / L2 round trip)
    float bf[2], bf_nxt[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) bf[s] = tile[khalf * PLANE + nbase[s]];
#pragma unroll
    for (int tap = 0; tap < 27; ++tap) {
      f32x4 a_nxt[MT];
      if (tap + 1 < 27) {
#pragma unroll
        for (int m = 0; m < MT; ++m)
          a_nxt[m] = *(const f32x4 *)(wchunk + (size_t)(tap + 1) * wtap_stride + (size_t)m * 32 * 4);
      }
#pragma unroll
      for (int kk = 0; kk < CONV_CK / 2; ++kk) {
        const int step = tap * (CONV_CK / 2) + kk + 1;  // the (tap, k-pair) after this one
        if (step < 27 * (CONV_CK / 2)) {
          const int ntap = step / (CONV_CK / 2), nkk = step % (CONV_CK / 2);
          const int ntoff = ((ntap / 9) * HH + (ntap / 3) % 3) * HW + ntap % 3;
#pragma unroll
          for (int s = 0; s < 2; ++s) bf_nxt[s] = tile[(2 * nkk + khalf) * PLANE + nbase[s] + ntoff];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int s = 0; s < 2; ++s)
            acc[m][s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[m][kk], bf[s], acc[m][s], 0, 0, 0);
#pragma unroll
        for (int s = 0; s < 2; ++s) bf[s] = bf_nxt[s];
      }
      if (tap + 1 < 27) {
#pragma unroll
        for (int m = 0; m < MT; ++m) a_cur[m] = a_nxt[m];
      }
    }
  }

  // ---- epilogue: bias (or the boundary-class constant), store, GroupNorm partial statistics
  float *outb = out + (size_t)b * cout * R3;
  // voxel coordinates / boundary class of this lane's column in each of the wave's two N-tiles
  int vox[2], cls[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int t = 2 * wave + s;
    constexpr int HB = G::TH / G::NH;
    const int td = (t / HB) * G::ND, th = (t % HB) * G::NH;
    const int jw = l31 % G::TW, jr = l31 / G::TW;
    const int d = d0 + td + jr / G::NH, h = h0 + th + jr % G::NH, w = w0 + jw;
    vox[s] = (d * R + h) * R + w;
    const int cd = d == 0 ? 0 : (d == R - 1 ? 2 : 1), ch = h == 0 ? 0 : (h == R - 1 ? 2 : 1),
              cw = w == 0 ? 0 : (w == R - 1 ? 2 : 1);
    cls[s] = (cd * 3 + ch) * 3 + cw;
  }
#pragma unroll
  for (int m = 0; m < MT; ++m) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float vv[2][4];  // voxel-major stores: the four consecutive channels of register group g, per N-tile
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 4 * g + i;
        const int co = co0 + m * 32 + i + 8 * g + 4 * khalf;
        const bool cok = co < cout;
        const float bv = (cok && !out_class) ? bias[co] : 0.0f;
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          if (!nact[s]) continue;
          float v = acc[m][s][r] + bv;
          if (out_class && cok) v += out_class[((size_t)b * 27 + cls[s]) * cout + co];
          if (CL) vv[s][i] = v;
          else if (cok) outb[(size_t)co * R3 + vox[s]] = v;
          s1 += v;
          s2 += v * v;
        }
        if (stats_part) {
          // sum over the 32 lanes of this half-wave (a channel row lives in exactly one half of the wave),
          // one private slot per (sample, brick, wave, channel): plain stores, reduced later in fixed order
          s1 = halfwave_sum_to_last(s1);
          s2 = halfwave_sum_to_last(s2);
          if (l31 == 31 && cok) {
            float *p = stats_part + ((((size_t)b * NBRICK + brick) * 4 + wave) * cout + co) * 2;
            p[0] = s1;
            p[1] = s2;
          }
        }
      }
      if (CL) {
        const int cq = co0 + m * 32 + 8 * g + 4 * khalf;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          if (!nact[s]) continue;
          float *q = outb + (size_t)vox[s] * cout + cq;
          if (cq + 3 < cout && (cout & 3) == 0) *(f32x4 *)q = f32x4{vv[s][0], vv[s][1], vv[s][2], vv[s][3]};
          else
            for (int i = 0; i < 4; ++i)
              if (cq + i < cout) q[i] = vv[s][i];
        }
      }
    }
  }
}

// weights [cout][cin][3][3][3] -> packed [27][cin_pad/8][2][cout_pad][4] (zero padded):
// element (tap, chunk, khalf, co, kk) = W[co][chunk*8 + 2*kk + khalf][tap], so that the four k-pair
// values one lane needs for a tap are one aligned 16-byte load and lanes 0..31 read 512 contiguous bytes
static __global__ void conv3d_pack_kernel(int cout, int cin, int nchunk, int cout_pad, const float *__restrict__ w,
                                   float *__restrict__ wt) {
  const size_t total = (size_t)27 * nchunk * 8 * cout_pad;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int kk = (int)(e & 3);
    const int co = (int)((e >> 2) % cout_pad);
    size_t q = (e >> 2) / cout_pad;
    const int kh = (int)(q & 1);
    q >>= 1;
    const int chunk = (int)(q % nchunk), tap = (int)(q / nchunk);
    const int ci = chunk * 8 + 2 * kk + kh;
    wt[e] = (co < cout && ci < cin) ? w[((size_t)co * cin + ci) * 27 + tap] : 0.0f;
  }
}

extern "C" int p2pb_conv3d_k3_pack_weights(int cout, int cin, const float *w, float *wt_packed, void *stream) {
  if (cout <= 0 || cin <= 0) return P2PB_EINVAL;
  const int nchunk = (cin + CONV_CK - 1) / CONV_CK, cout_pad = (cout + 63) / 64 * 64;
  const size_t total = (size_t)27 * nchunk * 8 * cout_pad;
  hipLaunchKernelGGL(conv3d_pack_kernel, dim3((unsigned)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256)),
                     dim3(256), 0, (hipStream_t)stream, cout, cin, nchunk, cout_pad, w, wt_packed);
  return p2pb_launch_status();
}

extern "C" size_t p2pb_conv3d_k3_packed_floats(int cout, int cin) {
  const int cin_pad = (cin + CONV_CK - 1) / CONV_CK * CONV_CK, cout_pad = (cout + 63) / 64 * 64;
  return (size_t)27 * cin_pad * cout_pad;
}

template <int R, bool COMPACT, int MT, bool XF, bool CL>
static int conv_fp32_go(const ConvArgs &a) {
  const int nchunk = (a.cin + CONV_CK - 1) / CONV_CK, cout_pad = (a.cout + 63) / 64 * 64;
  dim3 grid(conv_bricks(R), (a.cout + 32 * MT - 1) / (32 * MT), a.b);
  if (a.brick_list) grid = dim3(conv_bricks(R) * a.b, (a.cout + 32 * MT - 1) / (32 * MT), 1);
  hipLaunchKernelGGL((conv3d_k3_kernel<R, COMPACT, MT, XF, CL>), grid, dim3(256), 0, a.s, a.cin, a.cout, nchunk, cout_pad, a.in,
                     (const float *)a.wt, a.bias, a.out_class, a.in_scale, a.in_shift, a.in_swish, a.in_sub, a.skip_zero,
                     a.brick_list, a.brick_count, a.out, a.stats_part);
  return p2pb_launch_status();
}
template <int R, bool COMPACT>
static int conv_fp32_form(int mt, const ConvArgs &a) {
  return for_flag(mt == 2, [&](auto WIDE) {
    return for_flag(a.in_scale != nullptr, [&](auto XF) {
      return for_flag(a.cl, [&](auto CL) {
        return conv_fp32_go<R, COMPACT, decltype(WIDE)::value ? 2 : 1, decltype(XF)::value, decltype(CL)::value>(a);
      });
    });
  });
}
int conv3d_fp32_launch(int r, bool compact, int mt, const ConvArgs &a) {
  switch (r) {
    case 32: return compact ? conv_fp32_form<32, true>(mt, a) : conv_fp32_form<32, false>(mt, a);
    case 16: return compact ? conv_fp32_form<16, true>(mt, a) : conv_fp32_form<16, false>(mt, a);
    case 8: return conv_fp32_form<8, false>(mt, a);
    case 4: return conv_fp32_form<4, false>(mt, a);
    default: return P2PB_EINVAL;
  }
}
