// conv3d_compact.h -- the compact (listed-voxel) form of the split-operand kernel (conv3d_split.h, whose tap loops and pre-split
// stage it shares) and its launcher; the lists come from active_lists_kernel (conv3d_lists.hip). Instantiated by conv3d.hip
// (f16x3) and conv3d_bf16x6.hip.
//
// Compact form of the split kernel: voxel-level sparsity inside the bricks.
//
// The first convolution of a PVConv is non-constant only on D1 = dilate(occupied, 1) (elsewhere every input in
// the 3x3x3 window is zero and the output is the bias), the second -- in its far-field form, operand x - a --
// only on D2 = dilate(D1, 1) (elsewhere the output is the boundary-class constant K). D1 / D2 are 15 % / 26 % of a
// 32^3 grid, 30 % / 50 % at 16^3, 57 % / 87 % at 8^3, while a brick (4x8x8) is "active" as soon as it holds one
// such voxel. So a workgroup computes only the ACTIVE outputs of its brick: their local ids come from a per-brick
// list (coordinate-only: built once per (level, resolution) on the geometry stream), they are packed 32 to an
// MFMA column tile, and the B fragment of (tile, tap) is still "halo slot of my voxel + constant tap offset" --
// the main loop is the split kernel's, with 1..8 gathered tiles instead of 8 fixed ones. The remaining voxels of the
// brick get their constant (and its exact contribution to the GroupNorm statistics) from the same workgroup.
// Waves: WM = 2 -> 64 channels per workgroup, the tiles are dealt to two wave columns; WM = 1 (layers of 32
// channels) -> four wave columns. Values are bit-identical to the dense split kernel on the computed outputs.
#pragma once
#include "conv3d_split.h"

template <int R, int WM, bool XF, int TERMS, bool PRE = false>  // TERMS, PRE: see conv3d_k3_split_kernel
__global__ __launch_bounds__(256, TERMS == SPLIT_F16X3 ? CONV_F16_WAVES : 2) void conv3d_k3_compact_kernel(int cin, int cout, int nchunk, int cout_pad,
                                                                const float *__restrict__ in,
                                                                const unsigned short *__restrict__ wt,
                                                                const float *__restrict__ bias,
                                                                const float *__restrict__ out_class,
                                                                const float *__restrict__ in_scale,
                                                                const float *__restrict__ in_shift, int in_swish,
                                                                const float *__restrict__ in_sub, int skip_zero,
                                                                const unsigned char *__restrict__ alist,
                                                                const int *__restrict__ acount,
                                                                float *__restrict__ out, float *__restrict__ stats_part) {
  using G = SplitGeom<R>;
  constexpr int HD = G::TD + 2, HH = G::TH + 2, HW = G::TW + 2;
  constexpr int PLANE = HD * HH * HW;
  constexpr int BH = R / G::TH, BW = R / G::TW, BD = R / G::TD, NBRICK = BD * BH * BW;
  constexpr int R3 = R * R * R;
  constexpr int WN = 4 / WM;
  static_assert(!PRE || (TERMS == SPLIT_F16X3 && !XF), "pre-split operands: f16x3, transform applied");
  __shared__ u32x4 tile[split_planes(TERMS) * 2 * PLANE];
  __shared__ u32x4 tile2[PRE ? split_planes(TERMS) * 2 * PLANE : 1];  // (its own object: see the split kernel)
  __shared__ unsigned char lst[256];
  __shared__ int ncls[27];
  __shared__ float wstat[4][2][16][2];  // per wave, half-wave, accumulator row: {sum, sumsq} over the active outputs

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, khalf = lane >> 5;
  // XCD-aware order (see the split kernel): XCD x gets the x-th contiguous eighth of (sample, brick, channel block)
  const unsigned lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  const unsigned nblk = gridDim.x * gridDim.y * gridDim.z;
  const int ncoblk = (cout + 32 * WM - 1) / (32 * WM);
  const unsigned v = nblk % 8 == 0 ? (lin % 8) * (nblk / 8) + lin / 8 : lin;
  const unsigned per_sample = NBRICK * ncoblk;
  const int b = v / per_sample;
  const int brick = (v % per_sample) / ncoblk, coblk = (v % per_sample) % ncoblk;
  const int bd = brick / (BH * BW), bh = (brick / BW) % BH, bw = brick % BW;
  const int d0 = bd * G::TD, h0 = bh * G::TH, w0 = bw * G::TW;
  const int wm = wave / WN, wn = wave % WN;
  const int cob = coblk * (32 * WM);  // first channel of the workgroup
  const int co0 = cob + 32 * wm;      // first channel of this wave's M-tile

  CONV_TL_INIT
  CONV_TL_ID(tid);
  CONV_TL(tid);  // 0: start
  const int count = acount[(size_t)b * NBRICK + brick];
  lst[tid] = alist[((size_t)b * NBRICK + brick) * 256 + tid];
  if (tid < 27) ncls[tid] = 0;
  __syncthreads();
  CONV_TL(tid);  // 1: brick list in LDS
  const int ntiles = (count + 31) >> 5;
  auto vox_of = [&](int l, int &cls) {
    const int d = d0 + (l >> 6), h = h0 + ((l >> 3) & 7), w = w0 + (l & 7);
    const int cd = d == 0 ? 0 : (d == R - 1 ? 2 : 1), ch = h == 0 ? 0 : (h == R - 1 ? 2 : 1),
              cw = w == 0 ? 0 : (w == R - 1 ? 2 : 1);
    cls = (cd * 3 + ch) * 3 + cw;
    return (d * R + h) * R + w;
  };

  constexpr int NP = (PLANE + 255) / 256;
  int soff[NP];
  unsigned voff[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int e = tid + j * 256;
    const int dz = e / (HH * HW), hy = (e / HW) % HH, wx = e % HW;
    const int d = d0 - 1 + dz, h = h0 - 1 + hy, w = w0 - 1 + wx;
    const bool ok = e < PLANE && (unsigned)d < (unsigned)R && (unsigned)h < (unsigned)R && (unsigned)w < (unsigned)R;
    soff[j] = ok ? (d * R + h) * R + w : -1;
    voff[j] = ok ? (unsigned)soff[j] * (unsigned)cin * 4u : 0x80000000u;
  }
  const float *inb = in + (size_t)b * cin * R3;
  float *outb = out + (size_t)b * cout * R3;
  float stg[CONV_SCK][NP];
  auto stage_load = [&](int ci0) {
    auto rs = __builtin_amdgcn_make_buffer_rsrc((void *)inb, 0, R3 * cin * 4, 0x00020000);
    if ((cin & 3) == 0) {
#pragma unroll
      for (int j = 0; j < NP; ++j)
#pragma unroll
        for (int q = 0; q < CONV_SCK / 4; ++q) {
          const f32x4 x = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff[j] + (unsigned)(ci0 + 4 * q) * 4u, 0, 0));
#pragma unroll
          for (int i = 0; i < 4; ++i) stg[4 * q + i][j] = x[i];
        }
    } else {
#pragma unroll
      for (int j = 0; j < NP; ++j)
#pragma unroll
        for (int c = 0; c < CONV_SCK; ++c)
          stg[c][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, voff[j] + (unsigned)(ci0 + c) * 4u, 0, 0));
    }
  };

  if (l31 == 31) {  // this wave's statistics accumulate in LDS across the passes (touched by lanes 31 / 63 only)
#pragma unroll
    for (int r = 0; r < 16; ++r) wstat[wave][khalf][r][0] = wstat[wave][khalf][r][1] = 0.0f;
  }

  // wave column wn takes tiles wn, wn + WN, ...: nt of them (<= 8 / WN <= 4), wave-uniform. The whole stage loop is
  // specialised on nt (1..4): each count keeps split_taps' rolling schedule and only its own accumulators
  int nt = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i * WN + wn < ntiles) nt = i + 1;

  auto run = [&](auto ntc_tag) {
    constexpr int NTC = decltype(ntc_tag)::value;  // 0: this wave has no tile, it only helps staging
    constexpr int NA = NTC > 0 ? NTC : 1;
    int nbase[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int o = (i * WN + wn) * 32 + l31;
      const int l = lst[o < count ? o : 0];
      nbase[i] = ((l >> 6) * HH + ((l >> 3) & 7)) * HW + (l & 7);
    }
    f32x16 acc[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
    float bvr[16];  // the epilogue's bias values, fetched in one batch under the stage loop (see the split kernel)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
      bvr[r] = (NTC > 0 && co < cout && !out_class) ? bias[co] : 0.0f;
    }

    if constexpr (PRE) {  // `in` = the pre-split operand grid: LDS-DMA stages, two buffers, one barrier per stage
      PreStage<R, HD, HH, HW> ps;
      ps.init(tid, d0, h0, w0, nchunk);
      const conv_i32x4 sg = conv_make_rsrc((const u32x4 *)in + (size_t)b * R3 * nchunk * 4, (unsigned)(R3 * nchunk * 64));
      ps.issue(sg, 0, tile, tid);
      CONV_TL(tid);  // 2: first DMA issued
      const unsigned stage_bytes = 6u * cout_pad * 16u, tap_bytes = (unsigned)nchunk * stage_bytes, plane_bytes = 2u * cout_pad * 16u;
      auto rsw = __builtin_amdgcn_make_buffer_rsrc((void *)wt, 0, 27 * (int)tap_bytes, 0x00020000);
      const unsigned wv = (unsigned)(khalf * cout_pad + co0 + l31) * 16u;
      u32x4 aring[CONV_PRE_AD + 1][2];
      if (NTC > 0) {
#pragma unroll
        for (int t = 0; t < CONV_PRE_AD; ++t)
#pragma unroll
          for (int s = 0; s < 2; ++s) aring[t][s] = conv_wload(rsw, wv, t * tap_bytes + s * plane_bytes);
      }
      auto stage = [&](int k, const u32x4 *cur, u32x4 *nxt) {
        __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0)
        __syncthreads();
        if (k < 4) CONV_TL_AT(tid, 3 + 2 * k);  // stage k released (k < 4)
        if (k + 1 < nchunk) ps.issue(sg, k + 1, nxt, tid);
        if (NTC > 0)
          split_taps_pre<NA, HH, HW, PLANE>(acc, cur, rsw, wv, (unsigned)k * stage_bytes, stage_bytes, tap_bytes, plane_bytes,
                                            k + 1 < nchunk, nbase, khalf, aring);
        if (k < 4) CONV_TL_AT(tid, 4 + 2 * k);  // its taps issued
      };
      for (int k = 0; k < nchunk; k += 2) {
        stage(k, tile, tile2);
        if (k + 1 < nchunk) stage(k + 1, tile2, tile);
      }
    } else {
    stage_load(0);
    for (int ci0 = 0; ci0 < cin; ci0 += CONV_SCK) {
      __syncthreads();
      int nonzero = 0;
#pragma unroll
      for (int c = 0; c < CONV_SCK; ++c) {
        float sc = 1.0f, sh = 0.0f, sub = 0.0f;
        const bool cok = ci0 + c < cin;
        if (XF && cok) {
          sc = in_scale[b * cin + ci0 + c];
          sh = in_shift[b * cin + ci0 + c];
          if (in_sub) sub = in_sub[b * cin + ci0 + c];
        }
#pragma unroll
        for (int j = 0; j < NP; ++j) {
          float x = cok ? stg[c][j] : 0.0f;
          if (XF && cok && soff[j] >= 0) x = xf_apply(x, sc, sh, in_swish) - sub;
          nonzero |= (x != 0.0f);
          stg[c][j] = x;
        }
      }
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        const int e = tid + j * 256;
        if (e < PLANE) {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            u32x4 q[3];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              unsigned p0, p1, p2;
              split_pair<TERMS>(stg[h * 8 + 2 * i][j], stg[h * 8 + 2 * i + 1][j], p0, p1, p2);
              q[0][i] = p0;
              q[1][i] = p1;
              q[2][i] = p2;
            }
#pragma unroll
            for (int s = 0; s < split_planes(TERMS); ++s) tile[(s * 2 + h) * PLANE + e] = q[s];
          }
        }
      }
      const int any = (skip_zero & 1) ? __syncthreads_or(nonzero) : (__syncthreads(), 1);
      if (ci0 + CONV_SCK < cin) {
        int nxt = ci0 + CONV_SCK;
        asm volatile("" : "+s"(nxt));
        stage_load(nxt);
      }
      if (!any || NTC == 0) continue;
      const u32x4 *wchunk = (const u32x4 *)wt + (((size_t)(ci0 / CONV_SCK) * 3) * 2 + khalf) * cout_pad + co0 + l31;
      const size_t wsplit_stride = (size_t)2 * cout_pad, wtap_stride = (size_t)nchunk * 3 * 2 * cout_pad;
      split_taps<NA, HH, HW, PLANE, TERMS>(acc, tile, wchunk, wsplit_stride, wtap_stride, nbase, khalf);
    }
    }  // !PRE
    CONV_TL_AT(tid, 11);  // stage loop done
    // boundary-class constants of a second convolution: the workgroup's [27][32 WM] slice of K[b] through LDS (the operand
    // tile is free now; every wave takes part, also those without a tile) instead of a dependent global load per
    // (row, tile) in the epilogue
    constexpr int NCW = 32 * WM;
    float *kl = (float *)tile;
    if (out_class) {
      __syncthreads();
      const float *kbs = out_class + (size_t)b * 27 * cout;
      for (int e = tid; e < 27 * NCW; e += 256) {
        const int c = e % NCW, co = cob + c;
        kl[e] = co < cout ? kbs[(e / NCW) * cout + co] : 0.0f;
      }
      __syncthreads();
    }
    CONV_TL_AT(tid, 12);  // class constants staged
    if (NTC == 0) return;
    if constexpr (TERMS == SPLIT_F16X3) {
      const float oscale = ((const float *)((const char *)wt + conv_split_trailer_bytes(nchunk, cout_pad)))[1];
#pragma unroll
      for (int n = 0; n < NA; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][r] *= oscale;
    }

    // ---- the active outputs: bias / class constant, 16-byte voxel-major stores, statistics
    int ovox[NA], ocls[NA];
    bool oact[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int o = (i * WN + wn) * 32 + l31;
      oact[i] = o < count;
      ovox[i] = vox_of(lst[oact[i] ? o : 0], ocls[i]);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float vv[NA][4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 4 * g + i;
        const int co = co0 + i + 8 * g + 4 * khalf;
        const bool cok = co < cout;
        const float bv = bvr[r];
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int n = 0; n < NA; ++n) {
          float x = acc[n][r] + bv;
          if (out_class && cok) x += kl[ocls[n] * NCW + 32 * wm + i + 8 * g + 4 * khalf];
          vv[n][i] = x;
          if (oact[n]) {
            s1 += x;
            s2 += x * x;
          }
        }
        s1 = halfwave_sum_to_last(s1);
        s2 = halfwave_sum_to_last(s2);
        if (l31 == 31) {
          wstat[wave][khalf][r][0] = s1;
          wstat[wave][khalf][r][1] = s2;
        }
      }
      const int cq = co0 + 8 * g + 4 * khalf;
#pragma unroll
      for (int n = 0; n < NA; ++n) {
        if (!oact[n]) continue;
        float *q = outb + (size_t)ovox[n] * cout + cq;
        if (cq + 3 < cout && (cout & 3) == 0) *(f32x4 *)q = f32x4{vv[n][0], vv[n][1], vv[n][2], vv[n][3]};
        else
          for (int i = 0; i < 4; ++i)
            if (cq + i < cout) q[i] = vv[n][i];
      }
    }
  };
  if (ntiles > 0) {  // (workgroup-uniform: every wave runs the stage loop, with its own tile count)
    if (nt == 0) run(std::integral_constant<int, 0>{});
    else if (nt == 1) run(std::integral_constant<int, 1>{});
    else if (nt == 2) run(std::integral_constant<int, 2>{});
    else if (nt == 3) run(std::integral_constant<int, 3>{});
    else run(std::integral_constant<int, 4>{});
  }
  __syncthreads();
  CONV_TL_AT(tid, 13);  // active outputs stored

  // ---- the brick's other voxels: their constant, and its exact share of the statistics
  const int ninact = 256 - count;
  for (int e = tid; e < ninact; e += 256) {
    int cls;
    (void)vox_of(lst[count + e], cls);
    atomicAdd(&ncls[cls], 1);
  }
  __syncthreads();
  const int cw = min(32 * WM, cout - cob);  // channels of this workgroup
  const float *kb = out_class ? out_class + (size_t)b * 27 * cout : nullptr;
  // (skip_zero bit 1 = "listed outputs only": the caller reads `out` at listed voxels alone -- a PVConv's second convolution, whose
  //  only reader is the devoxelisation: its corners lie within one voxel of an occupied voxel, inside D1 -- so the constants are
  //  not stored; their statistics below stay exact)
  if (skip_zero & 2) {
  } else if ((cout & 3) == 0) {  // 16 bytes per thread; (voxel, channel quad) advance incrementally, no division in the loop
    const int cw4 = cw >> 2, dq = 256 / cw4, dr = 256 % cw4;
    int vi = tid / cw4, c4 = tid % cw4;
    f32x4 bq = {0.0f, 0.0f, 0.0f, 0.0f};
    if (!kb) bq = *(const f32x4 *)(bias + cob + 4 * c4);
#pragma unroll 4
    for (; vi < ninact; vi += dq) {
      int cls;
      const int vx = vox_of(lst[count + vi], cls);
      *(f32x4 *)(outb + (size_t)vx * cout + cob + 4 * c4) = kb ? *(const f32x4 *)(kb + cls * cout + cob + 4 * c4) : bq;
      if (dr) {
        c4 += dr;
        if (c4 >= cw4) {
          c4 -= cw4;
          ++vi;
        }
        if (!kb) bq = *(const f32x4 *)(bias + cob + 4 * c4);
      }
    }
  } else {
    for (int e = tid; e < ninact * cw; e += 256) {
      const int vi = e / cw, c = e - vi * cw;
      int cls;
      const int vx = vox_of(lst[count + vi], cls);
      outb[(size_t)vx * cout + cob + c] = kb ? kb[cls * cout + cob + c] : bias[cob + c];
    }
  }
  if (stats_part) {
    // slots of the brick: [0, WN) = the wave columns' active sums, WN = the constants' sums, the rest zero
    float *sp = stats_part + (((size_t)b * NBRICK + brick) * 4) * cout * 2;
    if (l31 == 31) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
        if (co < cout) {
          sp[((size_t)wn * cout + co) * 2] = wstat[wave][khalf][r][0];
          sp[((size_t)wn * cout + co) * 2 + 1] = wstat[wave][khalf][r][1];
        }
      }
    }
    if (WN == 4) __syncthreads();
    if (tid < cw) {
      const int co = cob + tid;
      float s1 = 0.0f, s2 = 0.0f;
      if (kb) {
        for (int c = 0; c < 27; ++c) {
          const float x = kb[c * cout + co], n = (float)ncls[c];
          s1 += n * x;
          s2 += n * x * x;
        }
      } else {
        const float x = bias[co];
        s1 = (float)ninact * x;
        s2 = (float)ninact * x * x;
      }
      if (WN == 4) {  // no free slot: on top of wave column 0's sums (written before the barrier above)
        sp[(size_t)co * 2] += s1;
        sp[(size_t)co * 2 + 1] += s2;
      } else {
        sp[((size_t)WN * cout + co) * 2] = s1;
        sp[((size_t)WN * cout + co) * 2 + 1] = s2;
      }
      for (int sl = WN + 1; sl < 4; ++sl) {
        sp[((size_t)sl * cout + co) * 2] = 0.0f;
        sp[((size_t)sl * cout + co) * 2 + 1] = 0.0f;
      }
    }
  }
#ifdef CONV_TIMELINE
  __builtin_amdgcn_s_waitcnt(0x0f70);
  CONV_TL_AT(tid, 14);  // constants + statistics written
#endif
}

// in f32[b,r,r,r,cin] -> out f32[b,r,r,r,cout] (voxel-major), wt = split pack; alist/acount = ONE set of
// p2pb_conv3d_active_lists (D1 for a first convolution, D2 for a second one in far-field form). r in {8,16,32}.
template <int R, int WM, bool XF, int TERMS, bool PRE>
static int conv_compact_go(const ConvArgs &a) {
  const int nchunk = (a.cin + CONV_SCK - 1) / CONV_SCK, cout_pad = (a.cout + 63) / 64 * 64;
  const dim3 grid(conv_bricks(R), (a.cout + 32 * WM - 1) / (32 * WM), a.b);
  hipLaunchKernelGGL((conv3d_k3_compact_kernel<R, WM, XF, TERMS, PRE>), grid, dim3(256), 0, a.s, a.cin, a.cout, nchunk, cout_pad,
                     a.in, (const unsigned short *)a.wt, a.bias, a.out_class, a.in_scale, a.in_shift, a.in_swish, a.in_sub, a.skip_zero,
                     a.alist, a.acount, a.out, a.stats_part);
  return p2pb_launch_status();
}
template <int TERMS>
static int conv_compact_launch(int r, const ConvArgs &a) {
  return for_value<32, 16, 8>(r, [&](auto R) {
    // cout <= 32: one M-tile per workgroup, tiles dealt to four wave columns
    return for_flag(a.cout <= 32, [&](auto WM1) {
      constexpr int RR = decltype(R)::value, WM = decltype(WM1)::value ? 1 : 2;
      if constexpr (TERMS == SPLIT_F16X3) {
        if (a.pre) return conv_compact_go<RR, WM, false, TERMS, true>(a);
      }
      return a.in_scale != nullptr ? conv_compact_go<RR, WM, true, TERMS, false>(a) : conv_compact_go<RR, WM, false, TERMS, false>(a);
    });
  });
}
