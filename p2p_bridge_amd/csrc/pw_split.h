// pw_split.h -- the LDS-tiled split-operand 1x1-convolution GEMM: its epilogue (whose output layouts pw_pp512.h
// shares) and the kernel template. Instantiated and launched by pointwise_split.hip.
#pragma once
#include "pw_common.h"

// Split-operand form of the same GEMM for the matrix-bound layers (wide channel counts): fp32 operands as
// three bf16 terms, six bf16 MFMA products per fp32 product, fp32 accumulate -- the arithmetic of
// conv3d_split.h's split kernel (fp32-faithful: dropped terms < 2^-26 |x*w|), 2.67x fewer matrix cycles.
// At that rate the operands can no longer stream through per-lane global loads (pw_wide_kernel
// would need ~50 B/clk/CU of L1 bandwidth), so this one is the classic LDS-tiled GEMM:
//   workgroup = 4 waves as 2 (M) x 2 (N): 128 output channels x 128 positions, 32 input channels per stage;
//   A: pre-split packed weights, one contiguous 24 KB tile per (stage, 128-channel block), brought into a
//      double-buffered LDS tile by the LDS-DMA path (global_load_lds_dwordx4: no registers, no ds_write --
//      measured, the VGPR->LDS store path is what bounds this kernel: staging off = 141 -> 206 TFLOP/s);
//   B: each wave loads 8 channels x 128 positions (8-byte coalesced loads through scalar row descriptors),
//      applies the folded norm + Swish ONCE per element, splits, and writes 16-byte groups of 8 channels;
//   LDS[kstep][split][khalf][128 rows] x 16 B for both, so every MFMA fragment is one conflict-free
//   ds_read_b128 (positions are stored even/odd de-interleaved: lane j of N-tile n owns position 2j+n,
//   which also makes the epilogue's stores 8 bytes per lane).
// Global loads of the next stage fly during the MFMAs of the current one (register staged).

// Epilogue of the split-operand GEMM kernels for one wave's 64 channels x NB x 64 positions: bias, stores (channel- or
// point-major), GroupNorm partials per 64-position slot, optional {min, max} for the pooling that follows.
// PL (pooling form, compile time): 0 none, 1 global-pool partials (pool_u == 0), 32 neighbourhoods of 32 positions, 2 any other
// neighbourhood size (the per-row ladder)
template <int PL, int WM, int NB>
__device__ __forceinline__ void pws_epilogue(f32x16 (&acc)[2][2 * NB], int b, int bx, int gx, int pblk, int co0,
                                             int wm, int wn, int l31, int khalf, int cout, int P, int nslots,
                                             const float *__restrict__ bias, const float *__restrict__ bias_b,
                                             float *__restrict__ out, float *__restrict__ stats_part,
                                             float *__restrict__ mm_out, int pool_u, int out_pm, const float *sb) {
  // sb: the workgroup's bias (+ per-sample bias) values [64 WM], staged in LDS by the kernel's prologue. Fetched from
  // global memory inside the row loops below they were one L2 round trip each, serialised by the loops' branches (the
  // same finding as in the convolutions' epilogue, conv3d_split.h / tools/exp_conv_timeline.py).
#pragma unroll
  for (int pb = 0; pb < NB; ++pb) {  // the wave's NB blocks of 64 positions (even / odd tiles 2 pb, 2 pb + 1)
  const int p = pblk + 128 * pb + 2 * (wn * 32 + l31);
  const bool pok = p < P;
  if (WM == 2 && out_pm) {  // point-major output f32[b, P, cout]; no statistics in this form (128-channel form only)
    float *ob = out + (size_t)b * P * cout;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int cq = co0 + wm * 64 + m * 32 + 8 * g + 4 * khalf;
        float bv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) bv[i] = sb[cq + i - co0];
        if (pok && cq < cout) {
#pragma unroll
          for (int n = 0; n < 2; ++n) {
            float *q = ob + (size_t)(p + n) * cout + cq;
            const f32x4 v = {acc[m][2 * pb + n][4 * g] + bv[0], acc[m][2 * pb + n][4 * g + 1] + bv[1],
                             acc[m][2 * pb + n][4 * g + 2] + bv[2], acc[m][2 * pb + n][4 * g + 3] + bv[3]};
            if (cq + 3 < cout && (cout & 3) == 0) *(f32x4 *)q = v;
            else
              for (int i = 0; i < 4; ++i)
                if (cq + i < cout) q[i] = v[i];
          }
        }
      }
    continue;
  }
  // ---- epilogue: bias, 8-byte stores, GroupNorm partials per 64-position slot, optional {min, max}.
  // Row index of the reductions: idx = m*16 + r; rowreduce32 leaves row (l31) in lane l31.
  float *outb = out ? out + (size_t)b * cout * P : nullptr;
  const int slot = (bx * NB + pb) * 2 + wn;
  const int pool_g = pool_u ? pool_u / 2 : 32;
  // pass 1: bias (in place), stores, neighbourhood {min, max}
#pragma unroll
  for (int m = 0; m < 2; ++m) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + wm * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
      const bool cok = co < cout;
      const float bv = sb[co - co0];
      acc[m][2 * pb][r] += bv;
      acc[m][2 * pb + 1][r] += bv;
      const f32x2 v = {acc[m][2 * pb][r], acc[m][2 * pb + 1][r]};
      if (cok && pok && outb) *(f32x2 *)(outb + (size_t)co * P + p) = v;
      if constexpr (PL == 2) {
        float mn = pok ? fminf(v[0], v[1]) : INFINITY, mx = pok ? fmaxf(v[0], v[1]) : -INFINITY;
        group_minmax(mn, mx, pool_g);
        if (cok && pok && (pool_g == 32 ? l31 == 31 : (l31 & (pool_g - 1)) == 0)) {
          float *q = mm_out + (((size_t)b * cout + co) * (P / pool_u) + p / pool_u) * 2;
          q[0] = mn;
          q[1] = mx;
        }
      }
    }
  }
  if constexpr (PL == 32) {
    // 32 neighbours = 16 lanes of two positions: the rows' {min, max} through a reduce-scatter network (common.h groupreduce16:
    // rows i + 2 j end in lane j of the group; round 5 -- the per-row ladder above was 12 instructions per row and statistic)
    float tn[32], tx[32];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v0 = acc[m][2 * pb][r], v1 = acc[m][2 * pb + 1][r];
        tn[m * 16 + r] = pok ? vmin_raw(v0, v1) : INFINITY;
        tx[m * 16 + r] = pok ? -vmax_raw(v0, v1) : INFINITY;
      }
    groupreduce16<RowMin>(tn);
    groupreduce16<RowMin>(tx);
    const int j = l31 & 15;  // rows 2 j, 2 j + 1: m = j >> 3, r = 2 (j & 7) + i
    const int cb = co0 + wm * 64 + 32 * (j >> 3) + 2 * (j & 1) + 8 * ((j & 7) >> 1) + 4 * khalf;
    if (pok) {
      const size_t ngrp = (size_t)(P / 32);
      float *q = mm_out + (((size_t)b * cout + cb) * ngrp + p / 32) * 2;
#pragma unroll
      for (int i = 0; i < 2; ++i)
        if (cb + i < cout) *(f32x2 *)(q + (size_t)i * ngrp * 2) = f32x2{tn[i], -tx[i]};
    }
  }
  // this lane's row after the reductions; one 32-value array live at a time (register pressure: the other position
  // block's accumulators are still waiting)
  const int rm = l31 >> 4, rr = l31 & 15;
  const int rco = co0 + wm * 64 + rm * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * khalf;
  auto rowvals = [&](int kind, float (&v)[32]) {  // 0: sum, 1: sum of squares, 2: min, 3: max over the lane's pair
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + wm * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
        const float v0 = acc[m][2 * pb][r], v1 = acc[m][2 * pb + 1][r];
        const bool ok = co < cout && pok;
        v[m * 16 + r] = kind == 0 ? (ok ? v0 + v1 : 0.0f)
                        : kind == 1 ? (ok ? v0 * v0 + v1 * v1 : 0.0f)
                        : kind == 2 ? (pok ? fminf(v0, v1) : INFINITY)
                                    : (pok ? fmaxf(v0, v1) : -INFINITY);
      }
  };
  if (stats_part) {
    float tv[32];
    rowvals(0, tv);
    const float s1 = rowreduce32<RowAdd>(tv);
    rowvals(1, tv);
    const float s2 = rowreduce32<RowAdd>(tv);
    if (rco < cout) {
      float *q = stats_part + (((size_t)b * nslots + slot) * cout + rco) * 2;
      q[0] = s1;
      q[1] = s2;
      if (bx == gx - 1 && pb == NB - 1 && wn == 1)  // slots past the last position block (nslots is a multiple of 4)
        for (int sl = slot + 1; sl < nslots; ++sl) {
          float *z = stats_part + (((size_t)b * nslots + sl) * cout + rco) * 2;
          z[0] = 0.0f;
          z[1] = 0.0f;
        }
    }
  }
  if constexpr (PL == 1) {
    float tv[32];
    rowvals(2, tv);
    const float mn = rowreduce32<RowMin>(tv);
    rowvals(3, tv);
    const float mx = rowreduce32<RowMax>(tv);
    if (rco < cout) {
      float *q = mm_out + ((((size_t)b * gx * NB + bx * NB + pb) * 2 + wn) * cout + rco) * 2;
      q[0] = mn;
      q[1] = mx;
    }
  }
  }  // pb
}

// WM = waves along M: 2 -> 128 output channels per workgroup (4 waves, 48 KB of LDS, three workgroups per CU);
// 4 -> 256 channels (8 waves, 72 KB, two per CU): the activation tile is transformed / split / staged once per 256
// instead of once per 128 channels -- half the VALU + LDS-write work per MFMA -- for the layers whose grid still fills
// the chip (the global embedding's 512 -> 1024 GEMM). A wave's tile, fragments and epilogue are the same in both.
// NB = 128-position blocks per workgroup (1 or 2): with 2 a wave owns 64 channels x 128 positions (2 x 4 accumulator
// tiles), every A fragment feeds four MFMAs instead of two and the weight tile is streamed from L2 once per 256
// positions -- the 128 x 128 tiling moves 10.7 GB through L2 for the 512 -> 1024 x 262144 GEMM (6.4 GB of it the
// pre-split weights, re-read by 2048 position blocks), 256 x 256 moves 5.3 GB.
// TERMS: the arithmetic (common.h, p2pb_set_split_terms) -- SPLIT_F16X3 (default: fp16-pair split, three products, two
// operand planes: the third is neither fetched, written nor read) or SPLIT_BF16X6 (three bf16 terms, six products)
template <bool XF, int PL, int WM, int NB, int TERMS>
#ifndef PWS_WM4_WAVES
#define PWS_WM4_WAVES 4
#endif
__global__ __launch_bounds__(128 * WM, NB == 2 ? 2 : (WM == 2 ? 3 : PWS_WM4_WAVES)) void pw_split_kernel(int cin, int cout, int P, int nslots,
                                                       const float *__restrict__ in, const u32x4 *__restrict__ wp,
                                                       const float *__restrict__ bias,
                                                       const float *__restrict__ bias_b,
                                                       const float *__restrict__ in_scale,
                                                       const float *__restrict__ in_shift, int in_swish,
                                                       float *__restrict__ out, float *__restrict__ stats_part,
                                                       float *__restrict__ mm_out, int pool_u, int out_pm) {
  extern __shared__ u32x4 pws_lds[];  // [A: WM/2 blocks of 128 channels][B: NB blocks of 128 positions][XF: 2 cin floats]
  constexpr int NT = 128 * WM;
  constexpr int BS = 128 * NB;  // 16-byte groups per (kstep, split, khalf) row of the B tile
  u32x4 *lds_b = pws_lds + (WM / 2) * PWS_TILE;
  const u32x4 *lds_a = pws_lds;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform for the scalar descriptors
  const int l31 = lane & 31, khalf = lane >> 5;
  const int wm = wave >> 1, wn = wave & 1;
  // XCD-aware order: workgroup ids go round-robin over the 8 XCDs (each with its own L2), so XCD x takes the x-th
  // contiguous eighth of (sample, position block, channel block) with the channel block fastest: the 2..8 workgroups
  // that stage the SAME activation tile run side by side on one XCD and share it in its L2 (the dispatch order
  // x + gx*(y + gy*z) put them 64 workgroups apart: 2.6x the algorithmic bytes from HBM).
  const int ncoblk = gridDim.y;
  const unsigned lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  const unsigned nblk = gridDim.x * gridDim.y * gridDim.z;
  const unsigned vid = nblk % 8 == 0 ? (lin % 8) * (nblk / 8) + lin / 8 : lin;
  const int bx = (vid / ncoblk) % gridDim.x, by = vid % ncoblk;
  const int b = vid / (ncoblk * gridDim.x);
  const int pblk = bx * (128 * NB), co0 = by * (64 * WM);
  const float *inb = in + (size_t)b * cin * P;
  const bool mact = co0 + wm * 64 < cout;  // this wave's 64 channels exist (wave-uniform)
  __shared__ float pws_bias[64 * WM];  // bias (+ per-sample bias) of the workgroup's channels; published by the stage barriers
  if (tid < 64 * WM) {
    const int co = co0 + tid;
    float v = 0.0f;
    if (co < cout) {
      v = bias ? bias[co] : 0.0f;
      if (bias_b) v += bias_b[(size_t)b * cout + co];
    }
    pws_bias[tid] = v;
  }

  f32x16 acc[2][2 * NB];  // [M-tile][position block * 2 + even/odd tile]
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2 * NB; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.0f;

  // B staging: the stage's 4 channel groups (8 channels each) x NB position blocks are dealt to the 2*WM waves.
  //   WM == 2: wave w owns channel group w for ALL position blocks; lane l positions 2l, 2l+1 of each block;
  //   WM == 4, NB == 2: wave w owns channel group w >> 1 of position block w & 1; lane l positions 2l, 2l+1;
  //   WM == 4, NB == 1: wave w owns channel group w >> 1 for the position half w & 1; lane l position 64 (w & 1) + l.
  constexpr bool ONE = WM == 4 && NB == 1;      // one position per lane (4-byte loads)
  constexpr int NBW = WM == 2 ? NB : 1;         // position blocks staged by one wave
  const int bgrp = WM == 2 ? wave : wave >> 1, bsel = WM == 2 ? 0 : (wave & 1);
  unsigned voff[NBW];
#pragma unroll
  for (int q = 0; q < NBW; ++q) {
    const int pl = ONE ? pblk + 64 * bsel + lane : pblk + 128 * (WM == 2 ? q : bsel) + 2 * lane;
    voff[q] = (unsigned)(pl < P ? pl : P - (ONE ? 1 : 2)) * 4u;  // clamped lanes stage garbage that is never stored
  }
  float braw[NBW][8][ONE ? 1 : 2];  // (plain floats: an f32x2 with a dead half cost the 256-channel form 37 spilled VGPRs)
  auto load_b = [&](int ci0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = min(ci0 + 8 * bgrp + i, cin - 1);  // beyond cin: finite garbage x zero weights
      auto rs = __builtin_amdgcn_make_buffer_rsrc((void *)(inb + (size_t)row * P), 0, P * 4, 0x00020000);
#pragma unroll
      for (int q = 0; q < NBW; ++q) {
        if constexpr (!ONE) {
          const f32x2 v = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rs, voff[q], 0, 0));
          braw[q][i][0] = v[0];
          braw[q][i][1] = v[1];
        } else {
          braw[q][i][0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, voff[q], 0, 0));
        }
      }
    }
  };
  // A tile of stage `chunk` -> LDS, asynchronously: lane i of a wave lands at base + 16*i
  auto dma_a = [&](int chunk) {
    // (the pack is in 128-channel blocks; a 256-channel workgroup takes two consecutive ones)
    const int nblk128 = WM == 2 ? ncoblk : (cout + 127) / 128;
    const u32x4 *src = wp + ((size_t)chunk * nblk128 + by * (WM / 2)) * PWS_TILE;
    u32x4 *dst = pws_lds;
    const bool second_ok = WM == 2 || by * 2 + 1 < nblk128;  // odd block count: the last workgroup has one block only
#pragma unroll
    for (int i = 0; i < 6; ++i)
      if ((second_ok || i * NT + tid < PWS_TILE) && (TERMS == 6 || (((i * NT + wave * 64) % PWS_TILE) / 256) % 3 != 2))
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + i * NT + tid),
                                         (__attribute__((address_space(3))) void *)(dst + i * NT + wave * 64), 16, 0, 0);
  };
  load_b(0);
  // (the folded norm parameters of the operand travel through the scalar cache: an LDS broadcast at the top of the transform
  //  phase costs this kernel 1.2 % -- measured)

  for (int ci0 = 0; ci0 < cin; ci0 += PWS_CK) {
    __syncthreads();  // everyone is done reading the previous stage
    dma_a(ci0 / PWS_CK);  // lands while B is transformed and split below
    // ---- stage B: transform + split
    {
      constexpr int NE = ONE ? 1 : 2;
      if (XF) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int c = min(ci0 + 8 * bgrp + i, cin - 1);
          const float sc = in_scale[b * cin + c], sh = in_shift[b * cin + c];
#pragma unroll
          for (int q = 0; q < NBW; ++q)
#pragma unroll
            for (int e = 0; e < NE; ++e) {
              float v = braw[q][i][e] * sc + sh;
              if (in_swish) v = swishf(v);
              braw[q][i][e] = v;
            }
        }
      }
      const int kstep = bgrp >> 1, kh = bgrp & 1;
#pragma unroll
      for (int q = 0; q < NBW; ++q)
#pragma unroll
        for (int e = 0; e < NE; ++e) {
          u32x4 qq[3];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            unsigned p0, p1, p2;
            split_pair<TERMS>(braw[q][2 * i][e], braw[q][2 * i + 1][e], p0, p1, p2);
            qq[0][i] = p0;
            qq[1][i] = p1;
            qq[2][i] = p2;
          }
          // slot of position p of a 128-block: (p & 1) * 64 + (p >> 1)   (even / odd de-interleaved)
          const int blk = WM == 2 ? q : (NB == 2 ? bsel : 0);
          const int slot = blk * 128 + (ONE ? (lane & 1) * 64 + 32 * bsel + (lane >> 1) : e * 64 + lane);
#pragma unroll
          for (int s = 0; s < split_planes(TERMS); ++s) lds_b[((kstep * 3 + s) * 2 + kh) * BS + slot] = qq[s];
        }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this stage's A tile has landed
    __syncthreads();
    if (ci0 + PWS_CK < cin) load_b(ci0 + PWS_CK);  // next stage's B loads fly during the MFMAs
    if (!mact) continue;
#pragma unroll
    for (int kstep = 0; kstep < 2; ++kstep) {
      u32x4 af[3][2];
#pragma unroll
      for (int s = 0; s < split_planes(TERMS); ++s)
#pragma unroll
        for (int m = 0; m < 2; ++m)
          af[s][m] = lds_a[(wm >> 1) * PWS_TILE + ((kstep * 3 + s) * 2 + khalf) * 128 + (wm & 1) * 64 + m * 32 + l31];
      constexpr int PA[6] = {2, 1, 0, 1, 0, 0}, PB[6] = {0, 1, 2, 0, 1, 0};  // small terms first
      // the B fragments of one position block (2 tiles x 3 terms) at a time: 24 registers live instead of 24 NB
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        u32x4 bf[3][2];
#pragma unroll
        for (int s = 0; s < split_planes(TERMS); ++s)
#pragma unroll
          for (int n = 0; n < 2; ++n)
            bf[s][n] = lds_b[((kstep * 3 + s) * 2 + khalf) * BS + nb * 128 + n * 64 + wn * 32 + l31];
#pragma unroll
        for (int t = (TERMS == 6 ? 0 : 3); t < 6; ++t)
#pragma unroll
          for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n)
              if (X2W_KEEP_LOW_WEIGHT_PRODUCT || TERMS != SPLIT_F16X3 || PA[t] != 1)
                acc[m][2 * nb + n] = split_mfma<TERMS>(af[PA[t]][m], bf[PB[t]][n], acc[m][2 * nb + n]);
      }
    }
  }
  if (!mact) return;
  {
    if constexpr (TERMS == SPLIT_F16X3) {  // 1 / (S_x S_w), a power of two, stored behind the pack
      const int nblk128 = WM == 2 ? ncoblk : (cout + 127) / 128;
      const float oscale = ((const float *)(wp + (size_t)((cin + PWS_CK - 1) / PWS_CK) * nblk128 * PWS_TILE))[1];
  #pragma unroll
      for (int m = 0; m < 2; ++m)
  #pragma unroll
        for (int n = 0; n < 2 * NB; ++n)
  #pragma unroll
          for (int r = 0; r < 16; ++r) acc[m][n][r] *= oscale;
    }
  pws_epilogue<PL, WM, NB>(acc, b, bx, (int)gridDim.x, pblk, co0, wm, wn, l31, khalf, cout, P, nslots, bias, bias_b, out,
                             stats_part, mm_out, pool_u, out_pm, pws_bias);
  }
}
