// pw_wide.h -- the register-tiled 1x1-convolution kernel and its one launch site. Instantiated by pointwise_fp32.hip (TERMS = 0,
// the fp32 pack) and pointwise_f16.hip (TERMS = SPLIT_F16X3, the split pack; the gathered operand).
#pragma once
#include "pw_common.h"

// Wide tile (the default whenever rows are 16-byte aligned: npos % 4 == 0): a wave owns 32*MT output
// channels x 128 positions. Lane j of a half-wave holds positions 4j..4j+3 of one input channel in ONE
// 16-byte buffer load; MFMA column tile s is the position set {4j+s}, so the four tiles of a lane are the
// four components of that load and the epilogue stores 16 bytes per lane as well: 4x fewer memory
// instructions per MFMA than the one-position-per-lane kernel above, and the channel rows are addressed
// through scalar descriptors (no per-lane 64-bit address arithmetic). Chunks of 8 input channels are
// double-buffered in registers: 184 VGPRs, 2 waves/SIMD. Measured on 512->1024 x 262144 positions:
// 133 TFLOP/s without / 125 with the statistics epilogue (the MFMA-only loop of the same shape: 133),
// vs 86 for the narrow kernel.
// Ragged channel counts need no predicates: a row pair starting at ci >= cin is clamped to the last row
// (the packed weights are zero there, so the finite garbage contributes exactly 0), and the descriptor's
// num_records ends at the sample's last row, so the odd half of a half-valid pair reads hardware zeros.
#define PWW_CK 8

// POOL: additionally emit {min, max} of the raw output over groups of pool_g lanes (= 4*pool_g consecutive
// positions: a set-abstraction neighbourhood) or, pool_g == 32, over the wave's 128 positions (global max-pool
// partials); `out` may then be NULL. Swish (like every activation the network uses) is quasi-convex, so
//   max_p act(scale*x_p + shift) = max(act(scale*min_p x_p + shift), act(scale*max_p x_p + shift)),
// and the pooled tensor is produced by p2pb_minmax_act from 2/U-th of the data without the layer's
// output ever being written or re-read.
// TERMS == SPLIT_F16X3: the same tiling, operand path and epilogue with the products on the 16-bit matrix pipe (fp16-pair
// split, three MFMAs of K = 16 instead of eight exact-fp32 ones of K = 2: 5.3x fewer matrix cycles -- the exact-fp32
// MFMAs were HALF the time of the set-abstraction neighbourhood layers; round 2 measurement, docs/history). `wp` is then the split
// pack of pw_split_kernel (fragments read straight from L1 / L2, output scale in its trailer); 16 input channels per step:
// lane (l31, khalf) loads rows 8 khalf .. + 7 of the step for its four positions, transforms and splits them once.
// GATHER (f16x3 form only): the operand is the GROUPED tensor of a set abstraction without ever being built --
// operand[ci, p] = zt[idx[p]][ci] - cxt[p / gu][ci] from point-major rows zt f32[b, gn, cin] (`in`), cxt f32[b, P / gu, cin]
// and the neighbour lists idx i32[b, P] (csrc/neighbors.hip group_sub_kernel's arithmetic, bit for bit): a lane fetches the
// 8-channel piece of its four positions' rows (32 contiguous bytes each, L2-resident: the ungrouped tensor is 1 MB per
// sample) instead of four channel-major quads of a 268 MB tensor that group_sub wrote and this kernel read back.
// PG (pooling form, compile time): 0 none, 32 global-pool partials, 8 neighbourhoods of 8 lanes, 1 any other width (pool_g)
template <int MT, bool XF, bool STATS, int PG, int TERMS = 0, bool GATHER = false>
__global__ __launch_bounds__(256, 2) void pw_wide_kernel(int cin, int cout, int cout_pad, int P, int nslots,
                                                      const float *__restrict__ in, const float *__restrict__ wp,
                                                      const float *__restrict__ bias,
                                                      const float *__restrict__ bias_b,
                                                      const float *__restrict__ in_scale,
                                                      const float *__restrict__ in_shift, int in_swish,
                                                      float *__restrict__ out, float *__restrict__ stats_part,
                                                      float *__restrict__ mm_out, int pool_g, int out_pm,
                                                      PwGather gat) {
  static_assert(!GATHER || TERMS == SPLIT_F16X3, "the gathered operand exists in the f16x3 form");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, khalf = lane >> 5;
  const int co0 = blockIdx.y * (32 * MT), b = blockIdx.z;
  const int p = blockIdx.x * 512 + wave * 128 + l31 * 4;
  const bool pok = p < P;
  const int pc = pok ? p : P - 4;  // clamped lanes multiply garbage that is never stored
  const float *inb = in + (size_t)b * cin * P;
  // bias (+ per-sample bias) of the workgroup's channels through LDS: fetched from global memory inside the epilogue's row
  // loops they were one serialised L2 round trip per row (conv3d_split.h, tools/exp_conv_timeline.py)
  __shared__ float pww_bias[32 * MT];
  if (tid < 32 * MT) {
    const int co = co0 + tid;
    float v = 0.0f;
    if (co < cout) {
      v = bias ? bias[co] : 0.0f;
      if (bias_b) v += bias_b[(size_t)b * cout + co];
    }
    pww_bias[tid] = v;
  }
  __syncthreads();

  f32x16 acc[MT][4];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][s][r] = 0.0f;

  if constexpr (TERMS == SPLIT_F16X3) {
    constexpr int PWS_TILE_ = 2 * 3 * 2 * 128;  // (PWS_TILE of the split pack, pw_common.h)
    const u32x4 *wp4 = (const u32x4 *)wp;
    const int ncoblk128 = (cout + 127) / 128, nchunk32 = (cin + 31) / 32;
    const u32x4 *wtile = wp4 + (size_t)(co0 >> 7) * PWS_TILE_ + khalf * 128 + (co0 & 127) + l31;
    const unsigned voffh = (unsigned)(khalf * 8 * P + pc) * 4u, rowb = (unsigned)P * 4u;
    f32x4 braw[8];
    u32x4 a_nx[MT][2];
    // GATHER: this lane's four neighbour rows and its centre row (positions pc .. pc + 3 share a centre: gu % 4 == 0)
    int gid[4] = {0, 0, 0, 0};
    const float *grow[4] = {nullptr, nullptr, nullptr, nullptr}, *gcen = nullptr;
    if constexpr (GATHER) {
      const int *ip = gat.idx + (size_t)b * P + pc;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        gid[t] = ip[t];
        grow[t] = in + ((size_t)b * gat.gn + gid[t]) * cin;
      }
      if (gat.cxt) gcen = gat.cxt + ((size_t)b * (P / gat.gu) + pc / gat.gu) * cin;
    }
    auto load_bh = [&](int ci0) {
      if constexpr (GATHER) {
        // rows are point-major: channels ci0 + 8 khalf .. + 7 of position t are 32 contiguous bytes (cin % 8 == 0)
        const int cb = ci0 + 8 * khalf;
        f32x4 cen[2] = {{0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}};
        if (gcen && cb < cin) {
          cen[0] = *(const f32x4 *)(gcen + cb);
          cen[1] = *(const f32x4 *)(gcen + cb + 4);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          f32x4 r0 = {0.0f, 0.0f, 0.0f, 0.0f}, r1 = r0;
          if (cb < cin) {
            r0 = *(const f32x4 *)(grow[t] + cb);
            r1 = *(const f32x4 *)(grow[t] + cb + 4);
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            braw[i][t] = gcen ? r0[i] - cen[0][i] : r0[i];          // (group_sub_kernel: v = z; v -= cx)
            braw[4 + i][t] = gcen ? r1[i] - cen[1][i] : r1[i];
          }
        }
        return;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int row = min(ci0 + i, cin - 1);  // rows at or beyond cin: zero records -> hardware zeros (x zero weights)
        const int rec = ci0 + i < cin ? (int)((unsigned)(cin - row) * rowb) : 0;
        auto rs = __builtin_amdgcn_make_buffer_rsrc((void *)(inb + (size_t)row * P), 0, rec, 0x00020000);
        braw[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voffh, 0, 0));
      }
    };
    auto load_ah = [&](int ci0) {
      const u32x4 *t = wtile + (size_t)(ci0 >> 5) * ncoblk128 * PWS_TILE_ + ((ci0 >> 4) & 1) * (3 * 2 * 128);
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) a_nx[m][pl] = t[pl * 256 + m * 32];
    };
    load_bh(0);
    load_ah(0);
    for (int ci0 = 0; ci0 < cin; ci0 += 16) {
      if (XF) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int ca = b * cin + min(ci0 + i, cin - 1), cb = b * cin + min(ci0 + 8 + i, cin - 1);
          const float sca = in_scale[ca], scb = in_scale[cb], sha = in_shift[ca], shb = in_shift[cb];
          const float sc = khalf ? scb : sca, sh = khalf ? shb : sha;
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            float v = braw[i][t] * sc + sh;
            if (in_swish) v = swishf(v);
            braw[i][t] = v;
          }
        }
      }
      u32x4 pl0[4], pl1[4];
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          unsigned p0, p1, p2;
          split_pair<SPLIT_F16X3>(braw[2 * i][t], braw[2 * i + 1][t], p0, p1, p2);
          pl0[t][i] = p0;
          pl1[t][i] = p1;
        }
      u32x4 a_cu[MT][2];
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) a_cu[m][pl] = a_nx[m][pl];
      if (ci0 + 16 < cin) {  // the next step's loads fly during the MFMAs
        load_ah(ci0 + 16);
        load_bh(ci0 + 16);
      }
      // term by term over all the accumulators (a1 b0, a0 b1, a0 b0 per accumulator as before: same bits): the three MFMAs
      // that update one accumulator are 4 MT instructions apart instead of back to back
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if (X2W_KEEP_LOW_WEIGHT_PRODUCT) acc[m][t] = split_mfma<SPLIT_F16X3>(a_cu[m][1], pl0[t], acc[m][t]);
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[m][t] = split_mfma<SPLIT_F16X3>(a_cu[m][0], pl1[t], acc[m][t]);
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[m][t] = split_mfma<SPLIT_F16X3>(a_cu[m][0], pl0[t], acc[m][t]);
    }
    const float oscale = ((const float *)(wp4 + (size_t)nchunk32 * ncoblk128 * PWS_TILE_))[1];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][t][r] *= oscale;
  }
  const unsigned voff = (unsigned)(khalf * P + pc) * 4u;
  const unsigned rowbytes = (unsigned)P * 4u;
  f32x4 bcur[PWW_CK / 2], bnxt[PWW_CK / 2];
  auto load_b = [&](int ci0, f32x4(&dst)[PWW_CK / 2]) {
#pragma unroll
    for (int kk = 0; kk < PWW_CK / 2; ++kk) {
      const int row0 = min(ci0 + 2 * kk, cin - 1);
      auto rs = __builtin_amdgcn_make_buffer_rsrc((void *)(inb + (size_t)row0 * P), 0,
                                                  (int)(min(cin - row0, 2) * rowbytes), 0x00020000);
      dst[kk] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, 0, 0));
    }
  };
  const float *wbase = wp + ((size_t)khalf * cout_pad + co0 + l31) * 4;
  const size_t wchunk_stride = (size_t)2 * cout_pad * 4;
  f32x4 a_cur[MT], a_nxt[MT];
  auto load_a = [&](int chunk, f32x4(&dst)[MT]) {
#pragma unroll
    for (int m = 0; m < MT; ++m) dst[m] = *(const f32x4 *)(wbase + (size_t)chunk * wchunk_stride + (size_t)m * 32 * 4);
  };
  if constexpr (TERMS == 0) {
    load_b(0, bnxt);
    load_a(0, a_nxt);
  }

  for (int ci0 = 0; TERMS == 0 && ci0 < cin; ci0 += PWW_CK) {
    // rotate (the vmcnt wait lands here), request the next chunk, then multiply the current one
#pragma unroll
    for (int kk = 0; kk < PWW_CK / 2; ++kk) bcur[kk] = bnxt[kk];
#pragma unroll
    for (int m = 0; m < MT; ++m) a_cur[m] = a_nxt[m];
    if (ci0 + PWW_CK < cin) {
      load_a((ci0 >> 3) + 1, a_nxt);
      load_b(ci0 + PWW_CK, bnxt);
    }
    if (XF) {
#pragma unroll
      for (int kk = 0; kk < PWW_CK / 2; ++kk) {
        // wave-uniform indices: the folded norm parameters travel through the scalar cache
        const int ca = b * cin + min(ci0 + 2 * kk, cin - 1), cb = b * cin + min(ci0 + 2 * kk + 1, cin - 1);
        const float sca = in_scale[ca], scb = in_scale[cb], sha = in_shift[ca], shb = in_shift[cb];
        const float sc = khalf ? scb : sca, sh = khalf ? shb : sha;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          float v = bcur[kk][s] * sc + sh;
          if (in_swish) v = swishf(v);
          bcur[kk][s] = v;
        }
      }
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int s = 0; s < 4; ++s)
          acc[m][s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[m][kk], bcur[kk][s], acc[m][s], 0, 0, 0);
  }

  if (out_pm) {  // point-major output f32[b, P, cout] (the consumer gathers whole rows); no statistics in this form
    float *ob = out + (size_t)b * P * cout;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int cq = co0 + m * 32 + 8 * g + 4 * khalf;
        float bv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) bv[i] = pww_bias[cq + i - co0];
        if (pok && cq < cout) {
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            float *q = ob + (size_t)(p + s) * cout + cq;
            const f32x4 v = {acc[m][s][4 * g] + bv[0], acc[m][s][4 * g + 1] + bv[1], acc[m][s][4 * g + 2] + bv[2],
                             acc[m][s][4 * g + 3] + bv[3]};
            if (cq + 3 < cout && (cout & 3) == 0) *(f32x4 *)q = v;
            else
              for (int i = 0; i < 4; ++i)
                if (cq + i < cout) q[i] = v[i];
          }
        }
      }
    return;
  }
  // ---- epilogue (round 5). The first form reduced every one of the 32 MT rows on its own -- five DPP steps per statistic, a
  // runtime-width min / max ladder, and a predicated store with its own 64-bit address for every row: ~9000 of the POOL kernel's
  // 11900 instructions ran ONCE per wave, and with two 16-channel steps per wave (the 32 -> 64 set-abstraction layer) the launch
  // was bound by issuing them (271 us for 8.6 GFLOP; profiles/r05_overlap.txt). Now: bias in place + stores, then the rows'
  // reductions as reduce-scatter networks (common.h rowreduce32: lane l31 ends with the total of row l31; groupreduce8 below:
  // neighbourhoods of 8 lanes) and ONE store per lane. Sums: the lane's four positions (v0 + v1) + (v2 + v3) as before, then the
  // network's fixed tree instead of the 5-step ladder (the partials change in their last bit, deterministically).
  float *outb = out ? out + (size_t)b * cout * P : nullptr;
  const int slot = (blockIdx.x * 4 + wave) * 2;  // this wave fills slot `slot` with its 128-position sums and zeroes slot + 1
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
      const float bv = pww_bias[co - co0];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[m][t][r] += bv;
      if (co < cout && pok && outb)
        *(f32x4 *)(outb + (size_t)co * P + p) = f32x4{acc[m][0][r], acc[m][1][r], acc[m][2][r], acc[m][3][r]};
    }
  // the row whose total this lane holds after rowreduce32 (MT == 1: rows 0..15 twice, two statistics packed into one network)
  const int rrow = MT == 2 ? l31 : (l31 & 15);
  const int rco = co0 + (rrow >> 4) * 32 + (rrow & 3) + 8 * ((rrow & 15) >> 2) + 4 * khalf;
  auto rowval = [&](int kind, int m, int r) -> float {  // 0: sum, 1: sum of squares, 2: min, 3: -max over the lane's 4 positions
    const int co = co0 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
    const float v0 = acc[m][0][r], v1 = acc[m][1][r], v2 = acc[m][2][r], v3 = acc[m][3][r];
    const bool ok = co < cout && pok;
    if (kind == 0) return ok ? (v0 + v1) + (v2 + v3) : 0.0f;
    if (kind == 1) return ok ? (v0 * v0 + v1 * v1) + (v2 * v2 + v3 * v3) : 0.0f;
    if (kind == 2) return pok ? vmin_raw(vmin_raw(v0, v1), vmin_raw(v2, v3)) : INFINITY;
    return pok ? -vmax_raw(vmax_raw(v0, v1), vmax_raw(v2, v3)) : INFINITY;
  };
  if (STATS) {
    float s1, s2;
    float tv[32];
    if constexpr (MT == 2) {
#pragma unroll
      for (int i = 0; i < 32; ++i) tv[i] = rowval(0, i >> 4, i & 15);
      s1 = rowreduce32<RowAdd>(tv);
#pragma unroll
      for (int i = 0; i < 32; ++i) tv[i] = rowval(1, i >> 4, i & 15);
      s2 = rowreduce32<RowAdd>(tv);
    } else {
#pragma unroll
      for (int i = 0; i < 32; ++i) tv[i] = rowval(i >> 4, 0, i & 15);
      s1 = s2 = rowreduce32<RowAdd>(tv);  // lanes 0..15: sums, lanes 16..31: sums of squares, of rows l31 & 15
    }
    if (rco < cout) {
      if (slot < nslots) {
        float *q = stats_part + (((size_t)b * nslots + slot) * cout + rco) * 2;
        if constexpr (MT == 2) *(f32x2 *)q = f32x2{s1, s2};
        else q[l31 >> 4] = s1;
      }
      if (slot + 1 < nslots) {
        float *q = stats_part + (((size_t)b * nslots + slot + 1) * cout + rco) * 2;
        if constexpr (MT == 2) *(f32x2 *)q = f32x2{0.0f, 0.0f};
        else q[l31 >> 4] = 0.0f;
      }
    }
  }
  if constexpr (PG != 0) {
    float tv[32];
    if constexpr (PG == 32) {  // global max-pool partials: {min, max} over the wave's 128 positions
      float mn, mx;
      if constexpr (MT == 2) {
#pragma unroll
        for (int i = 0; i < 32; ++i) tv[i] = rowval(2, i >> 4, i & 15);
        mn = rowreduce32<RowMin>(tv);
#pragma unroll
        for (int i = 0; i < 32; ++i) tv[i] = rowval(3, i >> 4, i & 15);
        mx = -rowreduce32<RowMin>(tv);
      } else {
#pragma unroll
        for (int i = 0; i < 32; ++i) tv[i] = rowval(2 + (i >> 4), 0, i & 15);
        mn = rowreduce32<RowMin>(tv);  // lanes 0..15: min, lanes 16..31: -max, of rows l31 & 15
        mx = -mn;
      }
      if (rco < cout) {
        float *q = mm_out + ((((size_t)b * gridDim.x + blockIdx.x) * 4 + wave) * cout + rco) * 2;
        if constexpr (MT == 2) *(f32x2 *)q = f32x2{mn, mx};
        else q[l31 >> 4] = (l31 >> 4) ? mx : mn;
      }
    } else if constexpr (PG == 8) {  // neighbourhoods of 32 positions = aligned groups of 8 lanes (the bench's set abstractions)
      // groupreduce8 leaves rows i + 4 j (i = 0..3, j = lane & 7) of the lane's group in v[i]
      const int j = l31 & 7;
      const size_t ngrp = (size_t)(P / 32);
      if constexpr (MT == 2) {
        float tx[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) {
          tv[i] = rowval(2, i >> 4, i & 15);
          tx[i] = rowval(3, i >> 4, i & 15);
        }
        groupreduce8<RowMin>(tv);
        groupreduce8<RowMin>(tx);
        const int cb = co0 + 32 * (j >> 2) + 8 * (j & 3) + 4 * khalf;  // rows i + 4 j: channels cb + i
        if (pok) {
          float *q = mm_out + (((size_t)b * cout + cb) * ngrp + p / 32) * 2;
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (cb + i < cout) *(f32x2 *)(q + (size_t)i * ngrp * 2) = f32x2{tv[i], -tx[i]};
        }
      } else {
#pragma unroll
        for (int i = 0; i < 32; ++i) tv[i] = rowval(2 + (i >> 4), 0, i & 15);
        groupreduce8<RowMin>(tv);  // j < 4: min of rows i + 4 j, j >= 4: -max of rows i + 4 (j - 4)
        const int cb = co0 + 8 * (j & 3) + 4 * khalf;
        if (pok) {
          float *q = mm_out + (((size_t)b * cout + cb) * ngrp + p / 32) * 2 + (j >> 2);
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (cb + i < cout) q[(size_t)i * ngrp * 2] = (j >> 2) ? -tv[i] : tv[i];
        }
      }
    } else {  // other neighbourhood sizes: the per-row ladder
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int co = co0 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
          float mn = rowval(2, m, r), mx = -rowval(3, m, r);
          group_minmax(mn, mx, pool_g);
          if (co < cout && (l31 & (pool_g - 1)) == 0 && pok) {
            const int u = 4 * pool_g;
            float *q = mm_out + (((size_t)b * cout + co) * (P / u) + p / u) * 2;
            q[0] = mn;
            q[1] = mx;
          }
        }
    }
  }
}

// The launch site. The pooling width reaches the kernel in lanes of four positions (0 without a pooling epilogue).
template <int MT, bool XF, bool STATS, int PG, int TERMS, bool GATHER>
static int pw_wide_go(const PwArgs &a, const PwGather &gat) {
  const dim3 grid((a.P + 511) / 512, (a.cout + 32 * MT - 1) / (32 * MT), a.b);
  hipLaunchKernelGGL((pw_wide_kernel<MT, XF, STATS, PG, TERMS, GATHER>), grid, dim3(256), 0, a.s, a.cin, a.cout, pw_cout_pad(a.cout),
                     a.P, pw_nslots(a.P), a.in, (const float *)a.wp, a.bias, a.bias_b, a.in_scale, a.in_shift, a.in_swish, a.out,
                     a.stats_part, a.minmax, a.minmax ? pool_lanes(a.pool_u) : 0, a.out_pm, gat);
  return p2pb_launch_status();
}

// The plain (not gathered) forms of one arithmetic: MT x operand transform x epilogue. The epilogues that exist (EP): -1 none,
// 0 statistics, else statistics + the pooling form PG
template <int TERMS>
static int pw_wide_form(const PwArgs &a) {
  const int pool_g = pool_lanes(a.pool_u);
  const int ep = a.minmax ? (pool_g == 8 || pool_g == 32 ? pool_g : 1) : a.stats_part ? 0 : -1;
  return pw_for_mt(a.cout, [&](auto MT) {
    return for_flag(a.in_scale != nullptr, [&](auto XF) {
      return for_value<-1, 0, 1, 8, 32>(ep, [&](auto EP) {
        return pw_wide_go<MT(), XF(), EP() >= 0, (EP() > 0 ? EP() : 0), TERMS, false>(a, PwGather());
      });
    });
  });
}
