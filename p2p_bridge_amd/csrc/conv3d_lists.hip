// conv3d_lists.hip -- where the sparse forms of the voxel convolution (conv3d_common.h) get their work lists from the voxel
// occupancy: active / inactive bricks for the list-driven dense kernels (p2pb_conv3d_brick_lists), per-brick voxel lists for the
// compact kernel (p2pb_conv3d_active_lists), and the kernel that writes the known constants of the inactive bricks.
//
// Brick activity from the voxel occupancy (cnt of avg_voxelize), compact 4x8x8 bricks:
//   first conv : a brick has non-zero input in its halo  <=> an occupied voxel within brick +- 1
//   second conv: its operand differs from the far-field constant only inside dil(occupied, 1), so a brick
//                has work <=> an occupied voxel within brick +- 2
// Output: four compacted lists of (sample*NBRICK + brick): active/inactive for each conv, and their counts.
#include "conv3d_common.h"

template <int R>
__global__ __launch_bounds__(256) void brick_flags_kernel(const int *__restrict__ cnt, unsigned char *__restrict__ flags) {
  constexpr int TD = 4, TH = 8, TW = 8, BH = R / TH, BW = R / TW, NBRICK = (R / TD) * BH * BW;
  __shared__ int f1, f2;
  const int b = blockIdx.y, bk = blockIdx.x;
  const int d0 = (bk / (BH * BW)) * TD, h0 = ((bk / BW) % BH) * TH, w0 = (bk % BW) * TW;
  if (threadIdx.x == 0) f1 = f2 = 0;
  __syncthreads();
  constexpr int ED = TD + 4, EH = TH + 4, EW = TW + 4;
  int a1 = 0, a2 = 0;
  for (int e = threadIdx.x; e < ED * EH * EW; e += 256) {
    const int dz = e / (EH * EW), hy = (e / EW) % EH, wx = e % EW;
    const int d = d0 - 2 + dz, h = h0 - 2 + hy, w = w0 - 2 + wx;
    if ((unsigned)d < (unsigned)R && (unsigned)h < (unsigned)R && (unsigned)w < (unsigned)R) {
      if (cnt[(size_t)b * R * R * R + (d * R + h) * R + w] > 0) {
        a2 = 1;
        if (dz >= 1 && dz <= TD + 2 && hy >= 1 && hy <= TH + 2 && wx >= 1 && wx <= TW + 2) a1 = 1;
      }
    }
  }
  if (a1) f1 = 1;  // benign race: every writer stores 1
  if (a2) f2 = 1;
  __syncthreads();
  if (threadIdx.x == 0) {
    flags[((size_t)b * NBRICK + bk) * 2 + 0] = (unsigned char)f1;
    flags[((size_t)b * NBRICK + bk) * 2 + 1] = (unsigned char)f2;
  }
}

// single workgroup: compaction of up to 1024*PER entries into active/inactive lists for both convolutions
static __global__ __launch_bounds__(1024) void brick_compact_kernel(int total, const unsigned char *__restrict__ flags,
                                                            int *__restrict__ lists, int *__restrict__ counts) {
  __shared__ int wsum[16];
  const int t = threadIdx.x;
  const int per = (total + 1023) / 1024;
  const int beg = t * per, end = min(beg + per, total);
  for (int which = 0; which < 2; ++which) {
    int k = 0;
    for (int e = beg; e < end; ++e) k += flags[(size_t)e * 2 + which];
    // inclusive wave scan + cross-wave offsets
    int inc = k;
    for (int d = 1; d < 64; d <<= 1) {
      const int y = __shfl_up(inc, d);
      if ((t & 63) >= d) inc += y;
    }
    __syncthreads();
    if ((t & 63) == 63) wsum[t >> 6] = inc;
    __syncthreads();
    int base = 0, all = 0;
    for (int w = 0; w < 16; ++w) {
      if (w < (t >> 6)) base += wsum[w];
      all += wsum[w];
    }
    int apos = base + inc - k;      // active entries before this thread's range
    int ipos = beg - apos;          // inactive entries before it
    int *act = lists + (size_t)(2 * which) * total, *ina = lists + (size_t)(2 * which + 1) * total;
    for (int e = beg; e < end; ++e) {
      if (flags[(size_t)e * 2 + which]) act[apos++] = e;
      else ina[ipos++] = e;
    }
    if (t == 0) {
      counts[2 * which] = all;
      counts[2 * which + 1] = total - all;
    }
  }
}

// lists i32[4][b*NBRICK] = {active conv0, inactive conv0, active conv1, inactive conv1}, counts i32[4];
// flags_ws: b*NBRICK*2 bytes of scratch. r in {16, 32}.
extern "C" int p2pb_conv3d_brick_lists(int b, int r, const int *cnt, unsigned char *flags_ws, int *lists, int *counts,
                                       void *stream) {
  if (b <= 0 || (r != 16 && r != 32)) return P2PB_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int nb = conv_bricks(r);
  if (r == 32) hipLaunchKernelGGL(brick_flags_kernel<32>, dim3(nb, b), dim3(256), 0, s, cnt, flags_ws);
  else hipLaunchKernelGGL(brick_flags_kernel<16>, dim3(nb, b), dim3(256), 0, s, cnt, flags_ws);
  hipLaunchKernelGGL(brick_compact_kernel, dim3(1), dim3(1024), 0, s, nb * b, flags_ws, lists, counts);
  return p2pb_launch_status();
}

// per (sample, brick): local ids (ld*8 + lh)*8 + lw of the voxels in D1 (which = 0) / D2 (which = 1), in an
// LDS-conflict-avoiding order (below), followed by the ids NOT in the set; counts[which][b][brick] = size of the set.
template <int R>
__global__ __launch_bounds__(256) void active_lists_kernel(const int *__restrict__ cnt, unsigned char *__restrict__ lists,
                                                           int *__restrict__ counts, int nb) {
  constexpr int TD = 4, TH = 8, TW = 8, BH = R / TH, BW = R / TW, NBRICK = (R / TD) * BH * BW;
  constexpr int ED = TD + 4, EH = TH + 4, EW = TW + 4;  // occupancy, brick +- 2
  constexpr int FD = TD + 2, FH = TH + 2, FW = TW + 2;  // D1, brick +- 1
  __shared__ unsigned char occ[ED * EH * EW], d1[FD * FH * FW];
  __shared__ int wcount[2][4], wbc[2][4][16];
  const int b = blockIdx.y, bk = blockIdx.x, t = threadIdx.x;
  const int d0 = (bk / (BH * BW)) * TD, h0 = ((bk / BW) % BH) * TH, w0 = (bk % BW) * TW;
  for (int e = t; e < ED * EH * EW; e += 256) {
    const int d = d0 - 2 + e / (EH * EW), h = h0 - 2 + (e / EW) % EH, w = w0 - 2 + e % EW;
    const bool in = (unsigned)d < (unsigned)R && (unsigned)h < (unsigned)R && (unsigned)w < (unsigned)R;
    occ[e] = in && cnt[(size_t)b * R * R * R + (d * R + h) * R + w] > 0;
  }
  __syncthreads();
  for (int e = t; e < FD * FH * FW; e += 256) {
    const int z = e / (FH * FW), y = (e / FW) % FH, x = e % FW;  // voxel (d0-1+z, ...): occ index offset by +1
    int any = 0;
    for (int k = 0; k < 27; ++k) any |= occ[((z + k / 9) * EH + (y + (k / 3) % 3)) * EW + x + k % 3];
    // a voxel outside the grid is never an input: its D1 flag must not leak into D2 of its neighbours
    const int d = d0 - 1 + z, h = h0 - 1 + y, w = w0 - 1 + x;
    const bool in = (unsigned)d < (unsigned)R && (unsigned)h < (unsigned)R && (unsigned)w < (unsigned)R;
    d1[e] = in ? any : 0;
  }
  __syncthreads();
  const int ld = t / 64, lh = (t / 8) % 8, lw = t % 8;
  int f[2];
  f[0] = d1[((ld + 1) * FH + lh + 1) * FW + lw + 1];
  f[1] = 0;
  for (int k = 0; k < 27; ++k) f[1] |= d1[((ld + k / 9) * FH + lh + (k / 3) % 3) * FW + lw + k % 3];
  const int lane = t & 63, wave = t >> 6;
  // Order of the active ids: the convolution reads the B fragment of a column tile with one ds_read_b128 per lane at
  // "halo slot of my voxel + tap offset", served in groups of 16 lanes ({0-3,12-15,20-27}, {4-11,16-19,28-31} of a
  // half-wave), one cycle per group when the 16 slots differ mod 16. Sorting the ids by (rank inside their residue
  // class, residue) makes any 16 consecutive ones (nearly) distinct mod 16; full tiles then deal the first / second
  // 16 of their 32 ids to the lanes of the first / second service group. Ascending ids would be 2-3-way conflicted.
  const int rho = ((ld * (TH + 2) + lh) * (TW + 2) + lw) & 15;
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    int rk = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const unsigned long long m = __ballot(f[w] && rho == q);
      if (rho == q) rk = mbcnt(m);
      if (lane == 0) wbc[w][wave][q] = __popcll(m);
    }
    f[w] |= rk << 1;  // bit 0: active, the rest: rank among the wave's active ids of the same residue
  }
  __syncthreads();
  constexpr int POS[32] = {0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27,
                           4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31};
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    const int act = f[w] & 1;
    int rk = f[w] >> 1, total = 0, below = 0, inact_before = 0;
    for (int q = 0; q < wave; ++q) rk += wbc[w][q][rho];
    for (int q = 0; q < 16; ++q) {
      int c = 0;
      for (int v = 0; v < 4; ++v) c += wbc[w][v][q];
      total += c;
      below += min(c, rk) + (q < rho && c > rk);  // ids sorted before (rk, rho)
    }
    // inactive ids keep their ascending order behind the active ones
    const unsigned long long ia = __ballot(!act);
    if (lane == 0) wcount[w][wave] = __popcll(ia);
    __syncthreads();
    for (int q = 0; q < wave; ++q) inact_before += wcount[w][q];
    int slot;
    if (act) slot = below < (total & ~31) ? (below & ~31) + POS[below & 31] : below;
    else slot = total + inact_before + mbcnt(ia);
    unsigned char *dst = lists + (((size_t)w * nb + b) * NBRICK + bk) * 256;
    dst[slot] = (unsigned char)t;
    if (t == 0) counts[((size_t)w * nb + b) * NBRICK + bk] = total;
  }
}

// lists u8[2][b][NBRICK][256], counts i32[2][b][NBRICK]; r in {8, 16, 32}
extern "C" int p2pb_conv3d_active_lists(int b, int r, const int *cnt, unsigned char *lists, int *counts, void *stream) {
  if (b <= 0 || (r != 8 && r != 16 && r != 32)) return P2PB_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int nbrick = conv_bricks(r);
  if (r == 32) hipLaunchKernelGGL(active_lists_kernel<32>, dim3(nbrick, b), dim3(256), 0, s, cnt, lists, counts, b);
  else if (r == 16) hipLaunchKernelGGL(active_lists_kernel<16>, dim3(nbrick, b), dim3(256), 0, s, cnt, lists, counts, b);
  else hipLaunchKernelGGL(active_lists_kernel<8>, dim3(nbrick, b), dim3(256), 0, s, cnt, lists, counts, b);
  return p2pb_launch_status();
}

// inactive bricks: the convolution's output there is a known constant per channel (bias, or the
// boundary-class constant K): write it and the brick's exact {sum, sum of squares} partials
template <int R, bool CL>
__global__ __launch_bounds__(256) void conv3d_fill_kernel(int cout, const float *__restrict__ bias,
                                                          const float *__restrict__ out_class,
                                                          const int *__restrict__ brick_list,
                                                          const int *__restrict__ brick_count, float *__restrict__ out,
                                                          float *__restrict__ stats_part) {
  constexpr int TD = 4, TH = 8, TW = 8, BH = R / TH, BW = R / TW, NBRICK = (R / TD) * BH * BW, R3 = R * R * R;
  __shared__ int ncls[27];
  if ((int)blockIdx.x >= *brick_count) return;
  const int entry = brick_list[blockIdx.x];
  const int b = entry / NBRICK, bk = entry % NBRICK;
  const int d0 = (bk / (BH * BW)) * TD, h0 = ((bk / BW) % BH) * TH, w0 = (bk % BW) * TW;
  const int t = threadIdx.x;
  const int d = d0 + t / (TH * TW), h = h0 + (t / TW) % TH, w = w0 + t % TW;
  const int cd = d == 0 ? 0 : (d == R - 1 ? 2 : 1), ch = h == 0 ? 0 : (h == R - 1 ? 2 : 1),
            cw = w == 0 ? 0 : (w == R - 1 ? 2 : 1);
  const int cls = (cd * 3 + ch) * 3 + cw;
  if (t < 27) ncls[t] = 0;
  __syncthreads();
  atomicAdd(&ncls[cls], 1);
  __syncthreads();
  const float *kb = out_class ? out_class + (size_t)b * 27 * cout : nullptr;
  if (!out) {  // statistics only (p2pb_conv3d_k3_forward_sparse flags bit 5: nobody reads the inactive bricks' outputs)
  } else if (CL) {  // voxel-major: the brick's voxels x channels, channels fastest (coalesced)
    __shared__ unsigned char vcls[256];
    vcls[t] = (unsigned char)cls;
    __syncthreads();
    float *ob = out + (size_t)b * cout * R3;
    if ((cout & 3) == 0) {  // 16 bytes per thread, (voxel, channel quad) advanced without a division per element
      const int c4n = cout >> 2, dq = 256 / c4n, dr = 256 % c4n;
      int vl = t / c4n, c4 = t % c4n;
      for (; vl < 256; vl += dq) {
        const int dd = d0 + vl / (TH * TW), hh = h0 + (vl / TW) % TH, ww = w0 + vl % TW;
        const float *src = kb ? kb + vcls[vl] * cout : bias;
        *(f32x4 *)(ob + (size_t)((dd * R + hh) * R + ww) * cout + 4 * c4) = *(const f32x4 *)(src + 4 * c4);
        if (dr) {
          c4 += dr;
          if (c4 >= c4n) {
            c4 -= c4n;
            ++vl;
          }
        }
      }
    } else {
      for (int e = t; e < 256 * cout; e += 256) {
        const int vl = e / cout, co = e - vl * cout;
        const int dd = d0 + vl / (TH * TW), hh = h0 + (vl / TW) % TH, ww = w0 + vl % TW;
        ob[(size_t)((dd * R + hh) * R + ww) * cout + co] = kb ? kb[vcls[vl] * cout + co] : bias[co];
      }
    }
  } else {
    float *ob = out + (size_t)b * cout * R3 + (d * R + h) * R + w;
    for (int co = 0; co < cout; ++co) ob[(size_t)co * R3] = kb ? kb[cls * cout + co] : bias[co];
  }
  if (stats_part) {
    for (int co = t; co < cout; co += 256) {
      float s1 = 0.0f, s2 = 0.0f;
      if (kb) {
        for (int c = 0; c < 27; ++c) {
          const float v = kb[c * cout + co], n = (float)ncls[c];
          s1 += n * v;
          s2 += n * v * v;
        }
      } else {
        const float v = bias[co];
        s1 = 256.0f * v;
        s2 = 256.0f * v * v;
      }
      float *p = stats_part + (((size_t)b * NBRICK + bk) * 4) * cout * 2;
      p[(size_t)co * 2] = s1;
      p[(size_t)co * 2 + 1] = s2;
#pragma unroll
      for (int wv = 1; wv < 4; ++wv) {
        p[((size_t)wv * cout + co) * 2] = 0.0f;
        p[((size_t)wv * cout + co) * 2 + 1] = 0.0f;
      }
    }
  }
}

void conv3d_fill_launch(int r, const ConvArgs &a, const int *inactive_list, const int *inactive_count, bool stats_only) {
  for_value<32, 16>(r, [&](auto R) {
    return for_flag(a.cl, [&](auto CL) {
      hipLaunchKernelGGL((conv3d_fill_kernel<decltype(R)::value, decltype(CL)::value>), dim3(conv_bricks(r) * a.b), dim3(256), 0, a.s,
                         a.cout, a.bias, a.out_class, inactive_list, inactive_count, stats_only ? (float *)nullptr : a.out,
                         a.stats_part);
      return 0;
    });
  });
}
