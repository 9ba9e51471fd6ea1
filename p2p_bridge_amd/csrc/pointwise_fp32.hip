// pointwise_fp32.hip -- the 1x1 convolutions on the exact-fp32 MFMA (32x32x2) on the fp32 weight pack: M = output
// channels, N = positions, K = input channels. pw_conv_kernel below takes any position count and alignment; rows of whole,
// aligned quads run pw_wide_kernel<TERMS = 0> (pw_wide.h). These are P2PB_CONV_MATH=fp32 and the layers too narrow for a
// 16-channel step; the default arithmetic of everything else is f16x3 (pointwise_f16.hip, pointwise_split.hip).
#include "pw_wide.h"

#define PW_CK 16  // input channels per register stage (2 sub-chunks of 8): 3 waves/SIMD stay resident (32 -> 2)

// packed weights: wp[cin_pad/8][2][cout_pad][4], element (chunk, khalf, co, kk) = W[co][chunk*8 + 2*kk + khalf]
//
// No LDS, no barriers: in a 1x1 convolution the B operand (activations) is not shared between waves --
// each wave owns 64 distinct positions -- so every lane loads its own MFMA B fragments straight from HBM
// (lanes 0..31 = 32 consecutive positions of channel 2kk, lanes 32..63 of channel 2kk+1: two 128-byte
// segments per load instruction) and the four waves of a workgroup run fully decoupled. The loads of
// chunk c+1 are issued before chunk c is multiplied; A fragments (weights) are 16-byte L1/L2 loads issued
// first, so the in-order vmcnt wait in front of the MFMAs never covers the HBM prefetch.
template <int MT, bool XF, bool STATS>
__global__ __launch_bounds__(256, 3) void pw_conv_kernel(int cin, int cout, int cout_pad, int P,
                                                      const float *__restrict__ in, const float *__restrict__ wp,
                                                      const float *__restrict__ bias,
                                                      const float *__restrict__ bias_b,
                                                      const float *__restrict__ in_scale,
                                                      const float *__restrict__ in_shift, int in_swish,
                                                      float *__restrict__ out, float *__restrict__ stats_part) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, khalf = lane >> 5;
  const int p0 = blockIdx.x * 256, co0 = blockIdx.y * (32 * MT), b = blockIdx.z;
  const int pl[2] = {p0 + wave * 64 + l31, p0 + wave * 64 + 32 + l31};
  const bool pok[2] = {pl[0] < P, pl[1] < P};
  const float *inb = in + (size_t)b * cin * P;
  const int nchunk8 = (cin + 7) >> 3;
  __shared__ float pwc_bias[32 * MT];  // bias (+ per-sample bias) through LDS: see pw_wide_kernel
  if (tid < 32 * MT) {
    const int co = co0 + tid;
    float v = 0.0f;
    if (co < cout) {
      v = bias ? bias[co] : 0.0f;
      if (bias_b) v += bias_b[(size_t)b * cout + co];
    }
    pwc_bias[tid] = v;
  }
  __syncthreads();

  f32x16 acc[MT][2];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][s][r] = 0.0f;

  float bcur[PW_CK / 2][2], bnxt[PW_CK / 2][2];
  auto load_b = [&](int ci0, float(&dst)[PW_CK / 2][2]) {
#pragma unroll
    for (int kk = 0; kk < PW_CK / 2; ++kk) {
      const int ci = ci0 + 2 * kk + khalf;
#pragma unroll
      for (int s = 0; s < 2; ++s) dst[kk][s] = (ci < cin && pok[s]) ? inb[(size_t)ci * P + pl[s]] : 0.0f;
    }
  };
  load_b(0, bcur);
  const float *wbase = wp + ((size_t)khalf * cout_pad + co0 + l31) * 4;
  const size_t wchunk_stride = (size_t)2 * cout_pad * 4;
  f32x4 a_cur[PW_CK / 8][MT], a_nxt[PW_CK / 8][MT];
  auto load_a = [&](int chunk0, f32x4(&dst)[PW_CK / 8][MT]) {
#pragma unroll
    for (int sub = 0; sub < PW_CK / 8; ++sub) {
      const int ch = chunk0 + sub < nchunk8 ? chunk0 + sub : nchunk8 - 1;  // clamp: stays inside the buffer
#pragma unroll
      for (int m = 0; m < MT; ++m) dst[sub][m] = *(const f32x4 *)(wbase + (size_t)ch * wchunk_stride + (size_t)m * 32 * 4);
    }
  };
  load_a(0, a_cur);

  for (int ci0 = 0; ci0 < cin; ci0 += PW_CK) {
    const int chunk0 = ci0 >> 3;
    const bool more = ci0 + PW_CK < cin;
    if (more) {  // both operands of the NEXT chunk are requested before this chunk is multiplied
      load_a(chunk0 + PW_CK / 8, a_nxt);
      load_b(ci0 + PW_CK, bnxt);
    }
    if (XF) {
#pragma unroll
      for (int kk = 0; kk < PW_CK / 2; ++kk) {
        const int ci = ci0 + 2 * kk + khalf;
        if (ci < cin) {
          const float sc = in_scale[b * cin + ci], sh = in_shift[b * cin + ci];
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            float v = bcur[kk][s] * sc + sh;
            if (in_swish) v = swishf(v);
            bcur[kk][s] = pok[s] ? v : 0.0f;
          }
        }
      }
    }
#pragma unroll
    for (int sub = 0; sub < PW_CK / 8; ++sub) {
      if (chunk0 + sub >= nchunk8) break;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int s = 0; s < 2; ++s)
            acc[m][s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[sub][m][kk], bcur[sub * 4 + kk][s], acc[m][s], 0, 0, 0);
      }
    }
    if (more) {
#pragma unroll
      for (int kk = 0; kk < PW_CK / 2; ++kk)
#pragma unroll
        for (int s = 0; s < 2; ++s) bcur[kk][s] = bnxt[kk][s];
#pragma unroll
      for (int sub = 0; sub < PW_CK / 8; ++sub)
#pragma unroll
        for (int m = 0; m < MT; ++m) a_cur[sub][m] = a_nxt[sub][m];
    }
  }

  float *outb = out + (size_t)b * cout * P;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
      const float bv = pwc_bias[co - co0];
      float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int p = pl[s];
        const float v = acc[m][s][r] + bv;
        if (co < cout && pok[s]) {
          outb[(size_t)co * P + p] = v;
          if (STATS) {
            s1 += v;
            s2 += v * v;
          }
        }
      }
      if (STATS) {
        s1 = halfwave_sum_to_last(s1);
        s2 = halfwave_sum_to_last(s2);
        if (l31 == 31 && co < cout) {
          float *q = stats_part + ((((size_t)b * gridDim.x + blockIdx.x) * 4 + wave) * cout + co) * 2;
          q[0] = s1;
          q[1] = s2;
        }
      }
    }
  }
}

template <int MT, bool XF, bool STATS>
static int pw_conv_go(const PwArgs &a) {
  const dim3 grid((a.P + 255) / 256, (a.cout + 32 * MT - 1) / (32 * MT), a.b);
  hipLaunchKernelGGL((pw_conv_kernel<MT, XF, STATS>), grid, dim3(256), 0, a.s, a.cin, a.cout, pw_cout_pad(a.cout), a.P, a.in,
                     (const float *)a.wp, a.bias, a.bias_b, a.in_scale, a.in_shift, a.in_swish, a.out, a.stats_part);
  return p2pb_launch_status();
}
int pw_conv_launch(const PwArgs &a) {
  return pw_for_mt(a.cout, [&](auto MT) {
    return for_flag(a.in_scale != nullptr, [&](auto XF) {
      return for_flag(a.stats_part != nullptr, [&](auto ST) { return pw_conv_go<MT(), XF(), ST()>(a); });
    });
  });
}
int pw_wide_fp32_launch(const PwArgs &a) { return pw_wide_form<0>(a); }
