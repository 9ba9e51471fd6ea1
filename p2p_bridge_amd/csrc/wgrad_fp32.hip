// wgrad_fp32.hip -- the weight-gradient GEMMs of wgrad.hip in exact fp32 on the gfx950 matrix cores (v_mfma_f32_32x32x2_f32):
// P2PB_TRAIN_MATH=fp32 (math 2), and every launch whose larger operand reaches 2 GiB (64-bit addressing; wgrad.hip).
//
// 3x3x3: a K unit is a 4x8x8 voxel brick (the whole grid at r = 4). Per unit the workgroup stages the dY brick [64][256] and the
// zero-padded halo brick of X [32][6*10*10] in LDS (odd row pitches: the 32 lanes of a fragment read hit 32 distinct banks), then every
// k-pair (two voxels) is one ds_read_b32 per fragment. The 27 taps are dealt to the four waves (7/7/7/6): a wave keeps
// 2 x 7 accumulator tiles (224 VGPRs) and spends 9 LDS reads per 14 MFMAs (896 matrix cycles) -- the kernel is
// matrix-bound by construction, staging is ~2 % of a unit.
#include "wg_common.h"

#define WG_TPW 7  // taps per wave

template <int TD, int TH, int TW>
struct WBrick {
  static constexpr int HD = TD + 2, HH = TH + 2, HW = TW + 2;
  static constexpr int NV = TD * TH * TW, PLANE = HD * HH * HW;
  static constexpr int PA = NV + 1, PB = PLANE | 1;  // odd LDS row pitches
};

template <int R, int TD, int TH, int TW>
__global__ __launch_bounds__(256) void conv3d_k3_wgrad_kernel(int nb, int cin, int cout, int nsplit,
                                                              const float *__restrict__ x,
                                                              const float *__restrict__ dy,
                                                              float *__restrict__ part, float *__restrict__ bpart) {
  using G = WBrick<TD, TH, TW>;
  constexpr int R3 = R * R * R;
  constexpr int BD = R / TD, BH = R / TH, BW = R / TW, NBRICK = BD * BH * BW;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *dys = smem;                    // [WG_COT][PA]
  float *xs = smem + WG_COT * G::PA;    // [WG_CIT][PB]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, khalf = lane >> 5;
  const int split = blockIdx.x, co0 = blockIdx.y * WG_COT, ci0 = blockIdx.z * WG_CIT;
  const int tap0 = wave * WG_TPW;
  const int ntap = min(WG_TPW, 27 - tap0);

  f32x16 acc[2][WG_TPW];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int t = 0; t < WG_TPW; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][t][r] = 0.0f;
  float bsum = 0.0f;  // thread tid < WG_COT: running sum of dY row tid (only the ci-tile-0 workgroups write it)

  const int units = nb * NBRICK;
  for (int u = split; u < units; u += nsplit) {
    const int b = u / NBRICK, bk = u % NBRICK;
    const int d0 = (bk / (BH * BW)) * TD, h0 = ((bk / BW) % BH) * TH, w0 = (bk % BW) * TW;
    __syncthreads();  // everyone is done with the previous unit's tiles
    // ---- stage dY brick: thread -> voxel(s) j, all rows
    for (int j = tid; j < G::NV; j += 256) {
      const int jd = j / (TH * TW), jh = (j / TW) % TH, jw = j % TW;
      const size_t gv = ((size_t)(d0 + jd) * R + (h0 + jh)) * R + (w0 + jw);
      const float *src = dy + ((size_t)b * cout + co0) * R3 + gv;
#pragma unroll 8
      for (int c = 0; c < WG_COT; ++c) dys[c * G::PA + j] = (co0 + c < cout) ? src[(size_t)c * R3] : 0.0f;
    }
    // ---- stage the zero-padded halo brick of X
    for (int e = tid; e < G::PLANE; e += 256) {
      const int dz = e / (G::HH * G::HW), hy = (e / G::HW) % G::HH, wx = e % G::HW;
      const int d = d0 - 1 + dz, h = h0 - 1 + hy, w = w0 - 1 + wx;
      const bool ok = (unsigned)d < (unsigned)R && (unsigned)h < (unsigned)R && (unsigned)w < (unsigned)R;
      const float *src = x + ((size_t)b * cin + ci0) * R3 + ((size_t)d * R + h) * R + w;
#pragma unroll 8
      for (int c = 0; c < WG_CIT; ++c) xs[c * G::PB + e] = (ok && ci0 + c < cin) ? src[(size_t)c * R3] : 0.0f;
    }
    __syncthreads();
    if (bpart && blockIdx.z == 0 && tid < WG_COT) {
      float s = 0.0f;
      for (int j = 0; j < G::NV; ++j) s += dys[tid * G::PA + j];
      bsum += s;
    }
    // ---- K loop over voxel pairs: voxel v = 2*kk + khalf
    const float *arow = dys + l31 * G::PA;
    const float *brow = xs + l31 * G::PB;
#pragma unroll 2
    for (int kk = 0; kk < G::NV / 2; ++kk) {
      const int v = 2 * kk + khalf;
      const int jd = v / (TH * TW), jh = (v / TW) % TH, jw = v % TW;
      const int hb = (jd * G::HH + jh) * G::HW + jw;
      const float a0 = arow[v], a1 = arow[32 * G::PA + v];
#pragma unroll
      for (int t = 0; t < WG_TPW; ++t) {
        if (t < ntap) {
          const int tap = tap0 + t;
          const int toff = ((tap / 9) * G::HH + (tap / 3) % 3) * G::HW + tap % 3;
          const float bv = brow[hb + toff];
          acc[0][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv, acc[0][t], 0, 0, 0);
          acc[1][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv, acc[1][t], 0, 0, 0);
        }
      }
    }
  }
  // ---- partial out: part[split][tap][co][ci] (lanes = consecutive ci: coalesced rows), bias sums behind it
  float *po = part + (size_t)split * ((size_t)cout * cin * 27 + cout);
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int t = 0; t < WG_TPW; ++t) {
      if (t >= ntap) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf, ci = ci0 + l31;
        if (co < cout && ci < cin) po[((size_t)(tap0 + t) * cout + co) * cin + ci] = acc[m][t][r];
      }
    }
  if (bpart && blockIdx.z == 0 && tid < WG_COT && co0 + tid < cout) po[(size_t)cout * cin * 27 + co0 + tid] = bsum;
}

// 1x1 layers: units = PW_CH-position chunks of one sample; workgroup tile 64 x 64, wave (w & 1, w >> 1) owns one
// 32 x 32 tile
__global__ __launch_bounds__(256) void pointwise_wgrad_kernel(int nb, int cin, int cout, int npos, int nsplit,
                                                              const float *__restrict__ x,
                                                              const float *__restrict__ dy,
                                                              float *__restrict__ part, float *__restrict__ bpart) {
  constexpr int PA = PW_CH + 1;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *dys = smem;            // [64][PA]
  float *xs = smem + 64 * PA;   // [64][PA]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, khalf = lane >> 5;
  const int split = blockIdx.x, co0 = blockIdx.y * 64, ci0 = blockIdx.z * 64;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  float bsum = 0.0f;
  const int nchunk = (npos + PW_CH - 1) / PW_CH;
  const int units = nb * nchunk;
  for (int u = split; u < units; u += nsplit) {
    const int b = u / nchunk, p0 = (u % nchunk) * PW_CH;
    const int np = min(PW_CH, npos - p0);
    __syncthreads();
    {  // thread -> position tid (coalesced rows)
      const bool ok = tid < np;
      const float *sd = dy + ((size_t)b * cout + co0) * npos + p0 + tid;
      const float *sx = x + ((size_t)b * cin + ci0) * npos + p0 + tid;
#pragma unroll 8
      for (int c = 0; c < 64; ++c) {
        dys[c * PA + tid] = (ok && co0 + c < cout) ? sd[(size_t)c * npos] : 0.0f;
        xs[c * PA + tid] = (ok && ci0 + c < cin) ? sx[(size_t)c * npos] : 0.0f;
      }
    }
    __syncthreads();
    if (bpart && blockIdx.z == 0 && tid < 64) {
      float s = 0.0f;
      for (int j = 0; j < np; ++j) s += dys[tid * PA + j];
      bsum += s;
    }
    const float *arow = dys + ((wave & 1) * 32 + l31) * PA;
    const float *brow = xs + ((wave >> 1) * 32 + l31) * PA;
#pragma unroll 4
    for (int kk = 0; kk < PW_CH / 2; ++kk) {
      const int v = 2 * kk + khalf;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[v], brow[v], acc, 0, 0, 0);
    }
  }
  float *po = part + (size_t)split * ((size_t)cout * cin + cout);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int co = co0 + (wave & 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf, ci = ci0 + (wave >> 1) * 32 + l31;
    if (co < cout && ci < cin) po[(size_t)co * cin + ci] = acc[r];
  }
  if (bpart && blockIdx.z == 0 && tid < 64 && co0 + tid < cout) po[(size_t)cout * cin + co0 + tid] = bsum;
}

// ---- launch sites. 160 KB of dynamic LDS (above the 64 KB default): opt in once per kernel ----
template <int R>
static int conv_wgrad_fp32_go(const WgArgs &a) {
  constexpr int TD = 4, TH = R >= 8 ? 8 : 4, TW = TH;
  using G = WBrick<TD, TH, TW>;
  const int cot = (a.cout + WG_COT - 1) / WG_COT, cit = (a.cin + WG_CIT - 1) / WG_CIT;
  const size_t lds = (size_t)(WG_COT * G::PA + WG_CIT * G::PB) * sizeof(float);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void *)conv3d_k3_wgrad_kernel<R, TD, TH, TW>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr = true;
  }
  hipLaunchKernelGGL((conv3d_k3_wgrad_kernel<R, TD, TH, TW>), dim3(a.ns, cot, cit), dim3(256), lds, a.s, a.b, a.cin, a.cout,
                     a.ns, a.x, a.dy, a.ws, a.bias ? a.ws : nullptr);
  return 0;  // (the entry point asks for the launch status, behind the reduction)
}
int wg_conv_fp32_launch(const WgArgs &a) {
  return for_value<32, 16, 8, 4>(a.n, [&](auto R) { return conv_wgrad_fp32_go<R()>(a); });
}

int wg_pw_fp32_launch(const WgArgs &a) {
  const int cot = (a.cout + 63) / 64, cit = (a.cin + 63) / 64;
  const size_t lds = (size_t)(2 * 64 * (PW_CH + 1)) * sizeof(float);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void *)pointwise_wgrad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    attr = true;
  }
  hipLaunchKernelGGL(pointwise_wgrad_kernel, dim3(a.ns, cot, cit), dim3(256), lds, a.s, a.b, a.cin, a.cout, a.n, a.ns, a.x,
                     a.dy, a.ws, a.bias ? a.ws : nullptr);
  return 0;
}
