// vit_common.h -- what the two arithmetics of the DINOv2 forward share: vit.hip (fp32 operands on the vector pipe) and
// vit_f16.hip (fp16 operands on the matrix pipe). The LayerNorm is ONE kernel with the output type as its parameter, so the
// fp16 form is the fp32 result rounded once -- the same bits as `layernorm(x).half()`.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;  // (xor butterfly: every lane holds the same bits)
}

__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }

static inline bool aligned16(const void *p) { return ((size_t)p & 15) == 0; }

// ---- LayerNorm --------------------------------------------------------------------------------------------------------
// one wave per token, two passes over the row (the second hits the cache): mean, then the biased variance of the deviations
// x - mean (and their own small mean, which corrects the first pass's rounding). Never E[x^2] - E[x]^2 of the values, which
// cancels for a stream whose mean is far above its spread. OutT: float, or _Float16 (IEEE conversion, round-to-nearest-even).
template <class OutT>
__global__ __launch_bounds__(256) void vit_layernorm_kernel(int rows, int c, const float *__restrict__ x,
                                                            const float *__restrict__ gamma, const float *__restrict__ beta,
                                                            float eps, OutT *__restrict__ y) {
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int lane = lane_id();
  const float *xr = x + (size_t)r * c;
  float s = 0.0f;
  for (int i = lane; i < c; i += 64) s += xr[i];
  const float mean0 = wave_sum(s) / (float)c;  // off by the rounding of a sum of c terms of the stream's magnitude
  float q = 0.0f, e = 0.0f;
  for (int i = lane; i < c; i += 64) {
    const float d = xr[i] - mean0;
    e += d;
    q = __fmaf_rn(d, d, q);
  }
  // the residual mean of the deviations corrects the first estimate: sum (x - mean)^2 = sum d^2 - c * de^2, de << |d|
  const float de = wave_sum(e) / (float)c;
  const float mean = mean0 + de;
  const float rstd = 1.0f / sqrtf(fmaxf(wave_sum(q) / (float)c - de * de, 0.0f) + eps);
  OutT *yr = y + (size_t)r * c;
  for (int i = lane; i < c; i += 64) yr[i] = (OutT)((xr[i] - mean) * rstd * gamma[i] + beta[i]);
}

}  // namespace
