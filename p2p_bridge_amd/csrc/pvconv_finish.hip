// pvconv_finish.hip -- the small kernels between and behind the two convolutions of a PVConv block that turn statistics partials
// into per-(sample, channel) affines: GroupNorm(+AdaGN) folding (gn_affine_kernel; its arithmetic lives in common.h, GnFinish),
// the SE3d gate (se_gate_affine_kernel) and both in one launch with the point branch's norm (pvconv_tail_kernel).
#include "common.h"

// ------------------------------------------------------------------------------------------------
// GroupNorm(+AdaGN) folded to a per-(sample, channel) affine:  AdaGN(GN(x)) == x*scale + shift.
//   GroupNorm (biased variance, eps) : y = (x - mean_g) * rstd_g * gamma_c + beta_c
//   AdaGN (models/modules.py:341-358): z = y * factor_bc + bias_bc , (factor, bias) = chunk(style, 2)
// Statistics come from the producing kernel's per-slot partial {sum, sum of squares}; they are
// combined in double in a fixed order (deterministic). One thread per (sample, channel); the group
// moments are recomputed by each of the group's channels (C/G <= 64 channels x nslots partials, tiny).
// Also returns chmean[b,c] = mean over positions of the transformed output (SE3d's squeeze input).
// ------------------------------------------------------------------------------------------------
// one workgroup per (sample, group). Thread t accumulates channel (t mod cg) over the slots
// t/cg, t/cg + 256/cg, ... (adjacent threads read adjacent channels: coalesced), the 256/cg partial
// accumulators per channel are then summed in ascending order -- a fixed order, so deterministic.
static __global__ __launch_bounds__(256) void gn_affine_kernel(int c, int groups, int nslots, double count_per_channel,
                                                        const float *__restrict__ part, const float *__restrict__ gamma,
                                                        const float *__restrict__ beta, const float *__restrict__ style,
                                                        int style_stride, float eps, float *__restrict__ scale,
                                                        float *__restrict__ shift, float *__restrict__ chmean,
                                                        float *__restrict__ mean_rstd) {
  __shared__ double lds[4 * 256];
  GnFinish f;  // (the arithmetic lives in common.h: producing kernels handed a GnFinish run it themselves)
  f.gamma = gamma, f.beta = beta, f.style = style, f.scale = scale, f.shift = shift, f.chmean = chmean;
  f.count_per_channel = count_per_channel, f.style_stride = style_stride, f.groups = groups, f.eps = eps;
  gn_finish_group(c, nslots, part, f, blockIdx.y, blockIdx.x, lds, mean_rstd);
}

// part: f32[b, nslots, c, 2]; gamma/beta f32[c] or NULL; style = rows of (factor[c] | bias[c]) with a row pitch of
// style_stride floats (a column slice of the one style GEMM of the evaluation), or NULL -> scale/shift/chmean f32[b,c]
// (for the producers of other translation units that were handed a finisher they cannot run themselves)
int p2pb_gn_affine_launch(int b, int c, int nslots, const float *part, const GnFinish &f, hipStream_t s) {
  hipLaunchKernelGGL(gn_affine_kernel, dim3(f.groups, b), dim3(256), 0, s, c, f.groups, nslots, f.count_per_channel, part, f.gamma,
                     f.beta, f.style, f.style_stride, f.eps, f.scale, f.shift, f.chmean, (float *)nullptr);
  return p2pb_launch_status();
}
extern "C" int p2pb_gn_affine_params_ex(int b, int c, int groups, int nslots, double count_per_channel,
                                        const float *part, const float *gamma, const float *beta, const float *style,
                                        int style_stride, float eps, float *scale, float *shift, float *chmean,
                                        float *mean_rstd, void *stream) {
  if (b <= 0 || c <= 0 || nslots <= 0 || !gn_shape_ok(c, groups, style, style_stride)) return P2PB_EINVAL;
  hipLaunchKernelGGL(gn_affine_kernel, dim3(groups, b), dim3(256), 0, (hipStream_t)stream, c, groups, nslots,
                     count_per_channel, part, gamma, beta, style, style_stride, eps, scale, shift, chmean, mean_rstd);
  return p2pb_launch_status();
}

extern "C" int p2pb_gn_affine_params(int b, int c, int groups, int nslots, double count_per_channel,
                                     const float *part, const float *gamma, const float *beta, const float *style,
                                     int style_stride, float eps, float *scale, float *shift, float *chmean,
                                     void *stream) {
  return p2pb_gn_affine_params_ex(b, c, groups, nslots, count_per_channel, part, gamma, beta, style, style_stride, eps,
                                  scale, shift, chmean, nullptr, stream);
}

// hid[h] = relu(sum_i w1[h][i] * mean[i]) for the SE3d bottleneck (models/pvcnn.py SE3d.fc[0..1]): ONE WAVE PER ROW -- lane l adds
// the terms i = l, l + 64, ... in that order, then the 64 lane sums through a fixed xor tree. (Round 5: the first form gave a row
// to ONE THREAD, c dependent loads from global memory in a row: 16-32 busy threads and ~12 of the tail kernel's 16 us.)
// Both kernels below use it: the same bits whichever runs.
__device__ __forceinline__ void se_hidden(int c, int hidden, const float *__restrict__ w1, const float *mean, float *hid) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  for (int h = wave; h < hidden; h += nw) {
    float acc = 0.0f;
    // (a lane's terms eight at a time, the weight loads issued together from clamped addresses and the tail masked by a select:
    // term by term every load was waited for before the next was issued; profiles/r07_gather_wait_audit.txt. Same order.)
    for (int i0 = lane; i0 < c; i0 += 64 * 8) {
      float wv[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) wv[q] = w1[(size_t)h * c + min(i0 + 64 * q, c - 1)];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int i = i0 + 64 * q;
        const float t = __fmaf_rn(wv[q], mean[min(i, c - 1)], acc);
        acc = i < c ? t : acc;
      }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
    if (lane == 0) hid[h] = fmaxf(acc, 0.0f);
  }
}


// ------------------------------------------------------------------------------------------------
// Squeeze-excite gate (models/modules.py:362-378: Linear(c, c/8, no bias) -> ReLU -> Linear(c/8, c, no bias) ->
// Sigmoid on the per-channel mean of the normalised grid) folded into the devoxelisation affine:
//   gate = sigmoid(W2 relu(W1 chmean)),  aff_a = scale * gate,  aff_b = shift * gate.   One workgroup per sample.
// ------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void se_gate_affine_kernel(int c, int hidden, const float *__restrict__ chmean,
                                                             const float *__restrict__ w1, const float *__restrict__ w2,
                                                             const float *__restrict__ scale,
                                                             const float *__restrict__ shift, float *__restrict__ aff_a,
                                                             float *__restrict__ aff_b) {
  extern __shared__ float se_sm[];  // c means + hidden activations
  float *mean = se_sm, *hid = se_sm + c;
  const int b = blockIdx.x, t = threadIdx.x;
  for (int i = t; i < c; i += 256) mean[i] = chmean[(size_t)b * c + i];
  __syncthreads();
  se_hidden(c, hidden, w1, mean, hid);
  __syncthreads();
  for (int i = t; i < c; i += 256) {
    float acc = 0.0f;
    for (int h = 0; h < hidden; ++h) acc = __fmaf_rn(w2[(size_t)i * hidden + h], hid[h], acc);
    const float gate = 1.0f / (1.0f + expf(-acc));
    aff_a[(size_t)b * c + i] = scale[(size_t)b * c + i] * gate;
    aff_b[(size_t)b * c + i] = shift[(size_t)b * c + i] * gate;
  }
}

// ------------------------------------------------------------------------------------------------
// The tail of a PVConv's voxel branch in ONE launch (round 5: three GroupNorm-folding launches + the gate -> one):
//   workgroup (0, b): GroupNorm(+AdaGN) of the SECOND convolution's output from its statistics partials (gn_finish_sample: the
//     arithmetic and bits of gn_affine_kernel) -> scale, shift, channel mean in LDS -> SE3d gate (se_gate_affine_kernel's
//     arithmetic) -> aff_a = scale * gate, aff_b = shift * gate (hidden == 0: no SE3d, aff = scale, shift);
//   workgroup (1, b): the GroupNorm(+AdaGN) of the POINT branch's 1x1 convolution (its partials have been waiting since
//     before the voxel branch started) -> scale_p, shift_p for the devoxelisation pass that adds swish(h * scale_p + shift_p).
// 1024 threads: four groups at a time. Replaces models/pvcnn.py:283-286 (AdaGN, SE3d) + models/pvcnn.py:162-205's norm.
// ------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(1024) void pvconv_tail_kernel(int c, int hidden, const float *__restrict__ part2, int nslots2,
                                                           GnFinish f2, const float *__restrict__ w1, const float *__restrict__ w2,
                                                           float *__restrict__ aff_a, float *__restrict__ aff_b,
                                                           int cp, const float *__restrict__ partp, int nslotsp, GnFinish fp) {
  extern __shared__ double pt_sm[];  // 4 x 1024 doubles | scale[c] | shift[c] | mean[c] | hid[hidden]
  const int b = blockIdx.y, t = threadIdx.x;
  if (blockIdx.x == 1) {
    gn_finish_sample<4>(cp, nslotsp, partp, fp, b, pt_sm);
    return;
  }
  float *sc = (float *)(pt_sm + 4096), *sh = sc + c, *mean = sh + c, *hid = mean + c;
  gn_finish_sample<4>(c, nslots2, part2, f2, b, pt_sm, sc, sh, mean);
  if (hidden <= 0) {
    for (int i = t; i < c; i += 1024) {
      aff_a[(size_t)b * c + i] = sc[i];
      aff_b[(size_t)b * c + i] = sh[i];
    }
    return;
  }
  se_hidden(c, hidden, w1, mean, hid);
  __syncthreads();
  for (int i = t; i < c; i += 1024) {
    float acc = 0.0f;
    for (int h = 0; h < hidden; ++h) acc = __fmaf_rn(w2[(size_t)i * hidden + h], hid[h], acc);
    const float gate = 1.0f / (1.0f + expf(-acc));
    aff_a[(size_t)b * c + i] = sc[i] * gate;
    aff_b[(size_t)b * c + i] = sh[i] * gate;
  }
}

// part2 f32[b, nslots2, c, 2] + its norm (count2 = positions per channel, groups2, gamma2, beta2, style2 rows of 2c floats or NULL)
// -> aff_a, aff_b f32[b, c] (SE3d gate from w1 f32[hidden, c], w2 f32[c, hidden]; hidden == 0: none); partp (may be NULL)
// f32[b, nslotsp, cp, 2] + its norm -> scale_p, shift_p f32[b, cp]
extern "C" int p2pb_pvconv_tail(int b, int c, int hidden, const float *part2, int nslots2, double count2, int groups2,
                                const float *gamma2, const float *beta2, const float *style2, int style_stride2, float eps2,
                                const float *w1, const float *w2, float *aff_a, float *aff_b, int cp, const float *partp,
                                int nslotsp, double countp, int groupsp, const float *gammap, const float *betap,
                                const float *stylep, int style_stridep, float epsp, float *scale_p, float *shift_p, void *stream) {
  if (b <= 0 || c <= 0 || hidden < 0 || !part2 || nslots2 <= 0 || !aff_a || !aff_b || (hidden > 0 && (!w1 || !w2)) ||
      !gn_shape_ok(c, groups2, style2, style_stride2))
    return P2PB_EINVAL;
  if (partp && (cp <= 0 || nslotsp <= 0 || !scale_p || !shift_p || !gn_shape_ok(cp, groupsp, stylep, style_stridep))) return P2PB_EINVAL;
  GnFinish f2 = {}, fp = {};
  f2.gamma = gamma2, f2.beta = beta2, f2.style = style2, f2.style_stride = style_stride2, f2.groups = groups2, f2.eps = eps2;
  f2.count_per_channel = count2;  // (scale / shift / chmean stay in the kernel's LDS tables)
  fp.gamma = gammap, fp.beta = betap, fp.style = stylep, fp.style_stride = style_stridep, fp.groups = groupsp, fp.eps = epsp;
  fp.count_per_channel = countp, fp.scale = scale_p, fp.shift = shift_p;
  const size_t lds = 4096 * 8 + (size_t)(3 * c + hidden) * 4;
  if (lds > 64 * 1024) return P2PB_EINVAL;
  hipLaunchKernelGGL(pvconv_tail_kernel, dim3(partp ? 2 : 1, b), dim3(1024), lds, (hipStream_t)stream, c, hidden, part2, nslots2, f2,
                     w1, w2, aff_a, aff_b, cp, partp, nslotsp, fp);
  return p2pb_launch_status();
}

extern "C" int p2pb_se_gate_affine(int b, int c, int hidden, const float *chmean, const float *w1, const float *w2,
                                   const float *scale, const float *shift, float *aff_a, float *aff_b, void *stream) {
  if (b <= 0 || c <= 0 || hidden <= 0) return P2PB_EINVAL;
  hipLaunchKernelGGL(se_gate_affine_kernel, dim3(b), dim3(256), (size_t)(c + hidden) * sizeof(float),
                     (hipStream_t)stream, c, hidden, chmean, w1, w2, scale, shift, aff_a, aff_b);
  return p2pb_launch_status();
}
