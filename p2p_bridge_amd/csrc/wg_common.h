// wg_common.h -- what the sources of the dense layers' weight gradients (wgrad*.hip) have in common: the plan of a launch (kernel
// form + K-splits, made once in wgrad.hip for the workspace helper and the launcher alike), the host-side argument struct that
// travels from an entry point to the launch site of the kernel that runs, and the small device helpers of the bf16 kernels.
#pragma once
#include "common.h"

#define WG_COT 64  // exact-fp32 3x3x3 form: output channels per workgroup (2 M-tiles)
#define WG_CIT 32  //                        input channels per workgroup (1 N-tile)
#define PW_CH 256  // exact-fp32 1x1 form: positions per K unit

// the kernel form that runs a layer (wgrad.hip: conv_wgrad_plan, pw_wgrad_plan)
enum WgForm {
  WG_FP32,  // exact-fp32 MFMA, operands through LDS, 64-bit addressing (wgrad_fp32.hip): math 2, or an operand of 2 GiB or more
  WG_LDS,   // bf16 terms, operands through LDS with coalesced 16-byte loads (wgrad_bf16.hip): r >= 8 | npos % 4 == 0
  WG_REG,   // bf16 terms, every lane loads its own fragments (wgrad_bf16.hip): r = 4 | the other 1x1 layers
};
struct WgPlan {
  WgForm form;
  int nterm;   // bf16 terms per operand: 2 = "bf16x3", 3 = "bf16x6" (unused by WG_FP32)
  int ns;      // K-splits = partial rows in the workspace
  size_t row;  // floats per partial row: the weights [taps][cout][cin], then cout bias sums
};

// One layer, as an entry point validated it. The kernels' own parameter lists are spelled once each, where the struct is unpacked
// (the *_go functions).
struct WgArgs {
  int b, cin, cout;
  int n;   // grid edge r of a 3x3x3 layer | positions per sample of a 1x1 layer
  int ns;  // WgPlan::ns
  const float *x, *dy;
  float *ws;  // ns partial rows
  bool bias;  // the bias sums are wanted
  hipStream_t s;
};

// launchers of the kernels, each in the object that instantiates them; wgrad.hip has checked the arguments and made the plan
int wg_conv_fp32_launch(const WgArgs &a);                     // wgrad_fp32.hip
int wg_pw_fp32_launch(const WgArgs &a);                       // wgrad_fp32.hip
int wg_conv_bf16_launch(const WgArgs &a, const WgPlan &p);    // wgrad_bf16.hip: WG_LDS | WG_REG
int wg_pw_bf16_launch(const WgArgs &a, const WgPlan &p);      // wgrad_bf16.hip: WG_LDS | WG_REG
// dw, db = the sum of the nsplit partial rows in ascending order (wgrad.hip)
void wg_reduce(int nsplit, int ntap, size_t cc, size_t nbias, const float *part, float *dw, float *db, hipStream_t s);

// (a, b) -> their first NTERM bf16 terms, packed as pairs (common.h split3)
template <int NTERM>
__device__ __forceinline__ void wg_terms(float a, float b, unsigned (&t)[NTERM]) {
  unsigned p0, p1, p2;
  split3(a, b, p0, p1, p2);
  t[0] = p0;
  if (NTERM > 1) t[1] = p1;
  if (NTERM > 2) t[2] = p2;
}

template <int NTERM>
__device__ __forceinline__ void mfma_products(f32x16 &acc, const u32x4 (&a)[NTERM], const u32x4 (&b)[NTERM]) {
  // small terms first; (i, j) with i + j < NTERM
#pragma unroll
  for (int s = NTERM - 1; s >= 0; --s)
#pragma unroll
    for (int i = 0; i <= s; ++i)
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[i]),
                                                    __builtin_bit_cast(bf16x8, b[s - i]), acc, 0, 0, 0);
}

__device__ __forceinline__ void load8(const float *p, bool vec, float (&f)[8]) {
  if (vec) {
    const float4 v0 = *(const float4 *)p, v1 = *(const float4 *)(p + 4);
    f[0] = v0.x, f[1] = v0.y, f[2] = v0.z, f[3] = v0.w, f[4] = v1.x, f[5] = v1.y, f[6] = v1.z, f[7] = v1.w;
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = p[i];
  }
}
