// pointwise_split.hip -- the matrix-bound 1x1 convolutions (>= 128 channels in and out) as LDS-tiled GEMMs on the 16-bit matrix
// pipe, reading the split weight pack: pw_split_kernel (pw_split.h: 128 or 256 channels x 128 positions per workgroup; f16x3,
// bf16x6, and bf16x3 for the training data gradient) and pw_pp512_kernel (pw_pp512.h: 512 x 128, f16x3 only).
#include "pw_split.h"
#include "pw_pp512.h"

// (256-position workgroups of pw_split_kernel, NB = 2 -- half the weight traffic through L2 at one wave per SIMD less -- measured
//  4 % / 7 % slower and are not instantiated; the wide tile lives in pw_pp512.h, with the pipeline it needs)
template <bool XF, int PL, int WM, int TERMS>
static int pw_split_go(const PwArgs &a) {
  constexpr int NB = 1, lds = (WM / 2 + NB) * PWS_TILE * 16;
  static bool once = false;  // 72 KB of dynamic LDS (above the 64 KB default): opt in once per instantiation
  if (!once) {
    (void)hipFuncSetAttribute((const void *)pw_split_kernel<XF, PL, WM, NB, TERMS>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    once = true;
  }
  const dim3 grid((a.P + 127) / 128, (a.cout + 64 * WM - 1) / (64 * WM), a.b);
  hipLaunchKernelGGL((pw_split_kernel<XF, PL, WM, NB, TERMS>), grid, dim3(128 * WM), lds, a.s, a.cin, a.cout, a.P, pw_nslots(a.P),
                     a.in, (const u32x4 *)a.wp, a.bias, a.bias_b, a.in_scale, a.in_shift, a.in_swish, a.out, a.stats_part, a.minmax,
                     a.pool_u, a.out_pm);
  return p2pb_launch_status();
}
// wm4: 256-channel workgroups. bf16x3 exists for the plain form alone (pointwise.hip refuses the rest).
int pw_split_launch(const PwArgs &a, int terms, bool wm4) {
  if (terms == SPLIT_BF16X3) return for_flag(wm4, [&](auto W4) { return pw_split_go<false, 0, (W4() ? 4 : 2), SPLIT_BF16X3>(a); });
  const int pl = !a.minmax ? 0 : a.pool_u == 0 ? 1 : a.pool_u == 32 ? 32 : 2;  // pws_epilogue's pooling form
  return for_flag(a.in_scale != nullptr, [&](auto XF) {
    return for_value<0, 1, 32, 2>(pl, [&](auto PL) {
      return for_flag(wm4, [&](auto W4) {
        return terms == SPLIT_F16X3 ? pw_split_go<XF(), PL(), (W4() ? 4 : 2), SPLIT_F16X3>(a)
                                    : pw_split_go<XF(), PL(), (W4() ? 4 : 2), SPLIT_BF16X6>(a);
      });
    });
  });
}

template <bool XF, bool POOL>
static int pw_pp512_go(const PwArgs &a) {
  static bool once = false;  // all 160 KB of the CU's LDS
  if (!once) {
    (void)hipFuncSetAttribute((const void *)pw_pp512_kernel<XF, POOL>, hipFuncAttributeMaxDynamicSharedMemorySize, P5_LDS_BYTES);
    once = true;
  }
  hipLaunchKernelGGL((pw_pp512_kernel<XF, POOL>), dim3((a.P + 127) / 128, a.cout / 512, a.b), dim3(512), P5_LDS_BYTES, a.s, a.cin,
                     a.cout, a.P, pw_nslots(a.P), a.in, (const u32x4 *)a.wp, a.bias, a.bias_b, a.in_scale, a.in_shift, a.in_swish,
                     a.out, a.stats_part, a.minmax, a.pool_u);
  return p2pb_launch_status();
}
int pw_pp512_launch(const PwArgs &a) {
  return for_flag(a.in_scale != nullptr, [&](auto XF) {
    return for_flag(a.minmax != nullptr, [&](auto POOL) { return pw_pp512_go<XF(), POOL()>(a); });
  });
}
