// pw_common.h -- what the sources of the shared point MLPs (1x1 convolutions, pointwise*.hip) have in common: the small device
// helpers of their kernels, the geometry of the weight packs, the `flags` bits of the entry points, and the one host-side
// argument struct that travels from an entry point (pointwise.hip) to the launch site of the kernel that runs the layer.
#pragma once
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Swish on the hardware exp2 / reciprocal units (see conv3d_common.h fast_swish for the error budget)
__device__ __forceinline__ float swishf(float v) {
  return v * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(v * -1.44269504088896340736f));
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_perm(float v) {
  const int i = __builtin_bit_cast(int, v);
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(i, i, CTRL, ROW_MASK, 0xf, false));
}
// min and max over aligned groups of g lanes. g = 2..16: every lane of the group ends with the result
// (xor-1, xor-2 inside quads, then the half-row and row mirrors); g = 32: lanes 31 / 63 hold their half-wave's.
__device__ __forceinline__ void group_minmax(float &mn, float &mx, int g) {
  if (g > 1) { mn = vmin_raw(mn, dpp_perm<0xB1, 0xf>(mn)); mx = vmax_raw(mx, dpp_perm<0xB1, 0xf>(mx)); }    // quad_perm [1,0,3,2]
  if (g > 2) { mn = vmin_raw(mn, dpp_perm<0x4E, 0xf>(mn)); mx = vmax_raw(mx, dpp_perm<0x4E, 0xf>(mx)); }    // quad_perm [2,3,0,1]
  if (g > 4) { mn = vmin_raw(mn, dpp_perm<0x141, 0xf>(mn)); mx = vmax_raw(mx, dpp_perm<0x141, 0xf>(mx)); }  // row_half_mirror
  if (g > 8) { mn = vmin_raw(mn, dpp_perm<0x140, 0xf>(mn)); mx = vmax_raw(mx, dpp_perm<0x140, 0xf>(mx)); }  // row_mirror
  if (g > 16) { mn = vmin_raw(mn, dpp_perm<0x142, 0xa>(mn)); mx = vmax_raw(mx, dpp_perm<0x142, 0xa>(mx)); } // row_bcast:15
}

// the weight packs (made in pointwise.hip). fp32 pack: wp[cin_pad/8][2][cout_pad][4]
static inline int pw_cin_pad(int cin) { return (cin + 7) / 8 * 8; }
static inline int pw_cout_pad(int cout) { return (cout + 127) / 128 * 128; }
// split pack: one tile per (32 input channels, 128 output channels), [kstep 2][split 3][khalf 2][128 co] x 16 bytes
#define PWS_CK 32
#define PWS_TILE (2 * 3 * 2 * 128)  // 16-byte groups per operand tile (24 KB)
static inline int pw_nslots(int P) { return (P + 255) / 256 * 4; }  // statistics slots per sample (p2pb_pointwise_stats_floats)

static bool pw_wide_ok(int P, const float *in, const float *out) {
  // 16-byte rows: every row of in/out starts on a 16-byte boundary and holds whole quads
  return P % 4 == 0 && (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
}

// pool_u = neighbourhood size (4, 8, 16, 32 or 64 consecutive positions) or 0 for the global pool
static int pool_lanes(int pool_u) { return pool_u == 0 ? 32 : pool_u / 4; }

// the `flags` argument of the convolution entry points (include/p2pb_hip.h)
enum {
  PW_SPLIT_PACK = 4,        // bit 2: wp is the split pack (pointwise_split.hip), else the fp32 pack
  PW_OUT_POINT_MAJOR = 32,  // bit 5: out f32[b, npos, cout]; no statistics
  PW_WIDE_TILING = 128,     // bit 7, with bit 2: the register-tiled kernel on the split pack (pointwise_f16.hip)
};

// the gathered operand of pw_wide_kernel<GATHER> (pw_wide.h)
struct PwGather {
  const float *cxt;  // f32[b, P / gu, cin] or NULL
  const int *idx;    // i32[b, P]
  int gn, gu;        // points per cloud, neighbours per centre
};

// One layer, as an entry point validated it. The kernels' own parameter lists are spelled once each, where the struct is
// unpacked: pw_conv_go, pw_wide_go, pw_split_go, pw_pp512_go.
struct PwArgs {
  int b, cin, cout, P;
  const float *in;  // f32[b, cin, P]; the gathered form: the point-major rows zt
  const void *wp;   // the weight pack of the form that is launched
  const float *bias, *bias_b, *in_scale, *in_shift;
  int in_swish;
  float *out, *stats_part;
  float *minmax;  // pooling epilogue: {min, max} per group of pool_u positions (0: the global pool's partials), or NULL
  int pool_u;
  int out_pm;  // point-major output
  hipStream_t s;
};

// MT, the 32-channel tiles per wave of the register-tiled kernels, as a template argument (common.h for_flag): 64 output channels
// per wave (128 measured slower: the accumulators alone would take 256 registers), 32 for the layers that have no more
template <class F>
static inline int pw_for_mt(int cout, F &&f) {
  return cout > 32 ? f(std::integral_constant<int, 2>{}) : f(std::integral_constant<int, 1>{});
}

// launchers of the kernels, each in the object that instantiates them; pointwise.hip chooses among them and has checked the arguments
int pw_conv_launch(const PwArgs &a);                         // pointwise_fp32.hip: any alignment; channel-major output, no pooling
int pw_wide_fp32_launch(const PwArgs &a);                    // pointwise_fp32.hip: 16-byte rows
int pw_wide_f16_launch(const PwArgs &a);                     // pointwise_f16.hip: 16-byte rows, split pack of f16x3
int pw_gather_launch(const PwArgs &a, const PwGather &gat);  // pointwise_f16.hip: statistics + neighbourhood pooling, nothing stored
int pw_split_launch(const PwArgs &a, int terms, bool wm4);   // pointwise_split.hip: terms = the arithmetic the pack was made for
int pw_pp512_launch(const PwArgs &a);                        // pointwise_split.hip: f16x3, cin % 64 == 0, cout % 512 == 0
