// conv3d_common.h -- what the forms of the 3x3x3 / stride 1 / pad 1 voxel convolution share: the formulation, the brick
// geometries, the folded operand transform, the pack sizes, and the host-side argument struct and dispatch helpers of the
// launchers. The forms, one file each:
//   conv3d_split.h    the split-operand dense kernel (fp32 operands as 16-bit terms on the matrix pipe; f16x3 is the default
//                     arithmetic and this kernel and its compact variant are where the network's time goes)
//   conv3d_compact.h  its compact variant: only the listed voxels of a brick are computed
//   conv3d_fp32.hip   the exact-fp32 MFMA kernel (conv_math = fp32) and its weight pack
//   conv3d.hip        the f16x3 instantiations, the forward / sparse / compact entry points, split packs, pre-split grids
//   conv3d_bf16x6.hip, conv3d_bf16x3.hip   the other two arithmetics' instantiations, behind bridge functions
//   conv3d_lists.hip  brick and voxel lists from the occupancy, the constant fill of inactive bricks
//   conv3d_farfield.hip   far-field constants of a second convolution
//
// Formulation: implicit GEMM   out[co, p] = sum_{tap, ci} W[tap][ci][co] * in[ci, p + off(tap)]
//   M = output channels (MFMA rows), N = voxels (MFMA columns), K = 27 * Cin.
// N is the voxel index on purpose: an accumulator register then holds consecutive w-voxels of one
// output channel across lanes 0..31, so the NCDHW store is lane-consecutive.
//
// Sparsity (exact, not approximate). A PU-Net patch is a 2-manifold: ~2.5 % of a 32^3 grid is occupied.
//   * first convolution of a PVConv: the input is zero away from the surface -> a (brick, chunk) whose
//     staged halo tile is all zero contributes exactly +0 and its 27x4 MFMA steps are skipped;
//   * second convolution: its input swish(affine(conv0)) equals a per-channel constant a[b,ci] wherever
//     conv0's input was zero (conv0 = bias there, exactly). By linearity
//         conv(x) = conv(x - a) + conv(a),
//     x - a is exactly zero in the far field (same skip applies) and conv(a) -- a constant field with
//     zero padding -- depends only on which of the 27 boundary classes (low/interior/high per axis) the
//     voxel is in: K[b, class, co] = bias + sum_{taps inside} sum_ci W*a, added in the epilogue.
// Every output voxel and every statistic is still produced by this kernel; only all-zero MFMA work is
// skipped. Compact 4x8x8 bricks (instead of full-row bricks) make the zero test fine-grained in 3-D.
#pragma once
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define CONV_CK 8  // input channels per LDS stage

// brick = TD x TH x TW voxels = 8 N-tiles of 32 (2 for R = 4); an N-tile = ND x NH x TW voxels
template <int R, bool COMPACT>
struct ConvGeom;
template <>
struct ConvGeom<32, false> {
  static constexpr int TD = 2, TH = 4, TW = 32, ND = 1, NH = 1;
};
template <>
struct ConvGeom<16, false> {
  static constexpr int TD = 2, TH = 8, TW = 16, ND = 1, NH = 2;
};
template <>
struct ConvGeom<8, false> {
  static constexpr int TD = 4, TH = 8, TW = 8, ND = 1, NH = 4;
};
template <>
struct ConvGeom<4, false> {
  static constexpr int TD = 4, TH = 4, TW = 4, ND = 2, NH = 4;
};
template <>
struct ConvGeom<32, true> : ConvGeom<8, false> {};
template <>
struct ConvGeom<16, true> : ConvGeom<8, false> {};
template <>
struct ConvGeom<8, true> : ConvGeom<8, false> {};
template <>
struct ConvGeom<4, true> : ConvGeom<4, false> {};

// Swish with the hardware exp2 / reciprocal units: v * rcp(1 + exp2(-v*log2(e))). ~1e-6 relative error
// (both units are 1 ulp), an order of magnitude below the fp32 summation-order noise of the dense layers
// and two below the 1e-4 parity budget; 6 VALU ops instead of ~45 for expf + IEEE divide. It matters
// because the activation is recomputed on every operand stage (once per output-channel block).
__device__ __forceinline__ float fast_swish(float v) {
  return v * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(v * -1.44269504088896340736f));
}

// the folded operand transform, ONE definition used by the staging code and by far_value_kernel so that
// "x - a" is bit-exactly zero wherever x is the far-field constant
__device__ __forceinline__ float xf_apply(float v, float sc, float sh, int swish) {
  v = v * sc + sh;
  return swish ? fast_swish(v) : v;
}

#define CONV_SCK 16  // input channels per LDS stage of the split kernel = K of one bf16 MFMA
// byte offset of the trailer {max|w| bits, 1 / (S_x S_w)} behind a split pack (fp16 mode, common.h)
static __host__ __device__ size_t conv_split_trailer_bytes(int nchunk, int cout_pad) {
  return (size_t)27 * nchunk * 3 * 2 * cout_pad * 8 * sizeof(unsigned short);
}

// Brick geometry of the split kernel: 4 x 8 x 8 bricks whose N-tiles are 4(d) x 1(h) x 8(w) columns. A B fragment is
// a ds_read_b128, which the LDS serves in four groups of 16 lanes ({0-3,12-15,20-27}, {4-11,16-19,28-31}, ...),
// one cycle per group if the 16 lanes hit 16 different 16-byte bank groups. With the d-plane pitch of the halo
// tile (100 slots = 4 mod 16) the four d-rows of an N-tile start 4 bank groups apart, and swapping the two w-halves
// in rows 1 and 2 (lane_w below) gives every service group the residues {0..15} exactly once -- conflict-free for
// every tap offset (a tap only adds a constant). The h-row shape of the fp32 kernel is 3-way conflicted (pitch 10).
template <int R>
struct SplitGeom {
  static constexpr int TD = 4, TH = 8, TW = 8, ND = 4, NH = 1;
};
template <>
struct SplitGeom<4> : ConvGeom<4, false> {};
template <int TW>
__device__ __forceinline__ int lane_w(int l31) {
  const int jw = l31 % TW, jr = l31 / TW;
  return (TW == 8 && (jr == 1 || jr == 2)) ? jw ^ 4 : jw;
}

static int conv_bricks(int r) { return r == 32 ? 128 : r == 16 ? 16 : r == 8 ? 2 : 1; }  // both geometries

// ---- host side: one argument struct from the entry points through the launchers and bridge functions to the kernel launch ----
// (the kernels' own parameter lists are spelled once each, where the struct is unpacked: conv_fp32_go, conv_split_go,
//  conv_compact_go)
struct ConvArgs {
  int b, cin, cout;
  const float *in;  // operand grid (pre: the pre-split S format of conv3d_split.h)
  const void *wt;   // packed weights of the form that is launched
  const float *bias, *out_class, *in_scale, *in_shift;
  int in_swish;
  const float *in_sub;
  int skip_zero;                        // the kernels' skip_zero argument (compact form: bit 1 = listed outputs only)
  const int *brick_list, *brick_count;  // dense forms: the active (sample, brick) pairs, or NULL = every brick
  const unsigned char *alist;           // compact form: per-brick voxel lists and their counts
  const int *acount;
  float *out, *stats_part;
  bool cl, pre;  // voxel-major tensors; `in` is pre-split
  hipStream_t s;
};

// launchers of the kernels that live in other objects than the entry points of conv3d.hip
// conv3d_fp32.hip: r in {4, 8, 16, 32} (else P2PB_EINVAL), compact bricks for r >= 16 only, mt = 32-channel tiles per workgroup
int conv3d_fp32_launch(int r, bool compact, int mt, const ConvArgs &a);
// conv3d_bf16x6.hip / conv3d_bf16x3.hip: the split kernels in the arithmetics that are not the default
int conv3d_bf16x6_split(int r, int mt, const ConvArgs &a);
int conv3d_bf16x6_compact(int r, const ConvArgs &a);
int conv3d_bf16x3_split(int r, int mt, const ConvArgs &a);
// conv3d_lists.hip: constants (and their statistics; stats_only: those alone) of the `inactive` bricks, r in {16, 32}. Launch only:
// the caller's p2pb_launch_status() behind its own launch reports for both
void conv3d_fill_launch(int r, const ConvArgs &a, const int *inactive_list, const int *inactive_count, bool stats_only);
