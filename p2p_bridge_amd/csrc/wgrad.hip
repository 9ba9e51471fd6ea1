// wgrad.hip -- weight gradients of the dense layers for training (BASELINE config 3): the entry points, the plan of a launch
// and the reduction of its partials. Replaces what cuDNN / cuBLAS compute for the reference's nn.Conv3d (models/pvcnn.py:265-282)
// and k=1 Conv1d / Conv2d (models/pvcnn.py:162-205, 803-823) in backward:
//
//   3x3x3 convolution:   dW[co][ci][tap] = sum_{b, v} dY[b, co, v] * X[b, ci, v + off(tap)]     (zero padding)
//   1x1 convolution:     dW[co][ci]      = sum_{b, p} dY[b, co, p] * X[b, ci, p]
//   both:                db[co]          = sum_{b, p} dY[b, co, p]
//
// (The data gradients need no kernel of their own: dX of the 3x3x3 convolution is the forward kernel of conv3d_split.h
// run on dY with the taps flipped and the channel roles swapped, dX of a 1x1 layer is the forward GEMM of
// pointwise.hip with the transposed weight -- p2p_bridge_amd/dense.py.)
//
// Formulation: a GEMM whose reduction dimension is the VOXEL / POSITION index: M = output channels (A operand = dY
// rows), N = input channels (B operand = X rows, shifted by the tap offset), K = B * r^3. The output is tiny and K is
// huge, so the launch is split over K: every workgroup owns one (co tile, ci tile) and walks a strided subset of
// the K units, keeping the accumulators in registers all the way, and writes ONE partial row [taps][co][ci] | bias sums;
// wgrad_reduce_kernel adds the partial rows in a fixed order (deterministic: no float atomics).
//
// Three kernel forms compute the partials (wg_common.h WgForm; chosen by conv_wgrad_plan / pw_wgrad_plan below):
//   math 0 = "bf16x3" (THE DEFAULT: "high" matmul precision, train.py:221) and 1 = "bf16x6" (fp32-faithful): operands split into
//     bf16 terms on the bf16 matrix pipe, wgrad_bf16.hip -- staged through LDS where the rows allow it (r >= 8; npos % 4 == 0:
//     every layer of the networks except the convolutions on 4^3 grids), else loaded by every lane for itself;
//   math 2 = exact fp32 MFMA, wgrad_fp32.hip -- also what runs a bf16 request whose larger operand reaches 2 GiB.
// The occupied-voxel form of a PVConv's first convolution has entry points of its own: wgrad_occ.hip.
#include "wg_common.h"

// out = sum_s part[s], s ascending (deterministic). A partial row is [ntap][cout*cin] weights | cout bias sums; the
// weights leave in the parameter's layout dw[co][ci][ntap] (coalesced reads of the partials, one scattered write).
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(int nsplit, int ntap, size_t cc, size_t nbias,
                                                           const float *__restrict__ part, float *__restrict__ dw,
                                                           float *__restrict__ db) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t n = cc * ntap, row = n + nbias;
  if (i >= (db ? row : n)) return;
  // same ascending order (same bits); eight partials in flight per thread -- the plain loop was one L2 round trip per
  // addend (23 us per launch, 52 launches per training step)
  float s = 0.0f;
  int k = 0;
  for (; k + 8 <= nsplit; k += 8) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = part[(size_t)(k + j) * row + i];
#pragma unroll
    for (int j = 0; j < 8; ++j) s += v[j];
  }
  for (; k < nsplit; ++k) s += part[(size_t)k * row + i];
  if (i < n) dw[(i % cc) * ntap + i / cc] = s;
  else db[i - n] = s;
}

void wg_reduce(int nsplit, int ntap, size_t cc, size_t nbias, const float *part, float *dw, float *db, hipStream_t s) {
  // (round 5: noting these ~50 reductions per step and performing them in batched launches behind backward measured SLOWER --
  //  12.9 -> 13.1 ms per config-3 step, profiles/r05b_defer_reduce_ab.txt: the partials are read back from HBM instead of L2)
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(cdiv((long)(cc * ntap + nbias), 256)), dim3(256), 0, s, nsplit, ntap, cc, nbias, part,
                     dw, db);
}

// K-splits of a launch: enough workgroups to fill the chip (`target`), but the partials (written once, read once by
// the reduction) stay below ~48 MB -- wide layers on small grids have few K units and large outputs
static int wgrad_nsplit(long units, int wgs_per_split, int target, size_t out_floats) {
  // `target` = the workgroup slots of the chip for this kernel (256 CUs x 2 for the bf16 forms): the largest split count whose
  // grid still fits them at once -- one more workgroup than slots is a second round for one CU and the launch waits for it
  // (round 5: 384 workgroups of the r = 32 layers on 256 CUs left half the CUs with two and half with one)
  long s = target >= wgs_per_split ? target / wgs_per_split : 1;
  const long cap = (long)((48u << 20) / (out_floats * sizeof(float)));
  if (s > cap) s = cap;
  if (s > units) s = units;
  if (s > 192) s = 192;
  return s < 1 ? 1 : (int)s;
}

// math: 0 = bf16x3 (default; "high" matmul precision, train.py:221), 1 = bf16x6 (fp32-faithful), 2 = exact fp32 MFMA.
// The plan of a launch: which form runs, its K-splits, its partial row. Made HERE and nowhere else, for the workspace helper and
// the launcher alike -- two answers would be a workspace overrun.
// The bf16 forms address both tensors through 32-bit buffer offsets (0x80000000 = "outside": the zero padding). A batch whose
// larger operand reaches 2 GiB therefore runs the exact-fp32 form (64-bit addressing; slower, never less accurate) instead of
// being refused mid-backward.
static WgPlan conv_wgrad_plan(int b, int cin, int cout, int r, int math) {
  if (math != 2 && (size_t)b * (cin > cout ? cin : cout) * r * r * r * 4 >= (1ull << 31)) math = 2;
  WgPlan p;
  p.form = math == 2 ? WG_FP32 : r >= 8 ? WG_LDS : WG_REG;
  p.nterm = math == 1 ? 3 : 2;
  // K units per sample: 4x8x8 bricks (fp32; one 4^3 brick at r = 4), 32 voxels (LDS form), 16 (r = 4)
  const int units = p.form == WG_FP32 ? (r >= 8 ? (r / 4) * (r / 8) * (r / 8) : 1) : p.form == WG_LDS ? r * r * r / 32 : r * r * r / 16;
  const int wgs = p.form == WG_FP32 ? ((cout + WG_COT - 1) / WG_COT) * ((cin + WG_CIT - 1) / WG_CIT)
                                    : ((cout + 63) / 64) * ((cin + 63) / 64) * 3;
  p.ns = wgrad_nsplit((long)b * units, wgs, 512, (size_t)cout * cin * 27);
  p.row = (size_t)cout * cin * 27 + cout;
  return p;
}
// 1x1: the LDS form takes rows of 16-byte pieces below 2 GiB, the register form the rest (64-bit addressing)
static WgPlan pw_wgrad_plan(int b, int cin, int cout, int npos, int math) {
  const bool lds = (npos & 3) == 0 && (size_t)b * (cin > cout ? cin : cout) * npos * 4 < (1ull << 31);
  WgPlan p;
  p.form = math == 2 ? WG_FP32 : lds ? WG_LDS : WG_REG;
  p.nterm = math == 1 ? 3 : 2;
  const int units = p.form == WG_FP32 ? (npos + PW_CH - 1) / PW_CH : p.form == WG_LDS ? (npos + 63) / 64 : (npos + 15) / 16;
  p.ns = wgrad_nsplit((long)b * units, ((cout + 63) / 64) * ((cin + 63) / 64), 512, (size_t)cout * cin);
  p.row = (size_t)cout * cin + cout;
  return p;
}

extern "C" size_t p2pb_conv3d_k3_wgrad_ws_floats(int b, int cin, int cout, int r, int math) {
  const WgPlan p = conv_wgrad_plan(b, cin, cout, r, math);
  return (size_t)p.ns * p.row;
}

extern "C" int p2pb_conv3d_k3_wgrad(int b, int cin, int cout, int r, const float *x, const float *dy, float *dw,
                                    float *db, float *ws, int math, void *stream) {
  if (b <= 0 || cin <= 0 || cout <= 0 || !x || !dy || !dw || !ws || math < 0 || math > 2) return P2PB_EINVAL;
  if (r != 4 && r != 8 && r != 16 && r != 32) return P2PB_EINVAL;
  const WgPlan p = conv_wgrad_plan(b, cin, cout, r, math);
  const WgArgs a = {b, cin, cout, r, p.ns, x, dy, ws, db != nullptr, (hipStream_t)stream};
  if (const int rc = p.form == WG_FP32 ? wg_conv_fp32_launch(a) : wg_conv_bf16_launch(a, p)) return rc;
  wg_reduce(p.ns, 27, (size_t)cout * cin, (size_t)cout, ws, dw, db, a.s);
  return p2pb_launch_status();
}

extern "C" size_t p2pb_pointwise_wgrad_ws_floats(int b, int cin, int cout, int npos, int math) {
  const WgPlan p = pw_wgrad_plan(b, cin, cout, npos, math);
  return (size_t)p.ns * p.row;
}

extern "C" int p2pb_pointwise_wgrad(int b, int cin, int cout, int npos, const float *x, const float *dy, float *dw,
                                    float *db, float *ws, int math, void *stream) {
  if (b <= 0 || cin <= 0 || cout <= 0 || npos <= 0 || !x || !dy || !dw || !ws || math < 0 || math > 2)
    return P2PB_EINVAL;
  const WgPlan p = pw_wgrad_plan(b, cin, cout, npos, math);
  const WgArgs a = {b, cin, cout, npos, p.ns, x, dy, ws, db != nullptr, (hipStream_t)stream};
  if (const int rc = p.form == WG_FP32 ? wg_pw_fp32_launch(a) : wg_pw_bf16_launch(a, p)) return rc;
  wg_reduce(p.ns, 1, (size_t)cout * cin, (size_t)cout, ws, dw, db, a.s);
  return p2pb_launch_status();
}
