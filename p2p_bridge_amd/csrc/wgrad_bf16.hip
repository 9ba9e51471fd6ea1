// wgrad_bf16.hip -- the split-operand (bf16) forms of the two weight-gradient GEMMs of wgrad.hip: the default.
// torch.set_float32_matmul_precision("high") (the reference's choice, train.py:221) means exactly this arithmetic: every fp32
// operand is the sum of bf16 terms and the product is accumulated in fp32 on the bf16 matrix pipe (v_mfma_f32_32x32x16_bf16: 16
// K-values per 32-cycle instruction against 2 per 64 cycles for the exact-fp32 MFMA of wgrad_fp32.hip). NTERM = 2 ("bf16x3": x0y0 +
// x0y1 + x1y0, 16 significand bits, the precision class of the reference's TF32 cuDNN / cuBLAS kernels, 3 MFMAs per 16 K-values) or
// NTERM = 3 ("bf16x6", fp32-faithful like the forward kernels, 6 MFMAs).
//
// K = voxels / positions, and an MFMA lane carries 8 CONSECUTIVE K-values of its row: 8 voxels along w. Both operands are
// activations that live in HBM as fp32 rows [channel][voxel]. Workgroup = 64 co x 64 ci (3x3x3: x ONE kd plane, 9 taps): wave
// (m, n) owns the 32 x 32 tile (m, n) -- 144 accumulator registers for the 9 taps -> two waves per SIMD. Split over K as in
// wgrad.hip. Two forms per layer type (wg_common.h WgForm): WG_LDS brings a K unit with coalesced 16-byte loads, splits every
// element once and hands the term planes to the waves through LDS (r >= 8; 1x1 layers whose rows are whole 16-byte pieces); in
// WG_REG every lane loads its own fragments from L1 / L2 and splits them in registers (r = 4; the other 1x1 layers). The LDS
// forms address both tensors through 32-bit buffer offsets (0x80000000 = "outside": the zero padding), which is why wgrad.hip
// sends a launch with an operand of 2 GiB or more to the exact-fp32 form.
#include "wg_common.h"

typedef float f32x4w __attribute__((ext_vector_type(4)));

// ---- 3x3x3, r >= 8: operands staged through LDS (round 5) -----------------------------------------------------------------------
// The register form, which ran every resolution until then, gave every lane its own 32-byte run of its own channel row: 64 lanes of
// a load touch 64 different cache lines, and the CU's address path processes ~one line per clock -- 14 such loads per K unit cost
// ~900 clocks of that path per wave against 864 matrix clocks, for four to eight waves per CU: the r = 32 launches ran at 17-21 %
// of their own MFMA time whatever the loads' latency.
// Here a K unit is 32 voxels (whole grid rows: one at r = 32, two at r = 16, four at r = 8), the workgroup brings
// the unit's dY tile [64 co][32] and the three kh-shifted X tiles [64 ci][32] (zero rows outside the grid: out-of-range buffer
// offsets) with COALESCED 16-byte loads (8 lanes per 128-byte row segment: 8 lines per load instead of 64), splits every element
// into its bf16 terms ONCE (the register form split each one in two waves and three kw alignments) and writes the term planes to
// LDS; a wave's fragments are one ds_read_b128 per plane, the kw = 0 / 2 fragments are the kw = 1 one shifted by a bf16 with
// v_alignbit and one neighbour word (zero at a row end). The next unit's loads are in flight while a unit is multiplied.
// Row pitch 80 bytes: the 16 lanes of a service group of a ds_read_b128 fall on all eight 16-byte bank groups twice.
// Same bf16 terms, products and per-accumulator order of K units within a split as the register form (the split of K over the
// workgroups differs: partial sums round differently, deterministically).
template <int R, int NTERM>
__global__ __launch_bounds__(256, 2) void conv3d_k3_wgrad_lds_kernel(int nb, int cin, int cout, int nsplit,
                                                                     const float *__restrict__ x,
                                                                     const float *__restrict__ dy,
                                                                     float *__restrict__ part,
                                                                     float *__restrict__ bpart) {
  static_assert((R >= 8 && 32 % R == 0) || R == 32, "a K unit is whole grid rows");
  constexpr int R3 = R * R * R, UPS = R3 / 32;  // units per sample
  constexpr int P = 80, ROWS = 256, PB = ROWS * P + 32;  // row pitch (bytes), rows per plane (64 dY + 3 x 64 X), plane bytes
  __shared__ __attribute__((aligned(16))) unsigned char lds[NTERM * PB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, khalf = lane >> 5;
  const int split = blockIdx.x, kd = blockIdx.z;
  const int ncit = (cin + 63) / 64;
  const int co_blk = (blockIdx.y / ncit) * 64, ci_blk = (blockIdx.y % ncit) * 64;
  const int co_t = co_blk + (wave & 1) * 32, ci_t = ci_blk + (wave >> 1) * 32;
  const int ci = ci_t + l31;
  const bool cik = ci < cin;
  const bool do_bias = bpart && kd == 0 && (blockIdx.y % ncit) == 0;
  const int srow = tid >> 3, sp = tid & 7;  // staging role: rows srow, srow + 32 of every tile; piece sp (4 voxels)
  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
  float bs[2] = {0.0f, 0.0f};
  const int total = nb * UPS;
  const auto rsa = __builtin_amdgcn_make_buffer_rsrc((void *)dy, 0, (int)((size_t)nb * cout * R3 * 4), 0x00020000);
  const auto rsx = __builtin_amdgcn_make_buffer_rsrc((void *)x, 0, (int)((size_t)nb * cin * R3 * 4), 0x00020000);
  constexpr unsigned OOB = 0x80000000u;
  f32x4w ra[2], rb[3][2];
  auto issue = [&](int u) {
    const int b = u / UPS, v = (u % UPS) * 32 + 4 * sp;
    const int d = v / (R * R), h = (v / R) % R, w = v % R;
    const bool in = u < total;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int co = co_blk + srow + 32 * j;
      ra[j] = __builtin_bit_cast(f32x4w, __builtin_amdgcn_raw_buffer_load_b128(
                                             rsa, (in && co < cout) ? (unsigned)(((size_t)b * cout + co) * R3 + v) * 4u : OOB, 0, 0));
    }
    const int nd = d + kd - 1;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int nh = h + kh - 1;
      const bool rok = in && (unsigned)nd < (unsigned)R && (unsigned)nh < (unsigned)R;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int c = ci_blk + srow + 32 * j;
        rb[kh][j] = __builtin_bit_cast(
            f32x4w, __builtin_amdgcn_raw_buffer_load_b128(
                        rsx, (rok && c < cin) ? (unsigned)(((size_t)b * cin + c) * R3 + ((size_t)nd * R + nh) * R + w) * 4u : OOB, 0, 0));
      }
    }
  };
  auto put = [&](const f32x4w &v, int row) {  // four voxels of one row -> NTERM planes of 8 bytes at piece sp
    unsigned t0[NTERM], t1[NTERM];
    wg_terms<NTERM>(v[0], v[1], t0);
    wg_terms<NTERM>(v[2], v[3], t1);
#pragma unroll
    for (int s = 0; s < NTERM; ++s) {
      typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
      *(u32x2 *)(lds + s * PB + 16 + row * P + sp * 8) = u32x2{t0[s], t1[s]};
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      put(ra[j], srow + 32 * j);
      if (do_bias) bs[j] += (ra[j][0] + ra[j][1]) + (ra[j][2] + ra[j][3]);
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) put(rb[kh][j], 64 + kh * 64 + srow + 32 * j);
    }
  };
  issue(split);
  for (int u = split; u < total; u += nsplit) {
    __syncthreads();  // the previous unit's fragments are read
    stash();
    __syncthreads();
    issue(u + nsplit);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int col = 16 * (2 * ks + khalf);  // byte offset of the lane's 8 bf16 inside a row
      const int wv = (16 * ks + 8 * khalf) % R;  // its first voxel's w
      const bool wl = wv > 0, wr = wv + 8 < R;
      u32x4 a[NTERM];
#pragma unroll
      for (int s = 0; s < NTERM; ++s) a[s] = *(const u32x4 *)(lds + s * PB + 16 + ((wave & 1) * 32 + l31) * P + col);
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        u32x4 fm[NTERM], fz[NTERM], fp[NTERM];  // kw = 0 (dw = -1), 1, 2
#pragma unroll
        for (int s = 0; s < NTERM; ++s) {
          const unsigned char *base = lds + s * PB + 16 + (64 + kh * 64 + (wave >> 1) * 32 + l31) * P + col;
          fz[s] = *(const u32x4 *)base;
          const unsigned lw = *(const unsigned *)(base - 4), rw = *(const unsigned *)(base + 16);
          const unsigned left = wl ? lw >> 16 : 0u, right = wr ? rw << 16 : 0u;
          fm[s][0] = (fz[s][0] << 16) | left;
#pragma unroll
          for (int i = 1; i < 4; ++i) fm[s][i] = __builtin_amdgcn_alignbit(fz[s][i], fz[s][i - 1], 16);
#pragma unroll
          for (int i = 0; i < 3; ++i) fp[s][i] = __builtin_amdgcn_alignbit(fz[s][i + 1], fz[s][i], 16);
          fp[s][3] = (fz[s][3] >> 16) | right;
        }
        mfma_products<NTERM>(acc[kh * 3 + 0], a, fm);
        mfma_products<NTERM>(acc[kh * 3 + 1], a, fz);
        mfma_products<NTERM>(acc[kh * 3 + 2], a, fp);
      }
    }
  }
  float *po = part + (size_t)split * ((size_t)cout * cin * 27 + cout);
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int oc = co_t + (r & 3) + 8 * (r >> 2) + 4 * khalf;
      if (oc < cout && cik) po[((size_t)(kd * 9 + t) * cout + oc) * cin + ci] = acc[t][r];
    }
  if (do_bias) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float v = bs[j];
      v += __shfl_xor(v, 1);
      v += __shfl_xor(v, 2);
      v += __shfl_xor(v, 4);
      const int co = co_blk + srow + 32 * j;
      if (sp == 0 && co < cout) po[(size_t)cout * cin * 27 + co] = v;
    }
  }
}

// ---- 3x3x3, r = 4 (64-voxel grids): the register form. A K unit is 16 voxels; a lane's fragment of 8 spans two h-rows of four
// voxels, so the fragment of every tap is gathered element-wise from L1 / L2 (no LDS: the reuse is across waves and taps, which the
// caches serve) and split in registers. Larger grids take the LDS form above; its comment says why.
template <int NTERM>
__global__ __launch_bounds__(256, 2) void conv3d_k3_wgrad_r4_kernel(int nb, int cin, int cout, int nsplit,
                                                                    const float *__restrict__ x,
                                                                    const float *__restrict__ dy,
                                                                    float *__restrict__ part,
                                                                    float *__restrict__ bpart) {
  constexpr int R = 4, R3 = R * R * R, KG = R3 / 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, khalf = lane >> 5;
  const int split = blockIdx.x, kd = blockIdx.z;
  const int ncit = (cin + 63) / 64;
  const int co_t = (blockIdx.y / ncit) * 64 + (wave & 1) * 32, ci_t = (blockIdx.y % ncit) * 64 + (wave >> 1) * 32;
  const int co = co_t + l31, ci = ci_t + l31;
  const bool cok = co < cout, cik = ci < cin;
  const bool want_bias = bpart && kd == 0 && (blockIdx.y % ncit) == 0 && (wave >> 1) == 0;
  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
  float bsum = 0.0f;
  const int total = nb * KG;
  for (int g = split; g < total; g += nsplit) {
    const int b = g / KG, q = (g % KG) * 16 + 8 * khalf;
    float fa[8];
    if (cok) load8(dy + ((size_t)b * cout + co) * R3 + q, true, fa);
    else {
#pragma unroll
      for (int i = 0; i < 8; ++i) fa[i] = 0.0f;
    }
    u32x4 a[NTERM];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      unsigned t[NTERM];
      wg_terms<NTERM>(fa[2 * i], fa[2 * i + 1], t);
#pragma unroll
      for (int s = 0; s < NTERM; ++s) a[s][i] = t[s];
    }
    if (want_bias) bsum += ((fa[0] + fa[1]) + (fa[2] + fa[3])) + ((fa[4] + fa[5]) + (fa[6] + fa[7]));
    const float *xrow = x + ((size_t)b * cin + (cik ? ci : 0)) * R3;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        float f[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int v = q + i;
          const int nd = v / (R * R) + kd - 1, nh = (v / R) % R + kh - 1, nw = v % R + kw - 1;
          const bool ok = cik && (unsigned)nd < (unsigned)R && (unsigned)nh < (unsigned)R && (unsigned)nw < (unsigned)R;
          f[i] = ok ? xrow[((size_t)nd * R + nh) * R + nw] : 0.0f;
        }
        u32x4 fb[NTERM];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          unsigned t[NTERM];
          wg_terms<NTERM>(f[2 * i], f[2 * i + 1], t);
#pragma unroll
          for (int s = 0; s < NTERM; ++s) fb[s][i] = t[s];
        }
        mfma_products<NTERM>(acc[kh * 3 + kw], a, fb);
      }
  }
  float *po = part + (size_t)split * ((size_t)cout * cin * 27 + cout);
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int oc = co_t + (r & 3) + 8 * (r >> 2) + 4 * khalf;
      if (oc < cout && cik) po[((size_t)(kd * 9 + t) * cout + oc) * cin + ci] = acc[t][r];
    }
  if (want_bias) {
    bsum += __shfl_xor(bsum, 32);
    if (khalf == 0 && cok) po[(size_t)cout * cin * 27 + co] = bsum;
  }
}

// ---- 1x1, rows of 16-byte pieces: operands through LDS (round 5; see conv3d_k3_wgrad_lds_kernel): a K unit is 64 positions of
// one sample, dY [64 co][64] and X [64 ci][64] arrive by coalesced 16-byte loads (16 lanes per 256-byte row segment), are split into
// their bf16 terms once and written as term planes (row pitch 144 bytes); four k-steps x three products per unit and wave. Rows of
// 16-byte pieces only (npos % 4 == 0: every layer of the networks); pieces past the row end read zeros.
template <int NTERM>
__global__ __launch_bounds__(256, 2) void pointwise_wgrad_lds_kernel(int nb, int cin, int cout, int npos, int nsplit,
                                                                     const float *__restrict__ x,
                                                                     const float *__restrict__ dy,
                                                                     float *__restrict__ part,
                                                                     float *__restrict__ bpart) {
  constexpr int P = 144, PB = 128 * P;  // row pitch (bytes); plane = 64 dY rows + 64 X rows
  __shared__ __attribute__((aligned(16))) unsigned char lds[NTERM * PB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, khalf = lane >> 5;
  const int split = blockIdx.x;
  const int ncit = (cin + 63) / 64;
  const int co_blk = (blockIdx.y / ncit) * 64, ci_blk = (blockIdx.y % ncit) * 64;
  const int co_t = co_blk + (wave & 1) * 32, ci_t = ci_blk + (wave >> 1) * 32;
  const int ci = ci_t + l31;
  const bool cik = ci < cin;
  const bool do_bias = bpart && (blockIdx.y % ncit) == 0;
  const int srow = tid >> 4, sp = tid & 15;  // staging role: rows srow + 16 j of both tiles, piece sp (4 positions)
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  float bs[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  const int UPS = (npos + 63) / 64, total = nb * UPS;
  const auto rsa = __builtin_amdgcn_make_buffer_rsrc((void *)dy, 0, (int)((size_t)nb * cout * npos * 4), 0x00020000);
  const auto rsx = __builtin_amdgcn_make_buffer_rsrc((void *)x, 0, (int)((size_t)nb * cin * npos * 4), 0x00020000);
  constexpr unsigned OOB = 0x80000000u;
  f32x4w ra[4], rb[4];
  auto issue = [&](int u) {
    const int b = u / UPS, pos = (u % UPS) * 64 + 4 * sp;
    const bool in = u < total && pos + 4 <= npos;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int co = co_blk + srow + 16 * j, c = ci_blk + srow + 16 * j;
      ra[j] = __builtin_bit_cast(f32x4w, __builtin_amdgcn_raw_buffer_load_b128(
                                             rsa, (in && co < cout) ? (unsigned)((b * cout + co) * npos + pos) * 4u : OOB, 0, 0));
      rb[j] = __builtin_bit_cast(f32x4w, __builtin_amdgcn_raw_buffer_load_b128(
                                             rsx, (in && c < cin) ? (unsigned)((b * cin + c) * npos + pos) * 4u : OOB, 0, 0));
    }
  };
  auto put = [&](const f32x4w &v, int row) {
    unsigned t0[NTERM], t1[NTERM];
    wg_terms<NTERM>(v[0], v[1], t0);
    wg_terms<NTERM>(v[2], v[3], t1);
#pragma unroll
    for (int s = 0; s < NTERM; ++s) {
      typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
      *(u32x2 *)(lds + s * PB + row * P + sp * 8) = u32x2{t0[s], t1[s]};
    }
  };
  issue(split);
  for (int u = split; u < total; u += nsplit) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      put(ra[j], srow + 16 * j);
      if (do_bias) bs[j] += (ra[j][0] + ra[j][1]) + (ra[j][2] + ra[j][3]);
      put(rb[j], 64 + srow + 16 * j);
    }
    __syncthreads();
    issue(u + nsplit);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int col = 32 * ks + 16 * khalf;
      u32x4 a[NTERM], bq[NTERM];
#pragma unroll
      for (int s = 0; s < NTERM; ++s) {
        a[s] = *(const u32x4 *)(lds + s * PB + ((wave & 1) * 32 + l31) * P + col);
        bq[s] = *(const u32x4 *)(lds + s * PB + (64 + (wave >> 1) * 32 + l31) * P + col);
      }
      mfma_products<NTERM>(acc, a, bq);
    }
  }
  float *po = part + (size_t)split * ((size_t)cout * cin + cout);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int oc = co_t + (r & 3) + 8 * (r >> 2) + 4 * khalf;
    if (oc < cout && cik) po[(size_t)oc * cin + ci] = acc[r];
  }
  if (do_bias) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v = bs[j];
      v += __shfl_xor(v, 1);
      v += __shfl_xor(v, 2);
      v += __shfl_xor(v, 4);
      v += __shfl_xor(v, 8);
      const int co = co_blk + srow + 16 * j;
      if (sp == 0 && co < cout) po[(size_t)cout * cin + co] = v;
    }
  }
}

// ---- 1x1, any row length (npos % 4 != 0 in practice): the register form. A K unit is 16 positions, a lane loads the 8 of its
// own row of dY and of X (element-wise in a ragged tail) and splits them in registers.
template <int NTERM>
__global__ __launch_bounds__(256, 2) void pointwise_wgrad_bf16_kernel(int nb, int cin, int cout, int npos, int nsplit,
                                                                      const float *__restrict__ x,
                                                                      const float *__restrict__ dy,
                                                                      float *__restrict__ part,
                                                                      float *__restrict__ bpart) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, khalf = lane >> 5;
  const int split = blockIdx.x;
  const int ncit = (cin + 63) / 64;
  const int co_t = (blockIdx.y / ncit) * 64 + (wave & 1) * 32, ci_t = (blockIdx.y % ncit) * 64 + (wave >> 1) * 32;
  const int co = co_t + l31, ci = ci_t + l31;
  const bool cok = co < cout, cik = ci < cin;
  const bool want_bias = bpart && (blockIdx.y % ncit) == 0 && (wave >> 1) == 0;
  const bool vec = (npos & 3) == 0;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  float bsum = 0.0f;
  const int KG = (npos + 15) / 16;
  const int total = nb * KG;
  auto consume = [&](const float (&fa)[8], const float (&fb)[8]) {
    if (want_bias) bsum += ((fa[0] + fa[1]) + (fa[2] + fa[3])) + ((fa[4] + fa[5]) + (fa[6] + fa[7]));
    u32x4 a[NTERM], bq[NTERM];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      unsigned t[NTERM];
      wg_terms<NTERM>(fa[2 * i], fa[2 * i + 1], t);
#pragma unroll
      for (int s = 0; s < NTERM; ++s) a[s][i] = t[s];
      wg_terms<NTERM>(fb[2 * i], fb[2 * i + 1], t);
#pragma unroll
      for (int s = 0; s < NTERM; ++s) bq[s][i] = t[s];
    }
    mfma_products<NTERM>(acc, a, bq);
  };
  for (int g = split; g < total; g += nsplit) {
    const int b = g / KG, p = (g % KG) * 16 + 8 * khalf;
    float fa[8], fb[8];
    const float *sa = dy + ((size_t)b * cout + (cok ? co : 0)) * npos + p;
    const float *sb = x + ((size_t)b * cin + (cik ? ci : 0)) * npos + p;
    if (p + 8 <= npos) {
      load8(sa, vec, fa);
      load8(sb, vec, fb);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        fa[i] = p + i < npos ? sa[i] : 0.0f;
        fb[i] = p + i < npos ? sb[i] : 0.0f;
      }
    }
    if (!cok) {
#pragma unroll
      for (int i = 0; i < 8; ++i) fa[i] = 0.0f;
    }
    if (!cik) {
#pragma unroll
      for (int i = 0; i < 8; ++i) fb[i] = 0.0f;
    }
    consume(fa, fb);
  }
  float *po = part + (size_t)split * ((size_t)cout * cin + cout);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int oc = co_t + (r & 3) + 8 * (r >> 2) + 4 * khalf;
    if (oc < cout && cik) po[(size_t)oc * cin + ci] = acc[r];
  }
  if (want_bias) {
    bsum += __shfl_xor(bsum, 32);
    if (khalf == 0 && cok) po[(size_t)cout * cin + co] = bsum;
  }
}

// ---- launch sites ----
static unsigned wg_tiles(const WgArgs &a) { return ((a.cout + 63) / 64) * ((a.cin + 63) / 64); }  // 64 x 64 channel tiles

template <int R, int NTERM>
static int conv_wgrad_lds_go(const WgArgs &a) {
  hipLaunchKernelGGL((conv3d_k3_wgrad_lds_kernel<R, NTERM>), dim3(a.ns, wg_tiles(a), 3), dim3(256), 0,
                     a.s, a.b, a.cin, a.cout, a.ns, a.x, a.dy, a.ws, a.bias ? a.ws : nullptr);
  return 0;  // (the entry point asks for the launch status, behind the reduction)
}
template <int NTERM>
static int conv_wgrad_r4_go(const WgArgs &a) {
  hipLaunchKernelGGL(conv3d_k3_wgrad_r4_kernel<NTERM>, dim3(a.ns, wg_tiles(a), 3), dim3(256), 0, a.s,
                     a.b, a.cin, a.cout, a.ns, a.x, a.dy, a.ws, a.bias ? a.ws : nullptr);
  return 0;
}
int wg_conv_bf16_launch(const WgArgs &a, const WgPlan &p) {
  return for_value<2, 3>(p.nterm, [&](auto NT) {
    if (p.form == WG_REG) return conv_wgrad_r4_go<NT()>(a);
    return for_value<32, 16, 8>(a.n, [&](auto R) { return conv_wgrad_lds_go<R(), NT()>(a); });
  });
}

template <int NTERM>
static int pw_wgrad_lds_go(const WgArgs &a) {
  hipLaunchKernelGGL(pointwise_wgrad_lds_kernel<NTERM>, dim3(a.ns, wg_tiles(a)), dim3(256), 0, a.s, a.b,
                     a.cin, a.cout, a.n, a.ns, a.x, a.dy, a.ws, a.bias ? a.ws : nullptr);
  return 0;
}
template <int NTERM>
static int pw_wgrad_reg_go(const WgArgs &a) {
  hipLaunchKernelGGL(pointwise_wgrad_bf16_kernel<NTERM>, dim3(a.ns, wg_tiles(a)), dim3(256), 0, a.s, a.b,
                     a.cin, a.cout, a.n, a.ns, a.x, a.dy, a.ws, a.bias ? a.ws : nullptr);
  return 0;
}
int wg_pw_bf16_launch(const WgArgs &a, const WgPlan &p) {
  return for_value<2, 3>(p.nterm, [&](auto NT) { return p.form == WG_LDS ? pw_wgrad_lds_go<NT()>(a) : pw_wgrad_reg_go<NT()>(a); });
}
