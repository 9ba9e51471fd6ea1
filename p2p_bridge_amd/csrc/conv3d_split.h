// conv3d_split.h -- the split-operand dense kernel of the voxel convolution (conv3d_common.h): its two tap loops, the LDS-DMA
// stage of pre-split operands, the kernel and its launcher. Included by the one object per arithmetic that instantiates it
// (conv3d.hip: f16x3, conv3d_bf16x6.hip, conv3d_bf16x3.hip); TERMS is a template argument all the way down.
//
// Split-operand form (the default): the same implicit GEMM on the bf16 matrix pipe, fp32-faithful.
//
// gfx950 multiplies fp32 on the matrix cores at 1/16 of the bf16 rate (v_mfma_f32_32x32x2_f32: 2048 MACs
// per 64 cycles; v_mfma_f32_32x32x16_bf16: 16384 per 32), and has no TF32. Each fp32 operand is therefore
// split into three bf16 terms, x = x0 + x1 + x2 with x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1)
// (round-to-nearest; the two residuals are exact in fp32), which carries 24+ significand bits, and a product
// is evaluated as the six terms
//        x*y ~= x2*y0 + x1*y1 + x0*y2 + x1*y0 + x0*y1 + x0*y0        (bf16 x bf16 is exact in fp32)
// accumulated in the fp32 MFMA accumulator, small terms first. The three dropped terms are below
// 2^-26 |x*y| (a quarter of an fp32 ulp), so the result differs from the exact-fp32 MFMA kernel above by
// less than a change of summation order: measured against fp64 on the network's layer shapes the rms error
// is 1.6e-7 for this kernel vs 1.9e-7 for the fp32 MFMA one (tests/test_fused_gpu.py pins this).
// Six bf16 MFMAs (192 cycles) replace eight fp32 ones (512 cycles) per 32x32x16 block: 2.67x fewer matrix
// cycles; measured 196 vs 120 TFLOP/s (fp32-equivalent) on the 128->128 r=16 layer.
//
// Layout: LDS tile[split][khalf][halo voxel] of 16-byte groups = 8 consecutive input channels as bf16, so a
// lane's B fragment of one MFMA is one ds_read_b128; weights pre-split and packed
// [tap][chunk16][split][khalf][cout_pad][8 bf16] so an A fragment is one 16-byte load. The operand
// transform (folded norm + Swish, far-field subtraction), the zero-tile skip, the brick lists and the epilogue
// are those of the fp32 kernel; the split happens once per staged element and is reused by 27 taps.
#pragma once
#include "conv3d_common.h"

#ifndef CONV_NTAPS
#define CONV_NTAPS 27  // (timing experiments compile fewer)
#endif
// The 27-tap MFMA loop of one input stage (16 channels) for NT column tiles of one M-tile.
// Six products per (tap, tile), the small ones first: x0y2, x1y1, x2y0 | x1y0, x0y1 | x0y0. The B fragments roll
// through ONE register set: y2 of the next tap is read as soon as this tap's x0y2 products have issued, y1 after
// x0y1, y0 at the top of the tap (it is first needed by the third product) -- every LDS read has >= 2 NT MFMAs
// in front of its first use without a second fragment buffer; A fragments come straight from L2, one tap ahead.
// The scheduling barriers pin this order, else every load sinks to its first use.
// TERMS == SPLIT_F16X3 (the default, p2pb_set_split_terms): the fp16-pair split of common.h -- two operand planes, three
// products h1g0, h0g1, h0g0 (<= 3 * 2^-22 |x*y| inside fp16's range); the third plane of tile / pack is then unused.
// (The same three products of the bf16 split -- TERMS == SPLIT_BF16X3, <= 3 * 2^-18 -- were measured at the same speed
// and 6.4e-5 network error, at the 1e-4 parity bar instead of inside it: superseded, not instantiated.)
#ifndef SPLIT_TAPS_AD
#define SPLIT_TAPS_AD 3  // taps of weight prefetch in split_taps (experiment builds: -DSPLIT_TAPS_AD=1 is the round-4 schedule)
#endif
template <int NT, int HH, int HW, int PLANE, int TERMS>
__device__ __forceinline__ void split_taps(f32x16 (&acc)[NT], const u32x4 *__restrict__ tile, const u32x4 *wchunk,
                                           size_t wsplit_stride, size_t wtap_stride, const int (&nbase)[NT], int khalf) {
  constexpr int NP = split_planes(TERMS);  // operand planes in use
  // A fragments (weights) in a ring, requested AD taps ahead of their first product (round 5: one tap ahead -- 6 NT MFMAs, 192 NT
  // cycles -- does not cover an L2 round trip when a SIMD holds ONE wave with NT = 2: the 8^3 layers of a training batch of 8 took
  // 102 us for 36 us of matrix time)
  constexpr int AD = TERMS == SPLIT_BF16X6 ? 1 : SPLIT_TAPS_AD;  // (three operand planes: the deeper ring spills the 64-channel forms)
  u32x4 a_ring[AD + 1][3], bf[3][NT];
#pragma unroll
  for (int t = 0; t < AD; ++t)
#pragma unroll
    for (int s = 0; s < NP; ++s) a_ring[t][s] = wchunk[(size_t)t * wtap_stride + s * wsplit_stride];
  auto load_b = [&](int s, int toff) {
#pragma unroll
    for (int n = 0; n < NT; ++n) bf[s][n] = tile[(s * 2 + khalf) * PLANE + nbase[n] + toff];
  };
  if constexpr (TERMS == 6) load_b(2, 0);
  load_b(1, 0);
#pragma unroll
  for (int tap = 0; tap < CONV_NTAPS; ++tap) {
    const int toff = ((tap / 9) * HH + (tap / 3) % 3) * HW + tap % 3;
    const int toff_n = (((tap + 1) / 9) * HH + ((tap + 1) / 3) % 3) * HW + (tap + 1) % 3;
    const u32x4(&a_cur)[3] = a_ring[tap % (AD + 1)];
    auto mfma_term = [&](int pa, int pb) {
#pragma unroll
      for (int n = 0; n < NT; ++n)
        acc[n] = split_mfma<TERMS>(a_cur[pa], bf[pb][n], acc[n]);
    };
    if (tap + AD < CONV_NTAPS) {
#pragma unroll
      for (int s = 0; s < NP; ++s) a_ring[(tap + AD) % (AD + 1)][s] = wchunk[(size_t)(tap + AD) * wtap_stride + s * wsplit_stride];
    }
    load_b(0, toff);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (TERMS == 6) {
      mfma_term(0, 2);
      __builtin_amdgcn_sched_barrier(0);
      if (tap + 1 < CONV_NTAPS) load_b(2, toff_n);
      __builtin_amdgcn_sched_barrier(0);
      mfma_term(1, 1);
      mfma_term(2, 0);
      mfma_term(1, 0);
    }
    mfma_term(0, 1);
    __builtin_amdgcn_sched_barrier(0);
    if (tap + 1 < CONV_NTAPS) load_b(1, toff_n);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (TERMS != 6 && (X2W_KEEP_LOW_WEIGHT_PRODUCT || TERMS != SPLIT_F16X3)) mfma_term(1, 0);
    mfma_term(0, 0);
  }
}

// The tap loop of the PRE = true kernels (f16x3): split_taps' B schedule, with the A fragments (weights) in a ring of
// three tap slots loaded TWO taps ahead and carried across stages -- a[t % 3] is tap t's; on entry a[0], a[1] hold taps
// 0, 1 of this stage, on exit those of the next one (has_next). Memory returns are in order per wave, so the first A load
// issued behind the LDS-DMA burst of the next stage cannot return before that burst has landed: with two taps of weights
// already in registers the burst has two taps of MFMAs (>= 768 cycles) to do so. Weights come through a buffer descriptor:
// per-lane byte offset wv (one register) + a scalar offset per (stage, tap, plane) -- no 64-bit address per tap.
__device__ __forceinline__ u32x4 conv_wload(__amdgpu_buffer_rsrc_t rs, unsigned wv, unsigned so) {
  return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, wv, so, 0));
}
#ifndef CONV_PRE_AD
// taps of weight prefetch; the ring has CONV_PRE_AD + 1 slots, which must divide 27. Round 3 measured 8 against 2 at +-0 -- on one
// chain of 32 patches, two waves per SIMD. With the sampler's two chains of 16 the 8^3 layers launch 256 workgroups: ONE wave per
// SIMD with two tiles, 192 cycles of MFMAs per tap, and two taps of cover are less than an L2 round trip (what section 3.7 found in
// split_taps): 8 taps ahead, bench 223.1 -> 220.6 ms per sample call (profiles/r05b_conv_pre_ad8_ab.txt; 72 ring registers, none spilled)
#define CONV_PRE_AD 8
#endif
static_assert(27 % (CONV_PRE_AD + 1) == 0, "the ring position of tap 0 must be the same in every stage");
template <int NT, int HH, int HW, int PLANE>
__device__ __forceinline__ void split_taps_pre(f32x16 (&acc)[NT], const u32x4 *__restrict__ tile, __amdgpu_buffer_rsrc_t rsw,
                                               unsigned wv, unsigned sbase, unsigned stage_bytes, unsigned tap_bytes,
                                               unsigned plane_bytes, bool has_next, const int (&nbase)[NT], int khalf,
                                               u32x4 (&a)[CONV_PRE_AD + 1][2]) {
  // B fragments: plane 1 (h1) in one register set, plane 0 (h0) in TWO (tap parity): every ds_read_b128 is issued a full
  // eight MFMAs (>= 256 cycles) before its first use -- with a single h0 set its reads could only start once the
  // previous tap's last product had issued, four MFMAs (128 cycles, about one LDS latency under load) ahead of their use.
  //   tap t:  [A loads of tap t + AD]  G1: a0(t) x h1(t)  | read h1(t+1) |  G2: a1(t) x h0(t)  | read h0(t+1) |  G3: a0(t) x h0(t)
  // (same three products in the same order as split_taps: bit-identical accumulators)
  u32x4 b1[NT], b0[2][NT];
  auto load_b1 = [&](int toff) {
#pragma unroll
    for (int n = 0; n < NT; ++n) b1[n] = tile[(2 + khalf) * PLANE + nbase[n] + toff];
  };
  auto load_b0 = [&](int set, int toff) {
#pragma unroll
    for (int n = 0; n < NT; ++n) b0[set][n] = tile[khalf * PLANE + nbase[n] + toff];
  };
  load_b1(0);
  load_b0(0, 0);
#pragma unroll
  for (int tap = 0; tap < CONV_NTAPS; ++tap) {
    const int toff_n = (((tap + 1) / 9) * HH + ((tap + 1) / 3) % 3) * HW + (tap + 1) % 3;
    constexpr int AD = CONV_PRE_AD;
    const int cur = tap % (AD + 1), nx2 = (tap + AD) % (AD + 1), par = tap & 1;
    if (tap + AD < CONV_NTAPS) {
      const unsigned so = sbase + (unsigned)(tap + AD) * tap_bytes;
#pragma unroll
      for (int s = 0; s < 2; ++s) a[nx2][s] = conv_wload(rsw, wv, so + s * plane_bytes);
    } else if (has_next) {
      const unsigned so = sbase + stage_bytes + (unsigned)(tap + AD - CONV_NTAPS) * tap_bytes;
#pragma unroll
      for (int s = 0; s < 2; ++s) a[nx2][s] = conv_wload(rsw, wv, so + s * plane_bytes);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = split_mfma<SPLIT_F16X3>(a[cur][0], b1[n], acc[n]);
    __builtin_amdgcn_sched_barrier(0);
    if (tap + 1 < CONV_NTAPS) load_b1(toff_n);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int n = 0; n < NT; ++n)
      if (X2W_KEEP_LOW_WEIGHT_PRODUCT) acc[n] = split_mfma<SPLIT_F16X3>(a[cur][1], b0[par][n], acc[n]);
    __builtin_amdgcn_sched_barrier(0);
    if (tap + 1 < CONV_NTAPS) load_b0(par ^ 1, toff_n);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = split_mfma<SPLIT_F16X3>(a[cur][0], b0[par][n], acc[n]);
  }
}

// ---- pre-split operand grids ("S format", round 3) ---------------------------------------------------------------
// The staging phase of the split kernels -- load fp32, folded norm + Swish, fp16-pair split, LDS write, redone for every
// brick whose 6x10x10 halo holds the voxel (2.34 x) and for every output-channel block -- is half of their time on the
// f16x3 arithmetic. PRE = true kernels take the operand ALREADY transformed and split, in the exact byte layout of the LDS
// tile, and bring a stage into LDS with LDS-DMA (buffer_load_dwordx4 ... lds: no registers, no VALU, no ds_write):
//     S[b][voxel][chunk16][plane 2][khalf 2] of 16 bytes = 8 fp16  (h0 | h1 of 4 x value, channels chunk*16 + khalf*8 + i)
// i.e. 4 bytes per (voxel, channel) like the fp32 grid it replaces, channel count padded to a multiple of 16. (A PLANAR
// order [chunk][plane][khalf][voxel] -- 160-byte runs per DMA instruction instead of one cache line per lane -- was built
// and measured: the convolutions alone 6 % faster, the bench 1.4 % SLOWER, because both producers then write through an
// LDS transpose or read strided; profiles/README.md.) Producers:
// the voxeliser for a first convolution (voxel_gather.hip vox_gather_cl_split_kernel: no extra pass), conv3d_presplit_kernel for
// a second one (one elementwise pass over y1 once its GroupNorm statistics are folded). Same transform, same split, same
// products in the same order as the staging code below: outputs are bit-identical to the PRE = false kernels.
// The stage loop is double-buffered (2 x 37.5 KB, two workgroups per CU) with ONE barrier per stage: wait for my DMA of
// stage k, barrier, issue the DMA of stage k + 1 into the other buffer, 27 taps on buffer k. Halo slots outside the grid
// carry an out-of-range buffer offset: the hardware's zero lands in LDS.
#ifdef CONV_TIMELINE  // experiment builds only (tools/exp_conv_timeline.py): s_memtime stamps of one wave per workgroup
static __device__ unsigned long long *conv_tl_buf;  // (this object's copy; conv3d.hip has the setter: the f16x3 kernels are stamped)
#define CONV_TL_INIT const unsigned tl_lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z); int tl_n = 0;
#define CONV_TL(tid_) do { if ((tid_) == 0 && conv_tl_buf && tl_n < 15) conv_tl_buf[(size_t)tl_lin * 16 + 1 + tl_n++] = __builtin_readcyclecounter(); } while (0)
#define CONV_TL_AT(tid_, slot_) do { if ((tid_) == 0 && conv_tl_buf) conv_tl_buf[(size_t)tl_lin * 16 + 1 + (slot_)] = __builtin_readcyclecounter(); } while (0)
#define CONV_TL_ID(tid_) do { if ((tid_) == 0 && conv_tl_buf) conv_tl_buf[(size_t)tl_lin * 16] = ((unsigned long long)__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11)) << 32) | (unsigned)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11)); } while (0)
#else
#define CONV_TL_INIT
#define CONV_TL(tid_)
#define CONV_TL_AT(tid_, slot_)
#define CONV_TL_ID(tid_)
#endif
typedef int conv_i32x4 __attribute__((ext_vector_type(4)));
template <int R, int HD, int HH, int HW>
struct PreStage {
  static constexpr int PLANE = HD * HH * HW, NF = 4 * PLANE, NJ = (NF + 255) / 256;
  unsigned off[NJ];  // byte offset of (voxel, stage 0, quarter) from the sample's base; 0x80000000: outside the grid
  __device__ __forceinline__ void init(int tid, int d0, int h0, int w0, int nchunk) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int f = tid + j * 256;
      const int q = f / PLANE, e = f % PLANE;
      const int dz = e / (HH * HW), hy = (e / HW) % HH, wx = e % HW;
      const int d = d0 - 1 + dz, h = h0 - 1 + hy, w = w0 - 1 + wx;
      const bool ok = f < NF && (unsigned)d < (unsigned)R && (unsigned)h < (unsigned)R && (unsigned)w < (unsigned)R;
      off[j] = ok ? ((unsigned)((d * R + h) * R + w) * (unsigned)(nchunk * 4) + (unsigned)q) * 16u : 0x80000000u;
    }
  }
  // stage `chunk` of the sample behind rs -> buf[0 .. NF); every wave issues its 64-slot runs (lane l lands at run + l).
  // Issued as inline assembly ON PURPOSE: the compiler's wait-count pass assumes that any ds_read may alias the
  // destination of an LDS-DMA it knows of and puts `s_waitcnt vmcnt(0)` in front of the first fragment read after the
  // burst -- which serialises the DMA of stage k + 1 with the taps of stage k (separate __shared__ objects do not help
  // with this compiler). The hand-written form is invisible to that pass; the kernel orders it itself: the builtin
  // s_waitcnt vmcnt(0) + barrier at the top of the next stage. (The pass's own waits for the weight loads it DOES know of
  // can only be stricter than needed: per-wave memory returns are in order.)
  __device__ __forceinline__ void issue(conv_i32x4 rs, int chunk, u32x4 *buf, int tid) const {
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const unsigned base = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) void *)buf);
    const unsigned so = (unsigned)chunk * 64u;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int f0 = j * 256 + wave * 64;  // wave-uniform
      if (f0 < NF) {
        const unsigned m0v = base + (unsigned)f0 * 16u;
        if (f0 + lane < NF)
          asm volatile("s_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %2 offen lds"
                       :
                       : "v"(off[j]), "s"(rs), "s"(so), "s"(m0v)
                       : "memory");  // (m0 is a reserved register: the compiler does not track it as a clobber -- and uses it nowhere in this
                                     //  object, tools/disasm.sh conv3d: every m0 reference is one of these s_mov_b32)
      }
    }
  }
};
// buffer descriptor words for the inline-assembly DMA above (what __builtin_amdgcn_make_buffer_rsrc(p, 0, bytes, 0x00020000)
// builds), forced into scalar registers
__device__ __forceinline__ conv_i32x4 conv_make_rsrc(const void *p, unsigned bytes) {
  const unsigned long long a = (unsigned long long)p;
  conv_i32x4 r;
  r[0] = __builtin_amdgcn_readfirstlane((int)(unsigned)a);
  r[1] = __builtin_amdgcn_readfirstlane((int)((unsigned)(a >> 32) & 0xffffu));
  r[2] = __builtin_amdgcn_readfirstlane((int)bytes);
  r[3] = 0x00020000;
  return r;
}

#ifndef CONV_F16_WAVES
#define CONV_F16_WAVES 2  // (waves per SIMD the f16x3 forms are compiled for; their two-plane tile would fit three workgroups)
#endif
template <int R, bool COMPACT, int MT, bool XF, bool CL, int TERMS, bool PRE = false>
__global__ __launch_bounds__(256, TERMS == SPLIT_F16X3 ? CONV_F16_WAVES : 2) void conv3d_k3_split_kernel(int cin, int cout, int nchunk, int cout_pad,
                                                             const float *__restrict__ in,
                                                             const unsigned short *__restrict__ wt,
                                                             const float *__restrict__ bias,
                                                             const float *__restrict__ out_class,
                                                             const float *__restrict__ in_scale,
                                                             const float *__restrict__ in_shift, int in_swish,
                                                             const float *__restrict__ in_sub, int skip_zero,
                                                             const int *__restrict__ brick_list,
                                                             const int *__restrict__ brick_count,
                                                             float *__restrict__ out, float *__restrict__ stats_part) {
  using G = SplitGeom<R>;
  constexpr int HD = G::TD + 2, HH = G::TH + 2, HW = G::TW + 2;
  constexpr int PLANE = HD * HH * HW;
  constexpr int NTILES = (G::TD * G::TH * G::TW) / 32;
  constexpr int BH = R / G::TH, BW = R / G::TW;
  constexpr int R3 = R * R * R;
  // tile[split][khalf][voxel] : 8 bf16 (16 bytes) = channels khalf*8 .. khalf*8+7 of the staged chunk (PRE: two buffers)
  static_assert(!PRE || (TERMS == SPLIT_F16X3 && !XF && CL), "pre-split operands: f16x3, voxel-major, transform applied");
  __shared__ u32x4 tile[split_planes(TERMS) * 2 * PLANE];
  // (PRE: the second stage buffer is its OWN object, and the stage loop is unrolled by two with the roles fixed, so that
  //  the compiler can tell the LDS-DMA into one buffer from the fragment reads of the other -- with one array it waits
  //  vmcnt(0) for the DMA burst of stage k + 1 in front of the first ds_read of stage k)
  __shared__ u32x4 tile2[PRE ? split_planes(TERMS) * 2 * PLANE : 1];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, khalf = lane >> 5;
  constexpr int BD = R / G::TD;
  constexpr int NBRICK = BD * BH * BW;
  // Workgroup -> (sample, brick, channel block). The hardware deals workgroups to the 8 XCDs round-robin in launch
  // order (id mod 8), and every XCD has its own 4 MB L2. The launch id is therefore re-read as (xcd, j) and XCD x is
  // given the x-th CONTIGUOUS eighth of the work list, ordered (sample, brick, channel block): the bricks of a
  // sample -- whose 6x10x10 halos overlap 2.34x -- and both channel blocks of a brick then share one L2.
  const unsigned lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  const unsigned nblk = gridDim.x * gridDim.y * gridDim.z;
  const int ncoblk = (cout + 32 * MT - 1) / (32 * MT);
  int bd, bh, bw, b, coblk;
  if (brick_list) {  // compacted list of ACTIVE (sample, brick) pairs; the rest is written by conv3d_fill_kernel
    const unsigned total = (unsigned)(*brick_count) * ncoblk;
    unsigned v = lin;
    if (nblk % 8 == 0) {
      const unsigned per = (total + 7) / 8;
      if (lin / 8 >= per) return;
      v = (lin % 8) * per + lin / 8;
    }
    if (v >= total) return;
    const int entry = brick_list[v / ncoblk];
    coblk = v % ncoblk;
    b = entry / NBRICK;
    const int bk = entry % NBRICK;
    bd = bk / (BH * BW);
    bh = (bk / BW) % BH;
    bw = bk % BW;
  } else {
    const unsigned v = nblk % 8 == 0 ? (lin % 8) * (nblk / 8) + lin / 8 : lin;
    const unsigned per_sample = NBRICK * ncoblk;
    b = v / per_sample;
    const unsigned rem = v % per_sample;
    const int bk = rem / ncoblk;
    coblk = rem % ncoblk;
    bd = bk / (BH * BW);
    bh = (bk / BW) % BH;
    bw = bk % BW;
  }
  const int brick = (bd * BH + bh) * BW + bw;
  const int d0 = bd * G::TD, h0 = bh * G::TH, w0 = bw * G::TW;
  // waves as WM x WN: every wave owns ONE 32-channel M-tile and NT N-tiles of the brick. With 64 channels per
  // workgroup (MT = 2) that is 2 x 2 waves of 4 N-tiles each: an A fragment (weights, a 16-byte L1/L2 load
  // per lane) then feeds four N-tiles instead of two -- measured, the A stream through the L1 is what bounds
  // this kernel (removing it: 179 -> 230 TFLOP/s), while B fragments come from LDS, which has room.
  constexpr int WM = MT, WN = 4 / WM, NT = (NTILES / WN) > 0 ? NTILES / WN : 1;
  const int wm = wave / WN, wn = wave % WN;
  const int co0 = coblk * (32 * MT) + 32 * wm;

  int nbase[NT];
  bool nact[NT];
#pragma unroll
  for (int s = 0; s < NT; ++s) {
    const int t = NT * wn + s;
    nact[s] = t < NTILES;
    constexpr int HB = G::TH / G::NH;
    const int td = (t / HB) * G::ND, th = (t % HB) * G::NH;
    const int jw = lane_w<G::TW>(l31), jr = l31 / G::TW;
    const int jh = jr % G::NH, jd = jr / G::NH;
    nbase[s] = ((td + jd) * HH + (th + jh)) * HW + jw;
  }

  f32x16 acc[NT];
#pragma unroll
  for (int s = 0; s < NT; ++s)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[s][r] = 0.0f;
  // The epilogue's additive constants are fetched HERE, sixteen loads in one batch under the stage loop. Left inside the
  // epilogue's (branchy) row loop the compiler issued them one at a time, each followed by its own vmcnt(0): sixteen
  // serialised L2 round trips per wave, 64 more for the boundary-class constants of a second convolution -- a timeline of
  // the r = 32 C64 launch (tools/exp_conv_timeline.py) showed 43 k of a workgroup's 144 k cycles in the epilogue.
  float bvr[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int co = co0 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
    bvr[r] = (co < cout && !out_class) ? bias[co] : 0.0f;
  }

  if constexpr (PRE) {
    // `in` = the pre-split operand grid (S format): LDS-DMA stages, two buffers, one barrier per stage
    CONV_TL_INIT
    CONV_TL_ID(tid);
    CONV_TL(tid);  // 0: start (after the index arithmetic above)
    PreStage<R, HD, HH, HW> ps;
    ps.init(tid, d0, h0, w0, nchunk);
    const conv_i32x4 sg = conv_make_rsrc((const u32x4 *)in + (size_t)b * R3 * nchunk * 4, (unsigned)(R3 * nchunk * 64));
    ps.issue(sg, 0, tile, tid);
    CONV_TL(tid);  // 1: first DMA issued
    // weights: [tap][stage][plane 3][khalf 2][cout_pad] of 16 bytes
    const unsigned stage_bytes = 6u * cout_pad * 16u, tap_bytes = (unsigned)nchunk * stage_bytes, plane_bytes = 2u * cout_pad * 16u;
    auto rsw = __builtin_amdgcn_make_buffer_rsrc((void *)wt, 0, 27 * (int)tap_bytes, 0x00020000);
    const unsigned wv = (unsigned)(khalf * cout_pad + co0 + l31) * 16u;
    u32x4 aring[CONV_PRE_AD + 1][2];
#pragma unroll
    for (int t = 0; t < CONV_PRE_AD; ++t)
#pragma unroll
      for (int s = 0; s < 2; ++s) aring[t][s] = conv_wload(rsw, wv, t * tap_bytes + s * plane_bytes);
    auto stage = [&](int k, const u32x4 *cur, u32x4 *nxt) {
      __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0): my share of stage k has landed (and the weights of its first taps)
      __syncthreads();                     // everyone's has; the other buffer is no longer read
      CONV_TL(tid);  // 2 + 2k: stage k released
      if (k + 1 < nchunk) ps.issue(sg, k + 1, nxt, tid);
      split_taps_pre<NT, HH, HW, PLANE>(acc, cur, rsw, wv, (unsigned)k * stage_bytes, stage_bytes, tap_bytes, plane_bytes,
                                        k + 1 < nchunk, nbase, khalf, aring);
      CONV_TL(tid);  // 3 + 2k: taps of stage k issued
    };
    for (int k = 0; k < nchunk; k += 2) {
      stage(k, tile, tile2);
      if (k + 1 < nchunk) stage(k + 1, tile2, tile);
    }
#ifdef CONV_TIMELINE
    __builtin_amdgcn_s_waitcnt(0x0f70);
    if (tid == 0 && conv_tl_buf) conv_tl_buf[(size_t)tl_lin * 16 + 14] = __builtin_readcyclecounter();  // 14: accumulators final
#endif
  } else {
  constexpr int NP = (PLANE + 255) / 256;
  int soff[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int e = tid + j * 256;
    const int dz = e / (HH * HW), hy = (e / HW) % HH, wx = e % HW;
    const int d = d0 - 1 + dz, h = h0 - 1 + hy, w = w0 - 1 + wx;
    const bool ok = e < PLANE && (unsigned)d < (unsigned)R && (unsigned)h < (unsigned)R && (unsigned)w < (unsigned)R;
    soff[j] = ok ? (d * R + h) * R + w : -1;
  }

  const float *inb = in + (size_t)b * cin * R3;
  float stg[CONV_SCK][NP];
  // unpredicated loads through scalar descriptors; halo positions outside the grid carry an out-of-range offset
  // and read the hardware's zero. Channel-major (reference) layout: one descriptor per channel row (rows past cin
  // are clamped and zeroed at staging time). Voxel-major layout (CL): a staged voxel's channels are contiguous,
  // 64 bytes per stage = 16-byte loads when cin % 4 == 0 (quads past cin are zeroed at staging time).
  unsigned voff[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j)
    voff[j] = soff[j] >= 0 ? (unsigned)soff[j] * (CL ? (unsigned)cin * 4u : 4u) : 0x80000000u;
  auto stage_load = [&](int ci0) {
    if (CL) {
      auto rs = __builtin_amdgcn_make_buffer_rsrc((void *)inb, 0, R3 * cin * 4, 0x00020000);
      if ((cin & 3) == 0) {
#pragma unroll
        for (int j = 0; j < NP; ++j)
#pragma unroll
          for (int q = 0; q < CONV_SCK / 4; ++q) {
            const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff[j] + (unsigned)(ci0 + 4 * q) * 4u, 0, 0));
#pragma unroll
            for (int i = 0; i < 4; ++i) stg[4 * q + i][j] = v[i];
          }
      } else {
#pragma unroll
        for (int j = 0; j < NP; ++j)
#pragma unroll
          for (int c = 0; c < CONV_SCK; ++c)
            stg[c][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, voff[j] + (unsigned)(ci0 + c) * 4u, 0, 0));
      }
    } else {
#pragma unroll
      for (int c = 0; c < CONV_SCK; ++c) {
        auto rs = __builtin_amdgcn_make_buffer_rsrc((void *)(inb + (size_t)min(ci0 + c, cin - 1) * R3), 0, R3 * 4, 0x00020000);
#pragma unroll
        for (int j = 0; j < NP; ++j) stg[c][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, voff[j], 0, 0));
      }
    }
  };
  stage_load(0);

  for (int ci0 = 0; ci0 < cin; ci0 += CONV_SCK) {
    __syncthreads();
    int nonzero = 0;
#pragma unroll
    for (int c = 0; c < CONV_SCK; ++c) {
      float sc = 1.0f, sh = 0.0f, sub = 0.0f;
      const bool cok = ci0 + c < cin;
      if (XF && cok) {
        sc = in_scale[b * cin + ci0 + c];  // (wave-uniform: through the scalar cache)
        sh = in_shift[b * cin + ci0 + c];
        if (in_sub) sub = in_sub[b * cin + ci0 + c];
      }
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        float v = cok ? stg[c][j] : 0.0f;
        if (XF && cok && soff[j] >= 0) v = xf_apply(v, sc, sh, in_swish) - sub;
        nonzero |= (v != 0.0f);
        stg[c][j] = v;
      }
    }
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const int e = tid + j * 256;
      if (e < PLANE) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          u32x4 q[3];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            unsigned p0, p1, p2;
            split_pair<TERMS>(stg[h * 8 + 2 * i][j], stg[h * 8 + 2 * i + 1][j], p0, p1, p2);
            q[0][i] = p0;
            q[1][i] = p1;
            q[2][i] = p2;
          }
#pragma unroll
          for (int s = 0; s < split_planes(TERMS); ++s) tile[(s * 2 + h) * PLANE + e] = q[s];
        }
      }
    }
    const int any = skip_zero ? __syncthreads_or(nonzero) : (__syncthreads(), 1);
    if (ci0 + CONV_SCK < cin) {  // next stage's loads fly during the MFMAs
      int nxt = ci0 + CONV_SCK;
      asm volatile("" : "+s"(nxt));  // opaque: unpredicated loads would otherwise be hoisted above the staging phase
      stage_load(nxt);
    }
    if (!any) continue;

    const u32x4 *wchunk = (const u32x4 *)wt + (((size_t)(ci0 / CONV_SCK) * 3) * 2 + khalf) * cout_pad + co0 + l31;
    const size_t wsplit_stride = (size_t)2 * cout_pad, wtap_stride = (size_t)nchunk * 3 * 2 * cout_pad;
    split_taps<NT, HH, HW, PLANE, TERMS>(acc, tile, wchunk, wsplit_stride, wtap_stride, nbase, khalf);
  }
  }  // !PRE
  if constexpr (TERMS == SPLIT_F16X3) {  // 1 / (S_x S_w): a power of two stored behind the pack
    const float oscale = ((const float *)((const char *)wt + conv_split_trailer_bytes(nchunk, cout_pad)))[1];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[n][r] *= oscale;
  }

  float *outb = out + (size_t)b * cout * R3;
  // boundary-class constants of a second convolution: the workgroup's [27][32 MT] slice of K[b] goes through LDS (the
  // operand tile is free now) -- one cooperative fetch instead of a dependent global load per (row, N-tile)
  constexpr int NCW = 32 * MT;
  float *kl = (float *)tile;
  if (out_class) {
    __syncthreads();  // every wave is done with the last stage's fragments
    const float *kb = out_class + (size_t)b * 27 * cout;
    const int cob = co0 - 32 * wm;
    for (int e = tid; e < 27 * NCW; e += 256) {
      const int c = e % NCW, co = cob + c;
      kl[e] = co < cout ? kb[(e / NCW) * cout + co] : 0.0f;
    }
    __syncthreads();
  }
  int vox[NT], cls[NT];
#pragma unroll
  for (int s = 0; s < NT; ++s) {
    const int t = NT * wn + s;
    constexpr int HB = G::TH / G::NH;
    const int td = (t / HB) * G::ND, th = (t % HB) * G::NH;
    const int jw = lane_w<G::TW>(l31), jr = l31 / G::TW;
    const int d = d0 + td + jr / G::NH, h = h0 + th + jr % G::NH, w = w0 + jw;
    vox[s] = (d * R + h) * R + w;
    const int cd = d == 0 ? 0 : (d == R - 1 ? 2 : 1), ch = h == 0 ? 0 : (h == R - 1 ? 2 : 1),
              cw = w == 0 ? 0 : (w == R - 1 ? 2 : 1);
    cls[s] = (cd * 3 + ch) * 3 + cw;
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    float vv[NT][4];  // voxel-major stores: the four consecutive channels of register group g, per N-tile
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 4 * g + i;
      const int co = co0 + i + 8 * g + 4 * khalf;
      const bool cok = co < cout;
      const float bv = bvr[r];
      float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
      for (int s = 0; s < NT; ++s) {
        if (!nact[s]) continue;
        float v = acc[s][r] + bv;
        if (out_class && cok) v += kl[cls[s] * NCW + 32 * wm + i + 8 * g + 4 * khalf];
        if (CL) vv[s][i] = v;
        else if (cok) outb[(size_t)co * R3 + vox[s]] = v;
        s1 += v;
        s2 += v * v;
      }
      if (stats_part) {
        // the brick's four statistics slots: wave column wn fills slot wn for its channels; with two wave rows
        // only two columns exist and slots 2, 3 are zeroed
        s1 = halfwave_sum_to_last(s1);
        s2 = halfwave_sum_to_last(s2);
        if (l31 == 31 && cok) {
          float *p = stats_part + ((((size_t)b * NBRICK + brick) * 4 + wn) * cout + co) * 2;
          p[0] = s1;
          p[1] = s2;
          if (WN < 4) {
            float *z = stats_part + ((((size_t)b * NBRICK + brick) * 4 + WN + wn) * cout + co) * 2;
            z[0] = 0.0f;
            z[1] = 0.0f;
          }
        }
      }
    }
    if (CL) {
      const int cq = co0 + 8 * g + 4 * khalf;
#pragma unroll
      for (int s = 0; s < NT; ++s) {
        if (!nact[s]) continue;
        float *q = outb + (size_t)vox[s] * cout + cq;
        if (cq + 3 < cout && (cout & 3) == 0) *(f32x4 *)q = f32x4{vv[s][0], vv[s][1], vv[s][2], vv[s][3]};
        else
          for (int i = 0; i < 4; ++i)
            if (cq + i < cout) q[i] = vv[s][i];
      }
    }
  }
#ifdef CONV_TIMELINE
  if constexpr (PRE) {
    __builtin_amdgcn_s_waitcnt(0x0f70);
    if (tid == 0 && conv_tl_buf)  // 15: epilogue stores issued and acknowledged
      conv_tl_buf[(size_t)(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z)) * 16 + 15] = __builtin_readcyclecounter();
  }
#endif
}

// ---- launch. PRE kernels take no skip flag: a pre-split stage is brought in whole
template <int R, int MT, bool XF, bool CL, int TERMS, bool PRE>
static int conv_split_go(const ConvArgs &a) {
  const int nchunk = (a.cin + CONV_SCK - 1) / CONV_SCK, cout_pad = (a.cout + 63) / 64 * 64;
  dim3 grid(conv_bricks(R), (a.cout + 32 * MT - 1) / (32 * MT), a.b);
  if (a.brick_list) grid = dim3(conv_bricks(R) * a.b, (a.cout + 32 * MT - 1) / (32 * MT), 1);
  hipLaunchKernelGGL((conv3d_k3_split_kernel<R, true, MT, XF, CL, TERMS, PRE>), grid, dim3(256), 0, a.s, a.cin, a.cout, nchunk,
                     cout_pad, a.in, (const unsigned short *)a.wt, a.bias, a.out_class, a.in_scale, a.in_shift, a.in_swish, a.in_sub,
                     PRE ? 0 : a.skip_zero, a.brick_list, a.brick_count, a.out, a.stats_part);
  return p2pb_launch_status();
}
template <int R, int MT, int TERMS>
static int conv_split_form(const ConvArgs &a) {
  if (a.pre) {  // `in` is the pre-split operand grid (S format): f16x3, voxel-major, transform already applied
    if constexpr (TERMS == SPLIT_F16X3 && R >= 8) {
      if (!a.cl || a.in_scale || a.in_sub) return P2PB_EINVAL;
      return conv_split_go<R, MT, false, true, TERMS, true>(a);
    }
    return P2PB_EINVAL;
  }
  if constexpr (TERMS == SPLIT_BF16X3) {  // the training data gradient's form only: plain operand, channel-major
    if (a.in_scale != nullptr || a.cl) return P2PB_EINVAL;
    return conv_split_go<R, MT, false, false, TERMS, false>(a);
  } else {
    return for_flag(a.in_scale != nullptr, [&](auto XF) {
      return for_flag(a.cl, [&](auto CL) { return conv_split_go<R, MT, decltype(XF)::value, decltype(CL)::value, TERMS, false>(a); });
    });
  }
}
// r in {4, 8, 16, 32} (else P2PB_EINVAL), mt = 32-channel tiles (= wave rows) per workgroup, 1 or 2
template <int TERMS>
static int conv_split_launch(int r, int mt, const ConvArgs &a) {
  return for_value<32, 16, 8, 4>(r, [&](auto R) {
    return mt == 2 ? conv_split_form<decltype(R)::value, 2, TERMS>(a) : conv_split_form<decltype(R)::value, 1, TERMS>(a);
  });
}
