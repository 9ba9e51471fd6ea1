// devoxelize.hip -- trilinear devoxelize for gfx950.
//   p2pb_trilinear_devoxelize_forward / _affine  (PN2/trilinear_devox_gpu.cu:21; its backward pass: scatter_grad.hip)
//   p2pb_trilinear_devoxelize_cl_affine          the voxel-major form of the fused inference branch (see voxel_gather.hip)
#include "voxel_common.h"

struct Corners {
  int idx[8];
  float w[8];
};

__device__ __forceinline__ Corners devox_corners(float x, float y, float z, int r) {
  Corners k;
  const int r2 = r * r;
  const float xl = floorf(x), yl = floorf(y), zl = floorf(z);
  const float xd1 = x - xl, yd1 = y - yl, zd1 = z - zl;
  const float xd0 = 1.0f - xd1, yd0 = 1.0f - yd1, zd0 = 1.0f - zd1;
  k.w[0] = xd0 * yd0 * zd0;
  k.w[1] = xd0 * yd0 * zd1;
  k.w[2] = xd0 * yd1 * zd0;
  k.w[3] = xd0 * yd1 * zd1;
  k.w[4] = xd1 * yd0 * zd0;
  k.w[5] = xd1 * yd0 * zd1;
  k.w[6] = xd1 * yd1 * zd0;
  k.w[7] = xd1 * yd1 * zd1;
  const int xlo = (int)xl, ylo = (int)yl, zlo = (int)zl;
  const int xhi = (xd1 > 0) ? -1 : 0, yhi = (yd1 > 0) ? -1 : 0, zhi = (zd1 > 0) ? 1 : 0;
  k.idx[0] = xlo * r2 + ylo * r + zlo;
  k.idx[1] = k.idx[0] + zhi;
  k.idx[2] = k.idx[0] + (yhi & r);
  k.idx[3] = k.idx[2] + zhi;
  k.idx[4] = k.idx[0] + (xhi & r2);
  k.idx[5] = k.idx[4] + zhi;
  k.idx[6] = k.idx[4] + (yhi & r);
  k.idx[7] = k.idx[6] + zhi;
  return k;
}

// AFF: the grid holds the RAW second-convolution output; the per-(sample, channel) affine that stands for
// AdaGN + SE gating (feat*A + B) is applied to each corner value before interpolating, i.e. the same
// "transform, then interpolate" order as the unfused graph, without a pass over the grid in between.
template <int CC, bool AFF>
__global__ __launch_bounds__(256) void devox_kernel(int c, int n, int r, int training,
                                                    const float *__restrict__ coords, const float *__restrict__ feat,
                                                    const float *__restrict__ aff_a, const float *__restrict__ aff_b,
                                                    int *__restrict__ inds, float *__restrict__ wgts,
                                                    float *__restrict__ outs) {
  const int b = blockIdx.z;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int r3 = r * r * r;
  const float *co = coords + (size_t)b * 3 * n;
  const Corners k = devox_corners(co[i], co[i + n], co[i + 2 * n], r);
  if (training && blockIdx.y == 0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      wgts[(size_t)b * 8 * n + (size_t)q * n + i] = k.w[q];
      inds[(size_t)b * 8 * n + (size_t)q * n + i] = k.idx[q];
    }
  }
  const int c0 = blockIdx.y * CC, c1 = min(c0 + CC, c);
  const float *f = feat + (size_t)b * c * r3;
  float *o = outs + (size_t)b * c * n + i;
  for (int j = c0; j < c1; ++j) {
    const float *fj = f + (size_t)j * r3;
    float fv[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) fv[q] = fj[k.idx[q]];
    if (AFF) {
      const float a = aff_a[(size_t)b * c + j], bb = aff_b[(size_t)b * c + j];
#pragma unroll
      for (int q = 0; q < 8; ++q) fv[q] = fv[q] * a + bb;
    }
    float acc = k.w[0] * fv[0];
#pragma unroll
    for (int q = 1; q < 8; ++q) acc = __fmaf_rn(k.w[q], fv[q], acc);
    o[(size_t)j * n] = acc;
  }
}

extern "C" int p2pb_trilinear_devoxelize_forward(int b, int c, int n, int r, int is_training, const float *coords,
                                                 const float *feat, int *inds, float *wgts, float *outs,
                                                 void *stream) {
  if (b <= 0 || c <= 0 || n <= 0 || r <= 0) return P2PB_EINVAL;
  if (is_training && (!inds || !wgts)) return P2PB_EINVAL;
  constexpr int CC = 16;
  hipLaunchKernelGGL((devox_kernel<CC, false>), dim3(cdiv(n, 256), cdiv(c, CC), b), dim3(256), 0, (hipStream_t)stream,
                     c, n, r, is_training, coords, feat, (const float *)nullptr, (const float *)nullptr, inds, wgts,
                     outs);
  return p2pb_launch_status();
}

// inference-only fused form: outs[b,c,i] = sum_k w_k * (feat[b,c,idx_k] * aff_a[b,c] + aff_b[b,c])
extern "C" int p2pb_trilinear_devoxelize_affine(int b, int c, int n, int r, const float *coords, const float *feat,
                                                const float *aff_a, const float *aff_b, float *outs, void *stream) {
  if (b <= 0 || c <= 0 || n <= 0 || r <= 0 || !aff_a || !aff_b) return P2PB_EINVAL;
  constexpr int CC = 16;
  hipLaunchKernelGGL((devox_kernel<CC, true>), dim3(cdiv(n, 256), cdiv(c, CC), b), dim3(256), 0, (hipStream_t)stream,
                     c, n, r, 0, coords, feat, aff_a, aff_b, (int *)nullptr, (float *)nullptr, outs);
  return p2pb_launch_status();
}

// ------------------------------------------------------------------------------------------------
// voxel-major grid f32[b, r^3, c] -> outs f32[b, c, n] = sum_k w_k * (grid[idx_k]*aff_a + aff_b)
// add (optional, f32[b,c,n]) with add_scale/add_shift f32[b,c]: outs += swish(add*add_scale + add_shift) -- PVConv's
// point branch (conv -> norm -> Swish, models/pvcnn.py:286,325) joined to the voxel branch in the same pass.
// A workgroup owns 64 points x one 64-channel chunk: corners staged in LDS (devox_stage_corners), the gather of the corner
// rows into tile[channel][point] (two forms below), then the transposed write-back (devox_write_back).
// ------------------------------------------------------------------------------------------------

// Every wave stages the trilinear corners of ITS OWN 16 points (lanes 0..15) of the workgroup's 64 (from p0; clamped to
// n - 1), with 16-byte LDS stores only. Ends with the barrier that publishes sidx / sw. lane, wave: the caller's t & 63 and
// t >> 6, passed in -- derived from threadIdx here, the compiler folds wave * 16 on its own before it meets the caller's uses of
// `wave`, and the kernels' prologues come out in another order than with the staging written in place.
// Round 4: the first form -- wave 0 staged all 64 points and the compiler merged a row's eight stores into ds_write_b96 +
// ds_write2_b32 + ds_write_b32 -- returned wrong values for wave 3's points when a matrix kernel of ANOTHER stream shared the CU
// (the two-chain sampler: 10-15 % of such launches had one wave's 16 points x 64 channels off by O(1); alone, or beside
// element-wise kernels, never; tools/dbg/devox_conc.py). Either change alone removes it (own points: 0 of 90 launches
// wrong; 16-byte stores: 0 of 90 as flat_store_dwordx4 -- what a volatile store through a generic pointer compiles to -- and
// 0 of 270 as the ds_write_b128 below); ds_write_b96 is not used anywhere in this library any more.
__device__ __forceinline__ void devox_stage_corners(int (&sidx)[64][8], float (&sw)[64][8], const float *coords,
                                                    int b, int n, int r, int p0, int lane, int wave) {
  if (lane < 16) {
    const int tt = wave * 16 + lane;
    const int i = min(p0 + tt, n - 1);
    const float *co = coords + (size_t)b * 3 * n;
    const Corners k = devox_corners(co[i], co[i + n], co[i + 2 * n], r);
    *(volatile P2PB_LDS i32x4 *)&sidx[tt][0] = i32x4{k.idx[0], k.idx[1], k.idx[2], k.idx[3]};
    *(volatile P2PB_LDS i32x4 *)&sidx[tt][4] = i32x4{k.idx[4], k.idx[5], k.idx[6], k.idx[7]};
    *(volatile P2PB_LDS f32x4 *)&sw[tt][0] = f32x4{k.w[0], k.w[1], k.w[2], k.w[3]};
    *(volatile P2PB_LDS f32x4 *)&sw[tt][4] = f32x4{k.w[4], k.w[5], k.w[6], k.w[7]};
  }
  __syncthreads();
}

// tile[channel][point] -> outs[b, c0 + channel, p0 + point] (+ the point branch): a thread writes point t & 63 of 16 rows.
// The point branch's values for the thread's 16 rows (`add`, and the row's scale / shift) are loaded here, all at once and from
// clamped addresses (rows >= c, points >= n), while the waves meet at the barrier behind the gather: loaded inside the
// write-back loop each row's three were waited for (vmcnt(0)) before the next row's were issued, sixteen L2 round trips behind
// the LDS transpose (profiles/r07_gather_wait_audit.txt).
// RAGGED: the chunk may end before 64 channels (rows >= c are clamped, then skipped); else c % 64 == 0. t: the caller's
// thread index (as for devox_stage_corners); `row` is spelled as each kernel had it (the whole-chunk form adds in 64 bits).
template <bool RAGGED>
__device__ __forceinline__ void devox_write_back(const float (&tile)[64][65], int c, int n, int b, int c0, int p0, int t,
                                                 const float *add, const float *add_scale,
                                                 const float *add_shift, float *outs) {
  const int pt = t & 63;
  float hv[16], hsc[16], hsh[16];
  if (add) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const size_t row = RAGGED ? (size_t)b * c + min(c0 + (t >> 6) + 4 * k, c - 1) : (size_t)b * c + c0 + (t >> 6) + 4 * k;
      hv[k] = add[row * n + min(p0 + pt, n - 1)];
      hsc[k] = add_scale[row];
      hsh[k] = add_shift[row];
    }
  }
  __syncthreads();
  if (p0 + pt < n) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int cr = (t >> 6) + 4 * k;
      if (!RAGGED || c0 + cr < c) {
        const size_t o = ((size_t)b * c + c0 + cr) * n + p0 + pt;
        float v = tile[cr][pt];
        if (add) {
          const float z = hv[k] * hsc[k] + hsh[k];
          v = z * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(z * -1.44269504088896340736f)) + v;
        }
        outs[o] = v;
      }
    }
  }
}

// 4-byte gathers: lane = channel of the chunk, a wave walks its 16 points; any c
__global__ __launch_bounds__(256) void devox_cl_kernel(int c, int n, int r, const float *__restrict__ coords,
                                                       const float *__restrict__ grid, const float *__restrict__ aff_a,
                                                       const float *__restrict__ aff_b, const float *__restrict__ add,
                                                       const float *__restrict__ add_scale,
                                                       const float *__restrict__ add_shift, float *__restrict__ outs) {
  __shared__ float tile[64][65];  // [channel][point]
  __shared__ __attribute__((aligned(16))) int sidx[64][8];
  __shared__ __attribute__((aligned(16))) float sw[64][8];
  const int b = blockIdx.z, p0 = blockIdx.x * 64, t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int r3 = r * r * r;
  devox_stage_corners(sidx, sw, coords, b, n, r, p0, lane, wave);
  const float *g = grid + (size_t)b * r3 * c;
  const int c0 = blockIdx.y * 64;  // one 64-channel chunk per workgroup
  const int ch = c0 + lane;
  if (ch < c) {
    const float a = aff_a ? aff_a[(size_t)b * c + ch] : 1.0f, bb = aff_b ? aff_b[(size_t)b * c + ch] : 0.0f;
    // (the corner rows of two points per batch: left to the unroller, one point's eight loads were waited for before the next
    // point's were issued, sixteen round trips for the wave's sixteen points)
    for (int pl0 = wave * 16; pl0 < wave * 16 + 16; pl0 += 2) {
      float fv[2][8];
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int q = 0; q < 8; ++q) fv[u][q] = g[(size_t)sidx[pl0 + u][q] * c + ch];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int pl = pl0 + u;
        if (aff_a) {
#pragma unroll
          for (int q = 0; q < 8; ++q) fv[u][q] = fv[u][q] * a + bb;
        }
        float acc = sw[pl][0] * fv[u][0];
#pragma unroll
        for (int q = 1; q < 8; ++q) acc = __fmaf_rn(sw[pl][q], fv[u][q], acc);
        tile[lane][pl] = acc;
      }
    }
  }
  devox_write_back<true>(tile, c, n, b, c0, p0, t, add, add_scale, add_shift, outs);
}

// the same pass with 16-byte gathers (round 5, last session): a lane owns FOUR channels of one point -- 16 lanes cover the 64-channel
// chunk, a wave instruction fetches the corner rows of four points -- a quarter of the load instructions for the same bytes; every
// (point, channel) value goes through the same multiplies and fused adds in the same order: bit-identical. c % 64 == 0.
__global__ __launch_bounds__(256) void devox_cl4_kernel(int c, int n, int r, const float *__restrict__ coords,
                                                        const float *__restrict__ grid, const float *__restrict__ aff_a,
                                                        const float *__restrict__ aff_b, const float *__restrict__ add,
                                                        const float *__restrict__ add_scale,
                                                        const float *__restrict__ add_shift, float *__restrict__ outs) {
  __shared__ float tile[64][65];  // [channel][point]
  __shared__ __attribute__((aligned(16))) int sidx[64][8];
  __shared__ __attribute__((aligned(16))) float sw[64][8];
  const int b = blockIdx.z, p0 = blockIdx.x * 64, t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int r3 = r * r * r;
  devox_stage_corners(sidx, sw, coords, b, n, r, p0, lane, wave);
  const float *g = grid + (size_t)b * r3 * c;
  const int c0 = blockIdx.y * 64;
  {
    const int cq = lane & 15, ps = lane >> 4;
    const int ch4 = c0 + 4 * cq;
    f32x4 a4 = {1.0f, 1.0f, 1.0f, 1.0f}, b4 = {0.0f, 0.0f, 0.0f, 0.0f};
    if (aff_a) {
      a4 = *(const f32x4 *)(aff_a + (size_t)b * c + ch4);
      b4 = *(const f32x4 *)(aff_b + (size_t)b * c + ch4);
    }
#pragma unroll 2
    for (int it = 0; it < 4; ++it) {
      const int pl = wave * 16 + it * 4 + ps;
      f32x4 fv[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) fv[q] = *(const f32x4 *)(g + (size_t)sidx[pl][q] * c + ch4);
      if (aff_a) {
#pragma unroll
        for (int q = 0; q < 8; ++q)
#pragma unroll
          for (int i = 0; i < 4; ++i) fv[q][i] = fv[q][i] * a4[i] + b4[i];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float acc = sw[pl][0] * fv[0][i];
#pragma unroll
        for (int q = 1; q < 8; ++q) acc = __fmaf_rn(sw[pl][q], fv[q][i], acc);
        tile[4 * cq + i][pl] = acc;
      }
    }
  }
  devox_write_back<false>(tile, c, n, b, c0, p0, t, add, add_scale, add_shift, outs);
}

extern "C" int p2pb_trilinear_devoxelize_cl_affine(int b, int c, int n, int r, const float *coords, const float *grid,
                                                   const float *aff_a, const float *aff_b, const float *add,
                                                   const float *add_scale, const float *add_shift, float *outs,
                                                   void *stream) {
  if (b <= 0 || c <= 0 || n <= 0 || r <= 0 || ((aff_a == nullptr) != (aff_b == nullptr))) return P2PB_EINVAL;
  if (add && (!add_scale || !add_shift)) return P2PB_EINVAL;
  static const long wide = p2pb_experiment_long("devox_cl4", 1);  // (A/B switch: 0 = the 4-byte gathers everywhere)
  if (wide && c % 64 == 0 && (((size_t)grid | (size_t)aff_a | (size_t)aff_b) & 15) == 0)  // (16-byte loads: rows and tables aligned)
    hipLaunchKernelGGL(devox_cl4_kernel, dim3(cdiv(n, 64), c / 64, b), dim3(256), 0, (hipStream_t)stream, c, n, r, coords, grid,
                       aff_a, aff_b, add, add_scale, add_shift, outs);
  else
    hipLaunchKernelGGL(devox_cl_kernel, dim3(cdiv(n, 64), cdiv(c, 64), b), dim3(256), 0, (hipStream_t)stream, c, n, r, coords, grid,
                       aff_a, aff_b, add, add_scale, add_shift, outs);
  return p2pb_launch_status();
}
