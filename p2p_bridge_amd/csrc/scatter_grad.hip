// scatter_grad.hip -- the scatter-add backward passes: devoxelise, three-NN interpolation, grouping, gather.
//
//   gx[b, ch, idx[b, k, p]] += w[b, k, p] * gy[b * pitch + ch * P + p]      k < K, p < P
//
// with idx / w laid out [b][K][P] and rows gx[b][ch][0..L), L a grid (r^3) or a point count. With global fp32 atomics the
// chip retires ~14 G adds/s (profiles/r02_atomic_contention.txt), 0.55 ms for the 8.4 M adds of the r = 32 devoxelisation.
// A workgroup instead owns CH rows of one sample in LDS (CH * L floats <= 128 KB): it zeroes them, adds every contribution
// with ds_add_f32, and writes the rows out once, coalesced -- no zero-fill launch, no HBM atomics, and the output is written
// exactly once. Rows longer than the LDS take the global-atomic kernel. Deterministic mode (abi.hip) runs the LDS rows with
// one wave per workgroup and refuses the rows that do not fit.
#include "common.h"

#define SCAT_THREADS 512
#define SCAT_LDS_MAX (128 * 1024)

// one scatter: contributions per point, whether they carry weights, the most rows a workgroup holds in LDS (0: the
// global-atomic kernel only, in either mode) and the channels a workgroup of the global-atomic kernel walks
template <int K_, bool W_, int CAP_, int CC_>
struct Scatter {
  static constexpr int K = K_, CAP = CAP_, CC = CC_;
  static constexpr bool W = W_;
};
using DevoxGrad = Scatter<8, true, 16, 16>;   // L = r^3, P = n
using InterpGrad = Scatter<3, true, 8, 16>;   // L = m,   P = n
using GroupGrad = Scatter<1, false, 8, 8>;    // L = n,   P = m * u
using GatherGrad = Scatter<1, false, 0, 1>;   // L = n,   P = m

// threads per workgroup of the LDS-row kernels: one wave in deterministic mode (adds in program order), 8 waves otherwise
static inline int scat_threads() { return p2pb_deterministic() ? 64 : SCAT_THREADS; }
// channels per workgroup: as many rows as fit 64 KB (two workgroups per CU), at most `cap`; one row up to 128 KB; 0 = no fit
static inline int scat_rows(long L, int c, int cap) {
  if (L * 4 > SCAT_LDS_MAX) return 0;
  int ch = (int)((64 * 1024) / (L * 4));
  if (ch < 1) ch = 1;
  if (ch > cap) ch = cap;
  if (ch > c) ch = c;
  return ch;
}
__device__ __forceinline__ void scat_zero(float *rows, int count) {
  for (int i = threadIdx.x * 4; i < count; i += blockDim.x * 4) *(float4 *)(rows + i) = make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();
}
// rows[j][0..L) -> gx[(b * c + c0 + j)][0..L) for the nch rows of this workgroup; L * 4 bytes need not be 16-aligned
__device__ __forceinline__ void scat_store(const float *rows, int L, int Lp, int nch, float *gx_rows) {
  __syncthreads();
  for (int j = 0; j < nch; ++j)
    for (int i = threadIdx.x; i < L; i += blockDim.x) gx_rows[(size_t)j * L + i] = rows[j * Lp + i];
}

// global atomics: a thread owns one point and walks the CC channels of its workgroup; gx is zero on entry
template <int K, bool W, int CC>
__global__ __launch_bounds__(256) void scat_grad_kernel(int c, int L, int P, const float *__restrict__ gy, size_t pitch,
                                                        const int *__restrict__ inds, const float *__restrict__ wgts,
                                                        float *__restrict__ gx) {
  const int b = blockIdx.z;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  int idx[K];
  float w[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    idx[k] = inds[(size_t)b * K * P + (size_t)k * P + p];
    if constexpr (W) w[k] = wgts[(size_t)b * K * P + (size_t)k * P + p];
  }
  const int c0 = blockIdx.y * CC, c1 = min(c0 + CC, c);
  for (int j = c0; j < c1; ++j) {
    const float g = gy[(size_t)b * pitch + (size_t)j * P + p];
    float *o = gx + ((size_t)b * c + j) * L;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if constexpr (W)
        atomicAdd(o + idx[k], w[k] * g);
      else
        atomicAdd(o + idx[k], g);
    }
  }
}

// the CH rows of a workgroup in LDS; Lp = L rounded up to 4
template <int K, bool W, int CH>
__global__ __launch_bounds__(SCAT_THREADS) void scat_grad_lds_kernel(int c, int L, int Lp, int P, const float *__restrict__ gy,
                                                                    size_t pitch, const int *__restrict__ inds,
                                                                    const float *__restrict__ wgts, float *__restrict__ gx) {
  extern __shared__ float rows[];
  const int b = blockIdx.y, c0 = blockIdx.x * CH, nch = min(CH, c - c0);
  scat_zero(rows, CH * Lp);
  const int *ib = inds + (size_t)b * K * P;
  const float *wb = W ? wgts + (size_t)b * K * P : nullptr;
  const float *g0 = gy + (size_t)b * pitch + (size_t)c0 * P;
  for (int p = threadIdx.x; p < P; p += blockDim.x) {
    int idx[K];
    float w[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      idx[k] = ib[(size_t)k * P + p];
      if constexpr (W) w[k] = wb[(size_t)k * P + p];
    }
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      if (j < nch) {
        const float g = g0[(size_t)j * P + p];
#pragma unroll
        for (int k = 0; k < K; ++k) {
          if constexpr (W)
            atomicAdd(rows + j * Lp + idx[k], w[k] * g);
          else
            atomicAdd(rows + j * Lp + idx[k], g);
        }
      }
    }
  }
  scat_store(rows, L, Lp, nch, gx + ((size_t)b * c + c0) * L);
}

// pitch: floats between two samples of gy (>= c * P; a channel slice of a wider tensor is read in place); w: NULL unless S::W
template <class S>
static int scat_grad(int b, int c, int L, int P, const float *gy, size_t pitch, const int *idx, const float *w, float *gx,
                     hipStream_t s) {
  int ch = scat_rows(L, c, S::CAP);
  while (ch & (ch - 1)) ch &= ch - 1;  // down to a power of two
  if (ch > 0)
    return for_value<1, 2, 4, 8, 16>(ch, [&](auto CH) {
      if constexpr (CH() <= S::CAP) {
        const int Lp = (L + 3) & ~3;
        static bool once = false;
        if (!once) {
          (void)hipFuncSetAttribute((const void *)scat_grad_lds_kernel<S::K, S::W, CH()>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    SCAT_LDS_MAX);
          once = true;
        }
        hipLaunchKernelGGL((scat_grad_lds_kernel<S::K, S::W, CH()>), dim3(cdiv(c, CH()), b), dim3(scat_threads()),
                           sizeof(float) * (size_t)CH() * Lp, s, c, L, Lp, P, gy, pitch, idx, w, gx);
        return p2pb_launch_status();
      } else {
        return P2PB_EINVAL;  // (not reached: scat_rows stays at or below the cap)
      }
    });
  // rows beyond the LDS: only the global-atomic kernel is left, which deterministic mode refuses (a scatter without an LDS form,
  // gather, has never been refused)
  if (S::CAP > 0 && p2pb_deterministic()) return P2PB_EINVAL;
  int e = p2pb_zero_async(gx, sizeof(float) * (size_t)b * c * L, s);
  if (e != 0) return e;
  hipLaunchKernelGGL((scat_grad_kernel<S::K, S::W, S::CC>), dim3(cdiv(P, 256), cdiv(c, S::CC), b), dim3(256), 0, s, c, L, P, gy,
                     pitch, idx, w, gx);
  return p2pb_launch_status();
}

extern "C" int p2pb_trilinear_devoxelize_backward(int b, int c, int n, int r3, const int *inds, const float *wgts,
                                                  const float *grad_y, float *grad_x, void *stream) {
  if (b <= 0 || c <= 0 || n <= 0 || r3 <= 0) return P2PB_EINVAL;
  return scat_grad<DevoxGrad>(b, c, r3, n, grad_y, (size_t)c * n, inds, wgts, grad_x, (hipStream_t)stream);
}

// (gy_pitch >= c*n)
extern "C" int p2pb_three_nn_interpolate_backward_pitched(int b, int c, int n, int m, const float *grad_y, long gy_pitch,
                                                          const int *idx, const float *w, float *grad_x, void *stream) {
  if (b <= 0 || c <= 0 || n <= 0 || m <= 0 || gy_pitch < (long)c * n) return P2PB_EINVAL;
  return scat_grad<InterpGrad>(b, c, m, n, grad_y, (size_t)gy_pitch, idx, w, grad_x, (hipStream_t)stream);
}
extern "C" int p2pb_three_nn_interpolate_backward(int b, int c, int n, int m, const float *grad_y, const int *idx,
                                                  const float *w, float *grad_x, void *stream) {
  return p2pb_three_nn_interpolate_backward_pitched(b, c, n, m, grad_y, (long)c * n, idx, w, grad_x, stream);
}

// (gy_pitch >= c*m*u)
extern "C" int p2pb_grouping_backward_pitched(int b, int c, int n, int m, int u, const float *grad_y, long gy_pitch, const int *idx,
                                              float *grad_x, void *stream) {
  if (b <= 0 || c <= 0 || n <= 0 || m <= 0 || u <= 0 || gy_pitch < (long)c * m * u) return P2PB_EINVAL;
  return scat_grad<GroupGrad>(b, c, n, m * u, grad_y, (size_t)gy_pitch, idx, nullptr, grad_x, (hipStream_t)stream);
}
extern "C" int p2pb_grouping_backward(int b, int c, int n, int m, int u, const float *grad_y, const int *idx,
                                      float *grad_x, void *stream) {
  return p2pb_grouping_backward_pitched(b, c, n, m, u, grad_y, (long)c * m * u, idx, grad_x, stream);
}

extern "C" int p2pb_gather_features_backward(int b, int c, int n, int m, const float *grad_y, const int *idx,
                                             float *grad_x, void *stream) {
  if (b <= 0 || c <= 0 || n <= 0 || m <= 0) return P2PB_EINVAL;
  return scat_grad<GatherGrad>(b, c, n, m, grad_y, (size_t)c * m, idx, nullptr, grad_x, (hipStream_t)stream);
}
