// vit_f16.hip -- the DINOv2 forward in the arithmetic the reference runs it in (fp16 autocast, image_features.py:494): the
// LayerNorm with an fp16 result, the linear layers and softmax attention on v_mfma_f32_32x32x16_f16. Contract:
// include/p2pb_hip.h, "vision transformer" (the *_f16 entry points); the fp32 siblings are in vit.hip and stay as they are.
//
// Arithmetic: ONLY the operands of matrix products are fp16, each rounded once, round-to-nearest-even (the IEEE conversion
// v_cvt_f16_f32, never the packed round-toward-zero one): the norm outputs, the qkv rows, the softmax weights entering P.V,
// the attention output, the post-GELU activations and the four weights of a block. Products of two fp16 numbers are exact
// in fp32 and every accumulator, bias, GELU, LayerScale, residual, softmax and LayerNorm statistic is fp32. A value beyond
// +-65504 becomes +-inf, as torch.Tensor.half() makes it: nothing saturates and nothing checks.
// No atomics: one owner and one fixed summation order per output element, the same bits on every run.
//
// Fragment maps of v_mfma_f32_32x32x16_f16, D[32 x 32] += A[32 x 16] B[16 x 32], lane l, r = l & 31, h = l >> 5:
//   A element j (0..7) = A[r][8h + j]     B element j = B[8h + j][r]     D register t (0..15) = D[(t & 3) + 8 (t >> 2) + 4h][r]
// Both operands want 8 consecutive k per lane: one 16-byte load from a K-contiguous row (tokens [rows, C] and weights
// [out, in] both are). tests/test_dinov2_half_gpu.py pins these maps with exact integer data.
#include "vit_common.h"

#include <limits.h>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x16 mfma_f16(const u32x4 &a, const u32x4 &b, const f32x16 &c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
// row of D that register t of a lane in half h holds
__device__ __forceinline__ int d_row(int t, int h) { return (t & 3) + 8 * (t >> 2) + 4 * h; }

// ---- linear layers ----------------------------------------------------------------------------------------------------
// y[m, n] = epilogue(sum_k x[m, k] * w[n, k] + bias[n]), x and w fp16. A BM x 64 output tile per workgroup of BM / 16 waves,
// one 32 x 32 tile of it per wave; K in tiles of 64 (BM = 64) or 128 (BM = 32) through LDS (rows padded by 8 halves: the
// 16-byte fragment reads of 16 consecutive rows fall into 16 different bank groups); the next tile's global loads are in
// flight while the current one is multiplied. BM = 32 where 64 x 64 tiles would leave compute units idle (n = 384 at 1880
// rows: 180 tiles on 256 units); there a unit holds one or two workgroups, nothing but the tile's own products hides the
// latency of the next tile's loads, and the time is the number of K tiles times that latency: hence the deeper tile. The
// 64-row form runs where workgroups are many and measured faster with 64.
// A tile's fragments are all read from LDS before its first product and the products alternate between two accumulators
// (even and odd k-steps, added once at the end: a fixed order), so neither an LDS round trip nor the accumulator's latency
// sits between two MFMAs.
// Rows >= m and k >= kdim of a tile are zeros in LDS: their loads go to the last valid row / chunk instead (no branch per
// load) and the value is dropped at the LDS store, so nothing outside x[m, k] and w[n, k] is read; n % 64 == 0, so every
// weight row exists.
#define HG_BN 64
#define HG_BK_FOR(BM) ((BM) == 32 ? 128 : 64)  // the 32-row form runs where workgroups are few: fewer, deeper K tiles

template <int BM, int EPI>
__global__ __launch_bounds__(BM * 4) void vit_linear_f16_kernel(int m, int n, int kdim, const _Float16 *__restrict__ x,
                                                                const _Float16 *__restrict__ w, const float *__restrict__ bias,
                                                                const float *__restrict__ gamma, void *__restrict__ yv) {
  constexpr int NT = BM * 4;  // threads: one wave per 32 x 32 of the tile
  constexpr int HG_BK = HG_BK_FOR(BM), HG_CPR = HG_BK / 8, HG_LD = HG_BK + 8;  // HG_CPR: 16-byte chunks per tile row
  constexpr int ACH = BM * HG_CPR / NT;     // 16-byte chunks of the x tile per thread
  constexpr int BCH = HG_BN * HG_CPR / NT;  // and of the w tile
  __shared__ __attribute__((aligned(16))) _Float16 as[BM][HG_LD];
  __shared__ __attribute__((aligned(16))) _Float16 bs[HG_BN][HG_LD];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * HG_BN;
  u32x4 ga[ACH], gb[BCH];
  const u32x4 zero = {0u, 0u, 0u, 0u};

  auto load = [&](int k0) {
#pragma unroll
    for (int u = 0; u < ACH; ++u) {
      const int c = tid + NT * u, row = m0 + c / HG_CPR, k = k0 + (c % HG_CPR) * 8;
      ga[u] = *reinterpret_cast<const u32x4 *>(x + (size_t)min(row, m - 1) * kdim + min(k, kdim - 8));
    }
#pragma unroll
    for (int u = 0; u < BCH; ++u) {
      const int c = tid + NT * u, row = n0 + c / HG_CPR, k = k0 + (c % HG_CPR) * 8;
      gb[u] = *reinterpret_cast<const u32x4 *>(w + (size_t)row * kdim + min(k, kdim - 8));
    }
  };

  f32x16 acc, acc1;
#pragma unroll
  for (int t = 0; t < 16; ++t) acc[t] = 0.0f, acc1[t] = 0.0f;
  load(0);
  for (int k0 = 0; k0 < kdim; k0 += HG_BK) {
    __syncthreads();  // the previous tile has been read
#pragma unroll
    for (int u = 0; u < ACH; ++u) {
      const int c = tid + NT * u;  // (the value is dropped HERE, not at the load: a select there would wait for it)
      const bool in = m0 + c / HG_CPR < m && k0 + (c % HG_CPR) * 8 < kdim;
      *reinterpret_cast<u32x4 *>(&as[c / HG_CPR][(c % HG_CPR) * 8]) = in ? ga[u] : zero;
    }
#pragma unroll
    for (int u = 0; u < BCH; ++u) {
      const int c = tid + NT * u;
      *reinterpret_cast<u32x4 *>(&bs[c / HG_CPR][(c % HG_CPR) * 8]) = k0 + (c % HG_CPR) * 8 < kdim ? gb[u] : zero;
    }
    __syncthreads();
    if (k0 + HG_BK < kdim) load(k0 + HG_BK);
    u32x4 af[HG_BK / 16], bf[HG_BK / 16];
#pragma unroll
    for (int kk = 0; kk < HG_BK / 16; ++kk) {
      af[kk] = *reinterpret_cast<const u32x4 *>(&as[wm * 32 + r][kk * 16 + 8 * h]);
      bf[kk] = *reinterpret_cast<const u32x4 *>(&bs[wn * 32 + r][kk * 16 + 8 * h]);
    }
#pragma unroll
    for (int kk = 0; kk < HG_BK / 16; kk += 2) {  // (a K tail multiplies zeros)
      acc = mfma_f16(af[kk], bf[kk], acc);
      acc1 = mfma_f16(af[kk + 1], bf[kk + 1], acc1);
    }
  }
#pragma unroll
  for (int t = 0; t < 16; ++t) acc[t] += acc1[t];
  // D[row of x][row of w]: the lane holds one output column, its registers 16 rows
  const int col = n0 + wn * 32 + r;
  const float bv = bias[col];
  float gv = 0.0f;
  float old[16];
  if constexpr (EPI == P2PB_VIT_EPI_RESIDUAL) {
    gv = gamma[col];
    // all 16 stream values are requested before the first is used (one round trip, not 16); a row >= m reads row m - 1
#pragma unroll
    for (int t = 0; t < 16; ++t)
      old[t] = reinterpret_cast<const float *>(yv)[(size_t)min(m0 + wm * 32 + d_row(t, h), m - 1) * n + col];
  }
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const int row = m0 + wm * 32 + d_row(t, h);
    if (row >= m) continue;
    float v = acc[t] + bv;
    if constexpr (EPI == P2PB_VIT_EPI_RESIDUAL) {
      // this lane is the element's only reader and writer
      reinterpret_cast<float *>(yv)[(size_t)row * n + col] = __fmaf_rn(gv, v, old[t]);
    } else {
      if constexpr (EPI == P2PB_VIT_EPI_GELU) v = gelu_erf(v);
      reinterpret_cast<_Float16 *>(yv)[(size_t)row * n + col] = (_Float16)v;  // IEEE: nearest-even, +-inf beyond 65504
    }
  }
}

template <int BM>
static int vit_linear_f16_launch(int m, int n, int k, const _Float16 *x, const _Float16 *w, const float *bias, int epilogue,
                                 const float *gamma, void *y, hipStream_t s) {
  const dim3 grid(n / HG_BN, cdiv(m, BM)), block(BM * 4);
  switch (epilogue) {
    case P2PB_VIT_EPI_BIAS:
      hipLaunchKernelGGL((vit_linear_f16_kernel<BM, P2PB_VIT_EPI_BIAS>), grid, block, 0, s, m, n, k, x, w, bias, gamma, y);
      break;
    case P2PB_VIT_EPI_GELU:
      hipLaunchKernelGGL((vit_linear_f16_kernel<BM, P2PB_VIT_EPI_GELU>), grid, block, 0, s, m, n, k, x, w, bias, gamma, y);
      break;
    case P2PB_VIT_EPI_RESIDUAL:
      hipLaunchKernelGGL((vit_linear_f16_kernel<BM, P2PB_VIT_EPI_RESIDUAL>), grid, block, 0, s, m, n, k, x, w, bias, gamma, y);
      break;
    default: return P2PB_EINVAL;
  }
  return p2pb_launch_status();
}

// ---- softmax attention, 64-wide heads ---------------------------------------------------------------------------------
// qkv f16[b, n, 3*heads*64], channel order (q | k | v) x heads x 64; out f16[b, n, heads*64]. One wave per (32-query tile,
// head, image) streams the keys in tiles of 32 with a running max and sum per query; nothing of size n^2 exists.
// Orientation (so that the weights feed the second product from the registers the first one left them in):
//   X[key][query] = K Q^T    A = K rows (keys), B = Q rows (queries), k = the 64 channels in 4 steps of 16. A lane then holds
//                            ONE query (its column r) and 16 of the tile's 32 keys; the lane 32 away holds the other 16. The
//                            whole softmax state (max, sum, the factor that moves the sums to a new max) is per lane.
//   O^T[d][query] = V^T P    B = the lane's weights, registers 8s .. 8s+7 rounded to fp16 as the fragment of k-step s (0, 1):
//                            element j is key 16s + 8 (j >> 2) + 4h + (j & 3) of the tile. A = V^T in that same key order: the
//                            values are staged TRANSPOSED in LDS ([channel][key], key pairs packed), so a lane reads its
//                            channel's keys 16s + 4h .. + 3 and 16s + 8 + 4h .. + 3 as two 8-byte words. Two 32-channel
//                            accumulators; the lane holds 32 of its query's 64 output channels, the partner lane the others.
// The next tile's keys and values are requested before the current tile is multiplied.
// Padding: only tokens < n_valid exist. Keys >= n_valid are never LOADED; their scores are -inf, their weights exactly 0 and
// their values zeros. Queries >= n_valid are not loaded either and their output rows are written as zeros.
#define HA_D 64
#define HA_KT 32
#define HA_VLD (HA_KT / 2 + 2)  // LDS pitch of a channel's row in key PAIRS (dwords): 8-byte aligned, conflict-free over 32 rows

__device__ __forceinline__ u32x4 ha_load(const _Float16 *__restrict__ p, bool live) {
  const u32x4 zero = {0u, 0u, 0u, 0u};
  return live ? *reinterpret_cast<const u32x4 *>(p) : zero;
}

__global__ __launch_bounds__(64) void vit_attention_f16_kernel(int heads, int n, int n_valid, const _Float16 *__restrict__ qkv,
                                                              _Float16 *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) unsigned vt[HA_D][HA_VLD];  // vt[d][p] = V[2p][d] | V[2p + 1][d] << 16
  const int hd = blockIdx.y, b = blockIdx.z, lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int i = blockIdx.x * 32 + r;  // this lane's query
  const size_t c = (size_t)heads * HA_D, ld = 3 * c;
  const _Float16 *base = qkv + (size_t)b * n * ld + (size_t)hd * HA_D;
  const bool live = i < n_valid;
  u32x4 qf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) qf[s] = ha_load(base + (size_t)i * ld + 16 * s + 8 * h, live);
  // staging of the values: this lane moves the 8 channels vd .. vd + 7 of the key pairs vp and vp + 8
  const int vp = lane >> 3, vd = (lane & 7) * 8;
  u32x4 kf[4], vf[2][2];

  auto load = [&](int j0) {
    const int key = j0 + r;
#pragma unroll
    for (int s = 0; s < 4; ++s) kf[s] = ha_load(base + (size_t)key * ld + c + 16 * s + 8 * h, key < n_valid);
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int kv = j0 + 2 * (vp + 8 * u) + e;
        vf[u][e] = ha_load(base + (size_t)kv * ld + 2 * c + vd, kv < n_valid);
      }
  };

  f32x16 o0, o1;
#pragma unroll
  for (int t = 0; t < 16; ++t) o0[t] = 0.0f, o1[t] = 0.0f;
  float mx = -INFINITY, l = 0.0f;
  load(0);
  for (int j0 = 0; j0 < n_valid; j0 += HA_KT) {
    __syncthreads();  // the previous tile's values have been read
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned lo = vf[u][0][e], hi = vf[u][1][e];  // channels vd + 2e, vd + 2e + 1 of the pair's two keys
        vt[vd + 2 * e][vp + 8 * u] = (lo & 0xffffu) | (hi << 16);
        vt[vd + 2 * e + 1][vp + 8 * u] = (lo >> 16) | (hi & 0xffff0000u);
      }
    f32x16 sc;
#pragma unroll
    for (int t = 0; t < 16; ++t) sc[t] = 0.0f;
#pragma unroll
    for (int s = 0; s < 4; ++s) sc = mfma_f16(kf[s], qf[s], sc);
    __syncthreads();
    if (j0 + HA_KT < n_valid) load(j0 + HA_KT);
    // the lane's 16 scores of its query: logits scaled by 64^-0.5 (exact), keys >= n_valid at -inf
    float mt = -INFINITY;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      sc[t] = (j0 + d_row(t, h) < n_valid) ? sc[t] * 0.125f : -INFINITY;
      mt = fmaxf(mt, sc[t]);
    }
    mt = fmaxf(mt, __shfl_xor(mt, 32));  // (key j0 of the tile exists, so one of the two halves saw a finite score)
    const float mn = fmaxf(mx, mt);
    float lt = 0.0f;
    u32x4 pf[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      f16x8 ph;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float p = expf(sc[8 * s + j] - mn);
        lt += p;
        ph[j] = (_Float16)p;
      }
      pf[s] = __builtin_bit_cast(u32x4, ph);
    }
    lt += __shfl_xor(lt, 32);  // (a + b in both halves: the same bits)
    // move the running sums to the new maximum (mx = -inf before the first tile: alpha = 0), then add the tile
    const float alpha = expf(mx - mn);
    l = l * alpha + lt;
#pragma unroll
    for (int t = 0; t < 16; ++t) o0[t] *= alpha, o1[t] *= alpha;
    mx = mn;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      // keys 16s + 4h .. + 3 and 16s + 8 + 4h .. + 3 = the pairs 8s + 2h, + 1 and 8s + 4 + 2h, + 1 of channel r (and 32 + r)
      const uint2 a0 = *reinterpret_cast<const uint2 *>(&vt[r][8 * s + 2 * h]);
      const uint2 a1 = *reinterpret_cast<const uint2 *>(&vt[r][8 * s + 4 + 2 * h]);
      const uint2 b0 = *reinterpret_cast<const uint2 *>(&vt[32 + r][8 * s + 2 * h]);
      const uint2 b1 = *reinterpret_cast<const uint2 *>(&vt[32 + r][8 * s + 4 + 2 * h]);
      const u32x4 va = {a0.x, a0.y, a1.x, a1.y}, vb = {b0.x, b0.y, b1.x, b1.y};
      o0 = mfma_f16(va, pf[s], o0);
      o1 = mfma_f16(vb, pf[s], o1);
    }
  }
  if (i >= n) return;
  const float inv = live ? 1.0f / l : 0.0f;  // (a padded query: zeros are written)
  _Float16 *orow = out + ((size_t)b * n + i) * c + (size_t)hd * HA_D;
#pragma unroll
  for (int g = 0; g < 4; ++g) {  // registers 4g .. 4g + 3 are the channels 8g + 4h .. + 3 (and 32 more for the second block)
    f16x4 w0, w1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      w0[e] = (_Float16)(live ? o0[4 * g + e] * inv : 0.0f);
      w1[e] = (_Float16)(live ? o1[4 * g + e] * inv : 0.0f);
    }
    *reinterpret_cast<f16x4 *>(orow + 8 * g + 4 * h) = w0;
    *reinterpret_cast<f16x4 *>(orow + 32 + 8 * g + 4 * h) = w1;
  }
}

}  // namespace

extern "C" int p2pb_vit_layernorm_f16(int rows, int c, const float *x, const float *gamma, const float *beta, float eps, void *y,
                                      void *stream) {
  if (rows <= 0 || c <= 0 || !(eps >= 0.0f)) return P2PB_EINVAL;
  if (!x || !gamma || !beta || !y) return P2PB_EINVAL;
  hipLaunchKernelGGL(vit_layernorm_kernel<_Float16>, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, rows, c, x, gamma,
                     beta, eps, (_Float16 *)y);
  return p2pb_launch_status();
}

extern "C" int p2pb_vit_linear_f16(int m, int n, int k, const void *x, const void *w, const float *bias, int epilogue,
                                   const float *gamma, void *y, void *stream) {
  if (m <= 0 || n <= 0 || k <= 0 || n % HG_BN != 0 || k % 32 != 0) return P2PB_EINVAL;
  if (!x || !w || !bias || !y || (epilogue == P2PB_VIT_EPI_RESIDUAL && !gamma)) return P2PB_EINVAL;
  if (!aligned16(x) || !aligned16(w) || !aligned16(bias) || !aligned16(y) || !aligned16(gamma)) return P2PB_EINVAL;
  if (cdiv(m, 32) > 65535u || (size_t)m * n > (size_t)INT_MAX) return P2PB_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const _Float16 *xh = (const _Float16 *)x, *wh = (const _Float16 *)w;
  // 64-row tiles only where they still give every compute unit two workgroups
  if ((long)cdiv(m, 64) * (n / HG_BN) >= 512) return vit_linear_f16_launch<64>(m, n, k, xh, wh, bias, epilogue, gamma, y, s);
  return vit_linear_f16_launch<32>(m, n, k, xh, wh, bias, epilogue, gamma, y, s);
}

extern "C" int p2pb_vit_attention_forward_f16(int b, int heads, int n, int n_valid, const void *qkv, void *out, void *stream) {
  if (b <= 0 || heads <= 0 || n <= 0 || n_valid <= 0 || n_valid > n || b > 65535 || heads > 65535) return P2PB_EINVAL;
  if (!qkv || !out || !aligned16(qkv) || !aligned16(out)) return P2PB_EINVAL;
  if ((size_t)b * n * 3 * heads * HA_D > (size_t)INT_MAX * 4) return P2PB_EINVAL;
  hipLaunchKernelGGL(vit_attention_f16_kernel, dim3(cdiv(n, 32), heads, b), dim3(64), 0, (hipStream_t)stream, heads, n, n_valid,
                     (const _Float16 *)qkv, (_Float16 *)out);
  return p2pb_launch_status();
}
