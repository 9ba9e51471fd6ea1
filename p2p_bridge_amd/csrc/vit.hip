// vit.hip -- the forward of a DINOv2 vision transformer (p2p_bridge_amd/dinov2.py): patch projection, LayerNorm, the linear
// layers with their epilogues, and softmax attention for 64-wide heads. Contract: include/p2pb_hip.h, "vision transformer".
//
// Layout: tokens are ROW-major here, x f32[rows = B*T, C], unlike the channel-major [B,C,N] point tensors of this library.
// Every reduction of a ViT runs over C (LayerNorm, a head's 64 channels, the K axis of all five GEMMs), the weights of the
// checkpoints are [out, in] with `in` contiguous, and the result the callers read is [B, T, C] (patch tokens, then the
// channel-last grid that p2pb_imgfeat_fuse_grid samples). With C contiguous all of these are 16-byte vector accesses at any
// T: T = 1 + h*w is 235 at 192 x 256 frames -- odd -- and a channel-major layout would need it padded to a multiple of 4 in
// every buffer and a transpose at both ends. Rows need no padding at all, so nothing here reads or writes a padded token.
//
// Arithmetic: fp32 operands, fp32 FMAs on the vector pipe, fp32 results: NOT the split-operand matrix arithmetic of
// pointwise*.hip. DINOv2 residual streams carry outlier channels in the thousands and post-GELU activations have no bound; the
// f16x3 split is exact only below 16380 / 4. An fp32 FMA has no range to audit, and gfx950's exact-fp32 MFMA runs at the fp32
// vector rate, so the matrix pipe would only pay in the six-product bf16 form. Sums over K are two-level: a
// 16-term tile into a fresh accumulator, the tile totals into the running sum, so the rounding error grows like
// sqrt(16) + sqrt(K/16) instead of sqrt(K). No atomics: one owner and one fixed summation order per output element, the same
// bits on every run.
//
// Launches of one forward_features call: 2 (im2col + class rows, patch GEMM) + 7 per block (norm1, qkv, attention, proj with
// the LayerScale residual, norm2, fc1 with GELU, fc2 with the LayerScale residual) + 1 (final norm) = 3 + 7 * depth:
// 87 for ViT-S/14 and ViT-B/14 (depth 12), 171 for ViT-L/14 (depth 24).
#include "vit_common.h"

#include <limits.h>

namespace {

// ---- linear layers ----------------------------------------------------------------------------------------------------
// y[m, n] = epilogue(sum_k x[m, k] * w[n, k] + bias[n]). A 64 x 64 output tile per 256-thread workgroup, 4 x 4 per thread, K in
// tiles of 16 through LDS (stored k-major so that a thread reads its four rows / columns as one 16-byte vector); the next
// tile's global loads are in flight while the current one is multiplied.
#define VG_BM 64
#define VG_BN 64
#define VG_BK 16
#define VG_LD (VG_BM + 4)  // LDS row pitch in floats: 16-byte aligned rows

#define VIT_EPI_PATCH 3  // internal: row m = (image, patch) goes to token row image * (P + 1) + 1 + patch, + pos[1 + patch]

__device__ __forceinline__ float4 vg_load(const float *__restrict__ base, int ld, int row, int nrows, int k, int kdim) {
  if (row < nrows && k < kdim) return *reinterpret_cast<const float4 *>(base + (size_t)row * ld + k);  // (kdim % 4 == 0)
  return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

template <int EPI>
__global__ __launch_bounds__(256) void vit_linear_kernel(int m, int n, int kdim, const float *__restrict__ x,
                                                         const float *__restrict__ w, const float *__restrict__ bias,
                                                         const float *__restrict__ aux, int patches, float *__restrict__ y) {
  __shared__ __attribute__((aligned(16))) float as[VG_BK][VG_LD];
  __shared__ __attribute__((aligned(16))) float bs[VG_BK][VG_LD];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int m0 = blockIdx.y * VG_BM, n0 = blockIdx.x * VG_BN;
  const int lr = tid >> 2, lk = (tid & 3) * 4;  // this thread's row of the tile and its four k of the 16
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
  float4 ga = vg_load(x, kdim, m0 + lr, m, lk, kdim);
  float4 gb = vg_load(w, kdim, n0 + lr, n, lk, kdim);
  for (int k0 = 0; k0 < kdim; k0 += VG_BK) {
    __syncthreads();  // the previous tile has been read
    as[lk][lr] = ga.x, as[lk + 1][lr] = ga.y, as[lk + 2][lr] = ga.z, as[lk + 3][lr] = ga.w;
    bs[lk][lr] = gb.x, bs[lk + 1][lr] = gb.y, bs[lk + 2][lr] = gb.z, bs[lk + 3][lr] = gb.w;
    __syncthreads();
    if (k0 + VG_BK < kdim) {
      ga = vg_load(x, kdim, m0 + lr, m, k0 + VG_BK + lk, kdim);
      gb = vg_load(w, kdim, n0 + lr, n, k0 + VG_BK + lk, kdim);
    }
    float part[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) part[i][j] = 0.0f;
#pragma unroll
    for (int kk = 0; kk < VG_BK; ++kk) {
      const float4 a4 = *reinterpret_cast<const float4 *>(&as[kk][ty * 4]);
      const float4 b4 = *reinterpret_cast<const float4 *>(&bs[kk][tx * 4]);
      const float a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) part[i][j] = __fmaf_rn(a[i], b[j], part[i][j]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] += part[i][j];
  }
  const int col = n0 + tx * 4;
  if (col >= n) return;  // (n % 4 == 0: a thread's four columns are inside or outside together)
  const float4 b4 = *reinterpret_cast<const float4 *>(bias + col);
  const float bv[4] = {b4.x, b4.y, b4.z, b4.w};
  float gv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if constexpr (EPI == P2PB_VIT_EPI_RESIDUAL) {
    const float4 g4 = *reinterpret_cast<const float4 *>(aux + col);
    gv[0] = g4.x, gv[1] = g4.y, gv[2] = g4.z, gv[3] = g4.w;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = m0 + ty * 4 + i;
    if (row >= m) continue;
    size_t orow = (size_t)row;
    float r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = acc[i][j] + bv[j];
    if constexpr (EPI == P2PB_VIT_EPI_GELU) {
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = gelu_erf(r[j]);
    }
    if constexpr (EPI == VIT_EPI_PATCH) {
      const int img = row / patches, p = row % patches;
      orow = (size_t)img * (patches + 1) + 1 + p;
      const float4 p4 = *reinterpret_cast<const float4 *>(aux + (size_t)(1 + p) * n + col);
      r[0] += p4.x, r[1] += p4.y, r[2] += p4.z, r[3] += p4.w;
    }
    float4 *dst = reinterpret_cast<float4 *>(y + orow * n + col);
    if constexpr (EPI == P2PB_VIT_EPI_RESIDUAL) {
      const float4 o = *dst;  // this thread is the element's only reader and writer
      r[0] = __fmaf_rn(gv[0], r[0], o.x), r[1] = __fmaf_rn(gv[1], r[1], o.y);
      r[2] = __fmaf_rn(gv[2], r[2], o.z), r[3] = __fmaf_rn(gv[3], r[3], o.w);
    }
    *dst = make_float4(r[0], r[1], r[2], r[3]);
  }
}

template <int EPI>
static int vit_linear_launch(int m, int n, int k, const float *x, const float *w, const float *bias, const float *aux,
                             int patches, float *y, hipStream_t s) {
  hipLaunchKernelGGL(vit_linear_kernel<EPI>, dim3(cdiv(n, VG_BN), cdiv(m, VG_BM)), dim3(256), 0, s, m, n, k, x, w, bias, aux,
                     patches, y);
  return p2pb_launch_status();
}

// ---- patch projection ---------------------------------------------------------------------------------------------------
// cols[(image, patch), ci*ps*ps + ky*ps + kx] = image[ci, py*ps + ky, px*ps + kx] (the order of a Conv2d weight's [C, 3, ps, ps]
// rows), and in the same launch the class rows x[image, 0, :] = cls + pos[0].
__global__ __launch_bounds__(256) void vit_im2col_kernel(int b, int hp, int wp, int ps, int c, long ncol_blocks,
                                                         const float *__restrict__ img, const float *__restrict__ cls,
                                                         const float *__restrict__ pos, float *__restrict__ cols,
                                                         float *__restrict__ x) {
  const int kdim = 3 * ps * ps, patches = hp * wp;
  if ((long)blockIdx.x < ncol_blocks) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)b * patches * kdim) return;
    const int k = (int)(e % kdim);
    const long bp = e / kdim;
    const int p = (int)(bp % patches), im = (int)(bp / patches);
    const int ci = k / (ps * ps), ky = (k / ps) % ps, kx = k % ps;
    const int py = p / wp, px = p % wp;
    const size_t hh = (size_t)hp * ps, ww = (size_t)wp * ps;
    cols[e] = img[(((size_t)im * 3 + ci) * hh + (size_t)py * ps + ky) * ww + (size_t)px * ps + kx];
    return;
  }
  const long e = ((long)blockIdx.x - ncol_blocks) * 256 + threadIdx.x;
  if (e >= (long)b * c) return;
  const int ch = (int)(e % c);
  x[(size_t)(e / c) * (patches + 1) * c + ch] = cls[ch] + pos[ch];
}

// ---- softmax attention, 64-wide heads --------------------------------------------------------------------------------
// qkv f32[b, n, 3*heads*64], channel order (q | k | v) x heads x 64; out f32[b, n, heads*64]. The streamed form of
// csrc/attention.hip (keys and values through LDS in 32-token tiles, running max and sum per query, nothing of size n^2), with
// more parallelism than its one-lane-per-query layout has at 235 tokens: a 256-thread workgroup per (64-query tile, head,
// image) shares the staged tiles; a wave owns 16 queries and FOUR lanes own one query (lane = slice * 16 + query), each lane
// walking every fourth key of a tile with its own running max / sum / accumulator; at the end the four partial softmaxes of
// a query are merged through two lane exchanges (xor 16, xor 32) with a symmetric formula, so all four lanes hold the same
// bits and the order of every sum is fixed: the same bits on every run.
// Padding: only tokens < n_valid exist. Keys >= n_valid are never LOADED (so whatever the padding holds, NaN included, it
// carries exactly zero weight), queries >= n_valid are not loaded either and their output rows are written as zeros.
// Sums over tokens are two-level (a lane's <= 8 terms of a tile into a fresh accumulator, then the tile totals).
#define VA_D 64
#define VA_KT 32
#define VA_LD (VA_D + 4)
#define VA_Q 64     // queries per workgroup
#define VA_SL 4     // lanes (key slices) per query

// (m, l, o) of this lane merged with the lane `mask` away: both partners compute the same bits (max and + commute)
__device__ __forceinline__ void va_merge(float &m, float &l, float *o, int mask) {
  const float m2 = __shfl_xor(m, mask), l2 = __shfl_xor(l, mask);
  const float mn = fmaxf(m, m2);
  // a slice that saw no key has m = -inf, l = 0, o = 0: its factor is 0 (exp(-inf - -inf) would be NaN)
  const float e1 = m == -INFINITY ? 0.0f : expf(m - mn), e2 = m2 == -INFINITY ? 0.0f : expf(m2 - mn);
  l = l * e1 + l2 * e2;
#pragma unroll
  for (int d = 0; d < VA_D; ++d) {
    const float o2 = __shfl_xor(o[d], mask);
    o[d] = o[d] * e1 + o2 * e2;
  }
  m = mn;
}

__global__ __launch_bounds__(256) void vit_attention_kernel(int heads, int n, int n_valid, const float *__restrict__ qkv,
                                                           float *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) float ks[VA_KT][VA_LD];
  __shared__ __attribute__((aligned(16))) float vs[VA_KT][VA_LD];
  __shared__ float ss[VA_KT / VA_SL][256];  // a lane's scores of the tile, one private column per thread
  const int h = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
  const int lane = t & 63, slice = lane >> 4;
  const int i = blockIdx.x * VA_Q + (t >> 6) * 16 + (lane & 15);
  const size_t c = (size_t)heads * VA_D, ld = 3 * c;
  const float *base = qkv + (size_t)b * n * ld + (size_t)h * VA_D;
  const bool live = i < n_valid;
  float q[VA_D], o[VA_D];
#pragma unroll
  for (int d = 0; d < VA_D; d += 4) {
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (live) v = *reinterpret_cast<const float4 *>(base + (size_t)i * ld + d);
    q[d] = v.x * 0.125f, q[d + 1] = v.y * 0.125f, q[d + 2] = v.z * 0.125f, q[d + 3] = v.w * 0.125f;  // 64^-0.5, exact
    o[d] = o[d + 1] = o[d + 2] = o[d + 3] = 0.0f;
  }
  float mx = -INFINITY, l = 0.0f;
  for (int j0 = 0; j0 < n_valid; j0 += VA_KT) {
    const int tn = min(VA_KT, n_valid - j0);
    __syncthreads();
    for (int e = t; e < VA_KT * (VA_D / 4); e += 256) {
      const int r = e / (VA_D / 4), d = (e % (VA_D / 4)) * 4;
      float4 kq = make_float4(0.0f, 0.0f, 0.0f, 0.0f), vq = kq;
      if (r < tn) {
        const float *row = base + (size_t)(j0 + r) * ld + d;
        kq = *reinterpret_cast<const float4 *>(row + c);
        vq = *reinterpret_cast<const float4 *>(row + 2 * c);
      }
      *reinterpret_cast<float4 *>(&ks[r][d]) = kq;
      *reinterpret_cast<float4 *>(&vs[r][d]) = vq;
    }
    __syncthreads();
    if (slice >= tn) continue;  // no key of this tile for this lane (the barriers above are reached by every thread first)
    float mt = mx;
    for (int r = slice, u = 0; r < tn; r += VA_SL, ++u) {
      float sc = 0.0f;
#pragma unroll
      for (int d = 0; d < VA_D; d += 4) {
        const float4 k4 = *reinterpret_cast<const float4 *>(&ks[r][d]);
        sc = __fmaf_rn(q[d], k4.x, sc);
        sc = __fmaf_rn(q[d + 1], k4.y, sc);
        sc = __fmaf_rn(q[d + 2], k4.z, sc);
        sc = __fmaf_rn(q[d + 3], k4.w, sc);
      }
      ss[u][t] = sc;
      mt = fmaxf(mt, sc);
    }
    float ot[VA_D];
#pragma unroll
    for (int d = 0; d < VA_D; ++d) ot[d] = 0.0f;
    float lt = 0.0f;
    for (int r = slice, u = 0; r < tn; r += VA_SL, ++u) {
      const float p = expf(ss[u][t] - mt);
      lt += p;
#pragma unroll
      for (int d = 0; d < VA_D; d += 4) {
        const float4 v4 = *reinterpret_cast<const float4 *>(&vs[r][d]);
        ot[d] = __fmaf_rn(p, v4.x, ot[d]);
        ot[d + 1] = __fmaf_rn(p, v4.y, ot[d + 1]);
        ot[d + 2] = __fmaf_rn(p, v4.z, ot[d + 2]);
        ot[d + 3] = __fmaf_rn(p, v4.w, ot[d + 3]);
      }
    }
    // move the running sums to the new maximum (mx = -inf before the lane's first key: alpha = 0), then add the tile's totals
    const float alpha = expf(mx - mt);
    l = l * alpha + lt;
#pragma unroll
    for (int d = 0; d < VA_D; ++d) o[d] = o[d] * alpha + ot[d];
    mx = mt;
  }
  va_merge(mx, l, o, 16);
  va_merge(mx, l, o, 32);
  if (i < n && slice == 0) {
    const float inv = live ? 1.0f / l : 0.0f;  // (a padded query: o = 0 and inv = 0, zeros are written)
    float *orow = out + ((size_t)b * n + i) * c + (size_t)h * VA_D;
#pragma unroll
    for (int d = 0; d < VA_D; d += 4)
      *reinterpret_cast<float4 *>(orow + d) = make_float4(o[d] * inv, o[d + 1] * inv, o[d + 2] * inv, o[d + 3] * inv);
  }
}

}  // namespace

extern "C" int p2pb_vit_layernorm(int rows, int c, const float *x, const float *gamma, const float *beta, float eps, float *y,
                                  void *stream) {
  if (rows <= 0 || c <= 0 || !(eps >= 0.0f)) return P2PB_EINVAL;
  if (!x || !gamma || !beta || !y) return P2PB_EINVAL;
  hipLaunchKernelGGL(vit_layernorm_kernel<float>, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, rows, c, x, gamma, beta, eps,
                     y);
  return p2pb_launch_status();
}

extern "C" int p2pb_vit_linear(int m, int n, int k, const float *x, const float *w, const float *bias, int epilogue,
                               const float *gamma, float *y, void *stream) {
  if (m <= 0 || n <= 0 || k <= 0 || n % 4 != 0 || k % 4 != 0) return P2PB_EINVAL;
  if (!x || !w || !bias || !y || (epilogue == P2PB_VIT_EPI_RESIDUAL && !gamma)) return P2PB_EINVAL;
  if (!aligned16(x) || !aligned16(w) || !aligned16(bias) || !aligned16(y) || !aligned16(gamma)) return P2PB_EINVAL;
  if (cdiv(m, VG_BM) > 65535u) return P2PB_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  switch (epilogue) {
    case P2PB_VIT_EPI_BIAS: return vit_linear_launch<P2PB_VIT_EPI_BIAS>(m, n, k, x, w, bias, nullptr, 1, y, s);
    case P2PB_VIT_EPI_GELU: return vit_linear_launch<P2PB_VIT_EPI_GELU>(m, n, k, x, w, bias, nullptr, 1, y, s);
    case P2PB_VIT_EPI_RESIDUAL: return vit_linear_launch<P2PB_VIT_EPI_RESIDUAL>(m, n, k, x, w, bias, gamma, 1, y, s);
  }
  return P2PB_EINVAL;
}

extern "C" size_t p2pb_vit_patch_embed_ws_floats(int b, int hp, int wp, int patch) {
  if (b <= 0 || hp <= 0 || wp <= 0 || patch <= 0) return 0;
  return (size_t)b * hp * wp * 3 * patch * patch;
}

extern "C" int p2pb_vit_patch_embed(int b, int hp, int wp, int patch, int c, const float *images, const float *weight,
                                    const float *bias, const float *cls, const float *pos, float *ws, float *x, void *stream) {
  if (b <= 0 || hp <= 0 || wp <= 0 || patch <= 0 || c <= 0 || c % 4 != 0 || patch % 2 != 0) return P2PB_EINVAL;
  if (!images || !weight || !bias || !cls || !pos || !ws || !x) return P2PB_EINVAL;
  if (!aligned16(weight) || !aligned16(bias) || !aligned16(pos) || !aligned16(ws) || !aligned16(x)) return P2PB_EINVAL;
  const size_t patches = (size_t)hp * wp, kdim = (size_t)3 * patch * patch;  // (patch even: kdim % 4 == 0)
  if (patches > 65535 || (size_t)b * patches * kdim > (size_t)INT_MAX || (size_t)b * (patches + 1) * c > (size_t)INT_MAX)
    return P2PB_EINVAL;
  const int m = (int)(b * patches);
  if (cdiv(m, VG_BM) > 65535u) return P2PB_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long ncol_blocks = cdiv((long)m * (long)kdim, 256);
  hipLaunchKernelGGL(vit_im2col_kernel, dim3((unsigned)(ncol_blocks + cdiv((long)b * c, 256))), dim3(256), 0, s, b, hp, wp, patch,
                     c, ncol_blocks, images, cls, pos, ws, x);
  int rc = p2pb_launch_status();
  if (rc) return rc;
  return vit_linear_launch<VIT_EPI_PATCH>(m, c, (int)kdim, ws, weight, bias, pos, (int)patches, x, s);
}

extern "C" int p2pb_vit_attention_forward(int b, int heads, int n, int n_valid, const float *qkv, float *out, void *stream) {
  if (b <= 0 || heads <= 0 || n <= 0 || n_valid <= 0 || n_valid > n || b > 65535 || heads > 65535) return P2PB_EINVAL;
  if (!qkv || !out || !aligned16(qkv) || !aligned16(out)) return P2PB_EINVAL;
  if ((size_t)b * n * 3 * heads * VA_D > (size_t)INT_MAX * 4) return P2PB_EINVAL;
  hipLaunchKernelGGL(vit_attention_kernel, dim3(cdiv(n, VA_Q), heads, b), dim3(256), 0, (hipStream_t)stream, heads, n, n_valid,
                     qkv, out);
  return p2pb_launch_status();
}
