// attention.hip -- the cores of the two attention modules for gfx950, forward and backward: LinearAttention
// (models/modules.py:165-194), below, and the softmax Attention of `attention_type: flash` (:197-264), further down.
//
//   qkv f32[b, 3*heads*32, n]  (the output of to_qkv, channel order (q | k | v) x heads x 32)
//   ks   = softmax over n of every k row
//   ctx  = ks v^T                   [32 x 32] per (sample, head):  ctx[d][e] = sum_n ks[d,n] v[e,n]
//   out  = ctx^T q                  out[e,n] = sum_d ctx[d][e] q[d,n]      -> f32[b, heads*32, n]
//
// The two 1x1 convolutions around it (to_qkv, to_out) are the pointwise GEMM kernels of pointwise.hip; this file
// is what sits between them. Tokens are the last level's centres (8 .. 195 in the BASELINE configs), so the work
// is tiny and latency-bound: ONE workgroup per (sample, head) keeps the whole head in LDS / registers and runs
// the three phases back to back -- the reference spends 2 einsum launches + a softmax + 3 rearranges on it.
// Any n is accepted (the rows are streamed in 64-token tiles), so a PVConv-level attention (cfg attentions[i] = 1
// on a set-abstraction stage) takes the same kernel.
#include "common.h"

#define LA_D 32    // dim_head (models/modules.py:170: dim_head=32 is never overridden)
#define LA_T 256   // threads: 4 waves
#define LA_TILE 64 // tokens per tile

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_maxf(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// row statistics of the k block: rmax[d] = max_n k[d,n], rinv[d] = 1 / sum_n exp(k[d,n] - rmax[d])
__device__ __forceinline__ void la_row_stats(const float *__restrict__ k, int n, float *rmax, float *rinv) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  for (int d = w; d < LA_D; d += LA_T / 64) {
    const float *row = k + (size_t)d * n;
    float m = -INFINITY;
    for (int i = l; i < n; i += 64) m = fmaxf(m, row[i]);
    m = wave_maxf(m);
    float s = 0.0f;
    for (int i = l; i < n; i += 64) s += expf(row[i] - m);
    s = wave_sum(s);
    if (l == 0) {
      rmax[d] = m;
      rinv[d] = 1.0f / s;
    }
  }
}

__global__ __launch_bounds__(LA_T) void linear_attention_fwd_kernel(int heads, int n, const float *__restrict__ qkv,
                                                                    float *__restrict__ out,
                                                                    float *__restrict__ ctx_out) {
  __shared__ float rmax[LA_D], rinv[LA_D];
  __shared__ float ks[LA_D][LA_TILE + 1], vs[LA_D][LA_TILE + 1];
  __shared__ float ctx[LA_D][LA_D + 1];
  const int h = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const size_t hid = (size_t)heads * LA_D;
  const float *q = qkv + ((size_t)b * 3 * hid + (size_t)h * LA_D) * n;
  const float *k = q + hid * n;
  const float *v = k + hid * n;
  la_row_stats(k, n, rmax, rinv);
  __syncthreads();
  // ctx[d][e]: thread owns d = t / 8, e = (t % 8) * 4 .. +3
  const int cd = t >> 3, ce = (t & 7) * 4;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int n0 = 0; n0 < n; n0 += LA_TILE) {
    const int tn = min(LA_TILE, n - n0);
    for (int e = t; e < LA_D * LA_TILE; e += LA_T) {
      const int r = e / LA_TILE, c = e % LA_TILE;
      const bool ok = c < tn;
      ks[r][c] = ok ? expf(k[(size_t)r * n + n0 + c] - rmax[r]) * rinv[r] : 0.0f;
      vs[r][c] = ok ? v[(size_t)r * n + n0 + c] : 0.0f;
    }
    __syncthreads();
    for (int c = 0; c < tn; ++c) {
      const float kk = ks[cd][c];
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = __fmaf_rn(kk, vs[ce + i][c], acc[i]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) ctx[cd][ce + i] = acc[i];
  __syncthreads();
  if (ctx_out) {  // saved for the backward pass
    float *co = ctx_out + ((size_t)b * heads + h) * LA_D * LA_D;
    for (int e = t; e < LA_D * LA_D; e += LA_T) co[e] = ctx[e / LA_D][e % LA_D];
  }
  // out[e][n]: lane = token (coalesced), wave w owns e = w*8 .. w*8+7
  float *o = out + ((size_t)b * hid + (size_t)h * LA_D) * n;
  const int w = t >> 6, l = t & 63;
  for (int n0 = 0; n0 < n; n0 += 64) {
    const int c = n0 + l;
    if (c < n) {
      float r[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int d = 0; d < LA_D; ++d) {
        const float qq = q[(size_t)d * n + c];
#pragma unroll
        for (int i = 0; i < 8; ++i) r[i] = __fmaf_rn(ctx[d][w * 8 + i], qq, r[i]);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) o[(size_t)(w * 8 + i) * n + c] = r[i];
    }
  }
}

// backward: given g = dL/dout f32[b, heads*32, n] (+ qkv and the saved ctx) -> dqkv f32[b, 3*heads*32, n]
//   dq[d,n]  = sum_e ctx[d][e] g[e,n]
//   dctx[d][e] = sum_n q[d,n] g[e,n]
//   dv[e,n]  = sum_d dctx[d][e] ks[d,n]
//   dks[d,n] = sum_e dctx[d][e] v[e,n];   dk[d,n] = ks[d,n] (dks[d,n] - sum_m ks[d,m] dks[d,m])
__global__ __launch_bounds__(LA_T) void linear_attention_bwd_kernel(int heads, int n, const float *__restrict__ qkv,
                                                                    const float *__restrict__ ctx_in,
                                                                    const float *__restrict__ g,
                                                                    float *__restrict__ dqkv) {
  __shared__ float rmax[LA_D], rinv[LA_D], rdot[LA_D];
  __shared__ float as[LA_D][LA_TILE + 1], bs[LA_D][LA_TILE + 1];
  __shared__ float ctx[LA_D][LA_D + 1], dctx[LA_D][LA_D + 1];
  const int h = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const size_t hid = (size_t)heads * LA_D;
  const float *q = qkv + ((size_t)b * 3 * hid + (size_t)h * LA_D) * n;
  const float *k = q + hid * n;
  const float *v = k + hid * n;
  const float *go = g + ((size_t)b * hid + (size_t)h * LA_D) * n;
  float *dq = dqkv + ((size_t)b * 3 * hid + (size_t)h * LA_D) * n;
  float *dk = dq + hid * n;
  float *dv = dk + hid * n;
  la_row_stats(k, n, rmax, rinv);
  {
    const float *ci = ctx_in + ((size_t)b * heads + h) * LA_D * LA_D;
    for (int e = t; e < LA_D * LA_D; e += LA_T) ctx[e / LA_D][e % LA_D] = ci[e];
  }
  __syncthreads();
  const int cd = t >> 3, ce = (t & 7) * 4;
  // dctx[d][e] = sum_n q[d,n] g[e,n]
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int n0 = 0; n0 < n; n0 += LA_TILE) {
    const int tn = min(LA_TILE, n - n0);
    for (int e = t; e < LA_D * LA_TILE; e += LA_T) {
      const int r = e / LA_TILE, c = e % LA_TILE;
      const bool ok = c < tn;
      as[r][c] = ok ? q[(size_t)r * n + n0 + c] : 0.0f;
      bs[r][c] = ok ? go[(size_t)r * n + n0 + c] : 0.0f;
    }
    __syncthreads();
    for (int c = 0; c < tn; ++c) {
      const float qq = as[cd][c];
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = __fmaf_rn(qq, bs[ce + i][c], acc[i]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) dctx[cd][ce + i] = acc[i];
  __syncthreads();
  const int w = t >> 6, l = t & 63;
  // rdot[d] = sum_n ks[d,n] dks[d,n] with dks[d,n] = sum_e dctx[d][e] v[e,n]; wave w owns d = w*8 .. +7
  {
    float part[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int c = l; c < n; c += 64) {
      float dks[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int e = 0; e < LA_D; ++e) {
        const float vv = v[(size_t)e * n + c];
#pragma unroll
        for (int i = 0; i < 8; ++i) dks[i] = __fmaf_rn(dctx[w * 8 + i][e], vv, dks[i]);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int d = w * 8 + i;
        part[i] = __fmaf_rn(expf(k[(size_t)d * n + c] - rmax[d]) * rinv[d], dks[i], part[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float s = wave_sum(part[i]);
      if (l == 0) rdot[w * 8 + i] = s;
    }
  }
  __syncthreads();
  for (int n0 = 0; n0 < n; n0 += 64) {
    const int c = n0 + l;
    if (c >= n) continue;
    float rq[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // dq[d = w*8+i]
    float rk[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // dks[d = w*8+i]
    for (int e = 0; e < LA_D; ++e) {
      const float gg = go[(size_t)e * n + c], vv = v[(size_t)e * n + c];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        rq[i] = __fmaf_rn(ctx[w * 8 + i][e], gg, rq[i]);
        rk[i] = __fmaf_rn(dctx[w * 8 + i][e], vv, rk[i]);
      }
    }
    float rv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // dv[e = w*8+i]
    for (int d = 0; d < LA_D; ++d) {
      const float kk = expf(k[(size_t)d * n + c] - rmax[d]) * rinv[d];
#pragma unroll
      for (int i = 0; i < 8; ++i) rv[i] = __fmaf_rn(dctx[d][w * 8 + i], kk, rv[i]);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int d = w * 8 + i;
      const float kk = expf(k[(size_t)d * n + c] - rmax[d]) * rinv[d];
      dq[(size_t)d * n + c] = rq[i];
      dk[(size_t)d * n + c] = kk * (rk[i] - rdot[d]);
      dv[(size_t)d * n + c] = rv[i];
    }
  }
}

extern "C" int p2pb_linear_attention_forward(int b, int heads, int dim_head, int n, const float *qkv, float *out,
                                             float *ctx, void *stream) {
  if (b <= 0 || heads <= 0 || n <= 0 || dim_head != LA_D || !qkv || !out) return P2PB_EINVAL;
  hipLaunchKernelGGL(linear_attention_fwd_kernel, dim3(heads, b), dim3(LA_T), 0, (hipStream_t)stream, heads, n, qkv,
                     out, ctx);
  return p2pb_launch_status();
}

extern "C" int p2pb_linear_attention_backward(int b, int heads, int dim_head, int n, const float *qkv,
                                              const float *ctx, const float *grad_out, float *grad_qkv,
                                              void *stream) {
  if (b <= 0 || heads <= 0 || n <= 0 || dim_head != LA_D || !qkv || !ctx || !grad_out || !grad_qkv)
    return P2PB_EINVAL;
  hipLaunchKernelGGL(linear_attention_bwd_kernel, dim3(heads, b), dim3(LA_T), 0, (hipStream_t)stream, heads, n, qkv,
                     ctx, grad_out, grad_qkv);
  return p2pb_launch_status();
}

// ---------------------------------------------------------------------------------------------------------------------
// Softmax attention (models/modules.py:197-264 `Attention(norm=False, flash=True)`, the `attention_type: flash` global
// attention of models/unet_pvc.py:98-99,238-240): the core between to_q / to_kv and to_out.
//
//   q  f32[b, heads*32, n]      kv f32[b, 2*heads*32, n]  (channel order (k | v) x heads x 32)
//   out[:, i] = sum_j softmax_j((q_i . k_j) * 32^-0.5) v[:, j]          -> f32[b, heads*32, n]
//   lse[i]    = log sum_j exp((q_i . k_j) * 32^-0.5)                    -> f32[b, heads, n]   (for the backward pass)
//
// Same regime as the linear core: n = 8 .. 195 tokens in the BASELINE configs, < 0.1 GFLOP per evaluation, latency-bound
// -- fp32 FMAs and expf on the vector pipe. One wave per (64-query tile, head, sample); a lane owns one query row (its q,
// its accumulator and its running max / sum live in registers, global accesses are coalesced along the token axis) and the
// keys / values stream through LDS in 32-token tiles that every lane reads at the same address (a broadcast): nothing of
// size n^2 exists and LDS use does not depend on n. No atomics anywhere: every output element has one owner and a fixed
// summation order, so both directions are bit-reproducible.
// Summation: a lane adds its n terms one after the other, and a plain fp32 chain of n additions drifts like sqrt(n) ulps
// (measured against fp64 at n = 4096: 1.2e-5 relative, outside the project's 1e-5 gate). Every sum over tokens is therefore
// two-level: a tile's <= 32 terms into a fresh accumulator, the tile totals into the running sum with a compensated
// (Kahan) addition -- the error stays at a tile's whatever n is, for 4 extra operations per 32 terms.
#define SA_T 64                      // threads: one wave, lane = query (forward, dQ) or key (dK / dV)
#define SA_KT 32                     // tokens of the streamed operand per LDS tile
#define SA_LD (LA_D + 4)             // LDS row pitch: 16-byte aligned rows for float4 reads
#define SA_SCALE 0.17677669529663687f  // 32^-0.5

// sum += x with the rounding error of the addition carried in comp
__device__ __forceinline__ void sa_kahan(float &sum, float &comp, float x) {
  const float y = x - comp;
  const float t = sum + y;
  comp = (t - sum) - y;
  sum = t;
}

// rows [j0, j0 + tn) of a channel-major [32 x n] block -> token-major LDS rows dst[token][channel], zero beyond tn
__device__ __forceinline__ void sa_stage(const float *__restrict__ src, int n, int j0, int tn, float (*dst)[SA_LD]) {
  for (int e = threadIdx.x; e < LA_D * SA_KT; e += SA_T) {
    const int d = e / SA_KT, c = e % SA_KT;
    dst[c][d] = c < tn ? src[(size_t)d * n + j0 + c] : 0.0f;
  }
}

// sum_d r[d] * row[d], d ascending (every kernel below forms its scores with this one order: the backward pass
// recomputes exactly the forward's scores)
__device__ __forceinline__ float sa_dot(const float *r, const float *row) {
  float s = 0.0f;
#pragma unroll
  for (int d = 0; d < LA_D; d += 4) {
    const float4 x = *reinterpret_cast<const float4 *>(row + d);
    s = __fmaf_rn(r[d], x.x, s);
    s = __fmaf_rn(r[d + 1], x.y, s);
    s = __fmaf_rn(r[d + 2], x.z, s);
    s = __fmaf_rn(r[d + 3], x.w, s);
  }
  return s;
}

// acc[d] += a * row[d]
__device__ __forceinline__ void sa_axpy(float a, const float *row, float *acc) {
#pragma unroll
  for (int d = 0; d < LA_D; d += 4) {
    const float4 x = *reinterpret_cast<const float4 *>(row + d);
    acc[d] = __fmaf_rn(a, x.x, acc[d]);
    acc[d + 1] = __fmaf_rn(a, x.y, acc[d + 1]);
    acc[d + 2] = __fmaf_rn(a, x.z, acc[d + 2]);
    acc[d + 3] = __fmaf_rn(a, x.w, acc[d + 3]);
  }
}

__global__ __launch_bounds__(SA_T) void softmax_attention_fwd_kernel(int heads, int n, const float *__restrict__ q,
                                                                     const float *__restrict__ kv,
                                                                     float *__restrict__ out, float *__restrict__ lse) {
  __shared__ __attribute__((aligned(16))) float ks[SA_KT][SA_LD];
  __shared__ __attribute__((aligned(16))) float vs[SA_KT][SA_LD];
  __shared__ float ss[SA_KT][SA_T];  // a tile's scores, one private column per lane
  const int h = blockIdx.y, b = blockIdx.z, t = threadIdx.x, i = blockIdx.x * SA_T + t;
  const size_t hid = (size_t)heads * LA_D;
  const float *qh = q + ((size_t)b * hid + (size_t)h * LA_D) * n;
  const float *kh = kv + ((size_t)b * 2 * hid + (size_t)h * LA_D) * n;
  const float *vh = kh + hid * n;
  const bool live = i < n;  // (lanes past the last query run on q = 0 and store nothing: they take part in the staging)
  float qr[LA_D], o[LA_D], oc[LA_D];
#pragma unroll
  for (int d = 0; d < LA_D; ++d) {
    qr[d] = live ? qh[(size_t)d * n + i] : 0.0f;
    o[d] = oc[d] = 0.0f;
  }
  float m = -INFINITY, l = 0.0f, lc = 0.0f;
  for (int j0 = 0; j0 < n; j0 += SA_KT) {
    const int tn = min(SA_KT, n - j0);
    __syncthreads();
    sa_stage(kh, n, j0, tn, ks);
    sa_stage(vh, n, j0, tn, vs);
    __syncthreads();
    float mt = m;
    for (int c = 0; c < tn; ++c) {
      const float sc = sa_dot(qr, ks[c]) * SA_SCALE;
      ss[c][t] = sc;
      mt = fmaxf(mt, sc);
    }
    float ot[LA_D];
#pragma unroll
    for (int d = 0; d < LA_D; ++d) ot[d] = 0.0f;
    float lt = 0.0f;
    for (int c = 0; c < tn; ++c) {
      const float p = expf(ss[c][t] - mt);
      lt += p;
      sa_axpy(p, vs[c], ot);
    }
    // the running sums move to the new maximum (tn >= 1: mt is finite; m = -inf before the first tile gives alpha = 0, and
    // alpha = 1 exactly once the maximum has settled), then take the tile's totals
    const float alpha = expf(m - mt);
    l *= alpha;
    lc *= alpha;
    sa_kahan(l, lc, lt);
#pragma unroll
    for (int d = 0; d < LA_D; ++d) {
      o[d] *= alpha;
      oc[d] *= alpha;
      sa_kahan(o[d], oc[d], ot[d]);
    }
    m = mt;
  }
  if (live) {
    const float inv = 1.0f / l;  // (n = 1: l = 1, out = v exactly)
    float *oh = out + ((size_t)b * hid + (size_t)h * LA_D) * n;
#pragma unroll
    for (int d = 0; d < LA_D; ++d) oh[(size_t)d * n + i] = o[d] * inv;
    if (lse) lse[((size_t)b * heads + h) * n + i] = m + logf(l);
  }
}

// backward, given g = dL/dout: P_ij = exp(s_ij - lse_i) with s = (q_i . k_j) * scale recomputed, D_i = sum_d g[d,i] out[d,i],
//   dS_ij = P_ij (g_i . v_j - D_i);   dq_i = scale * sum_j dS_ij k_j;   dk_j = scale * sum_i dS_ij q_i;   dv_j = sum_i P_ij g_i
// dQ: the forward's decomposition -- a lane owns a query row and walks the key tiles
__global__ __launch_bounds__(SA_T) void softmax_attention_bwd_dq_kernel(int heads, int n, const float *__restrict__ q,
                                                                        const float *__restrict__ kv,
                                                                        const float *__restrict__ out,
                                                                        const float *__restrict__ lse,
                                                                        const float *__restrict__ g,
                                                                        float *__restrict__ dq) {
  __shared__ __attribute__((aligned(16))) float ks[SA_KT][SA_LD];
  __shared__ __attribute__((aligned(16))) float vs[SA_KT][SA_LD];
  const int h = blockIdx.y, b = blockIdx.z, i = blockIdx.x * SA_T + threadIdx.x;
  const size_t hid = (size_t)heads * LA_D;
  const size_t qoff = ((size_t)b * hid + (size_t)h * LA_D) * n;
  const float *kh = kv + ((size_t)b * 2 * hid + (size_t)h * LA_D) * n;
  const float *vh = kh + hid * n;
  const bool live = i < n;
  float qr[LA_D], gr[LA_D], acc[LA_D], accc[LA_D];
  float dsum = 0.0f;
#pragma unroll
  for (int d = 0; d < LA_D; ++d) {
    qr[d] = live ? q[qoff + (size_t)d * n + i] : 0.0f;
    gr[d] = live ? g[qoff + (size_t)d * n + i] : 0.0f;
    dsum = __fmaf_rn(gr[d], live ? out[qoff + (size_t)d * n + i] : 0.0f, dsum);
    acc[d] = accc[d] = 0.0f;
  }
  const float ls = live ? lse[((size_t)b * heads + h) * n + i] : 0.0f;
  for (int j0 = 0; j0 < n; j0 += SA_KT) {
    const int tn = min(SA_KT, n - j0);
    __syncthreads();
    sa_stage(kh, n, j0, tn, ks);
    sa_stage(vh, n, j0, tn, vs);
    __syncthreads();
    float at[LA_D];
#pragma unroll
    for (int d = 0; d < LA_D; ++d) at[d] = 0.0f;
    for (int c = 0; c < tn; ++c) {
      const float p = expf(sa_dot(qr, ks[c]) * SA_SCALE - ls);
      const float ds = p * (sa_dot(gr, vs[c]) - dsum);
      sa_axpy(ds, ks[c], at);
    }
#pragma unroll
    for (int d = 0; d < LA_D; ++d) sa_kahan(acc[d], accc[d], at[d]);
  }
  if (live) {
#pragma unroll
    for (int d = 0; d < LA_D; ++d) dq[qoff + (size_t)d * n + i] = acc[d] * SA_SCALE;
  }
}

// dK, dV: a lane owns a key (its k, v, dk and dv rows in registers) and walks the query tiles, so neither sum crosses a
// workgroup
__global__ __launch_bounds__(SA_T) void softmax_attention_bwd_dkv_kernel(int heads, int n, const float *__restrict__ q,
                                                                         const float *__restrict__ kv,
                                                                         const float *__restrict__ out,
                                                                         const float *__restrict__ lse,
                                                                         const float *__restrict__ g,
                                                                         float *__restrict__ dkv) {
  __shared__ __attribute__((aligned(16))) float qs[SA_KT][SA_LD];
  __shared__ __attribute__((aligned(16))) float gs[SA_KT][SA_LD];
  __shared__ float lses[SA_KT], dsums[SA_KT];
  const int h = blockIdx.y, b = blockIdx.z, t = threadIdx.x, j = blockIdx.x * SA_T + t;
  const size_t hid = (size_t)heads * LA_D;
  const size_t qoff = ((size_t)b * hid + (size_t)h * LA_D) * n;
  const size_t koff = ((size_t)b * 2 * hid + (size_t)h * LA_D) * n;
  const size_t voff = koff + hid * n;
  const bool live = j < n;
  float kr[LA_D], vr[LA_D], dk[LA_D], dv[LA_D], dkc[LA_D], dvc[LA_D];
#pragma unroll
  for (int d = 0; d < LA_D; ++d) {
    kr[d] = live ? kv[koff + (size_t)d * n + j] : 0.0f;
    vr[d] = live ? kv[voff + (size_t)d * n + j] : 0.0f;
    dk[d] = dv[d] = dkc[d] = dvc[d] = 0.0f;
  }
  for (int i0 = 0; i0 < n; i0 += SA_KT) {
    const int tn = min(SA_KT, n - i0);
    __syncthreads();
    sa_stage(q + qoff, n, i0, tn, qs);
    sa_stage(g + qoff, n, i0, tn, gs);
    if (t < tn) {  // D_i in the dQ kernel's order
      float dsum = 0.0f;
      for (int d = 0; d < LA_D; ++d)
        dsum = __fmaf_rn(g[qoff + (size_t)d * n + i0 + t], out[qoff + (size_t)d * n + i0 + t], dsum);
      dsums[t] = dsum;
      lses[t] = lse[((size_t)b * heads + h) * n + i0 + t];
    }
    __syncthreads();
    float dkt[LA_D], dvt[LA_D];
#pragma unroll
    for (int d = 0; d < LA_D; ++d) dkt[d] = dvt[d] = 0.0f;
    for (int c = 0; c < tn; ++c) {
      const float p = expf(sa_dot(kr, qs[c]) * SA_SCALE - lses[c]);
      sa_axpy(p, gs[c], dvt);
      const float ds = p * (sa_dot(vr, gs[c]) - dsums[c]);
      sa_axpy(ds, qs[c], dkt);
    }
#pragma unroll
    for (int d = 0; d < LA_D; ++d) {
      sa_kahan(dk[d], dkc[d], dkt[d]);
      sa_kahan(dv[d], dvc[d], dvt[d]);
    }
  }
  if (live) {
#pragma unroll
    for (int d = 0; d < LA_D; ++d) {
      dkv[koff + (size_t)d * n + j] = dk[d] * SA_SCALE;
      dkv[voff + (size_t)d * n + j] = dv[d];
    }
  }
}

static bool sa_grid(int b, int heads, int n, dim3 *grid) {
  // (tile, head, sample): the y and z extents of a grid stop at 65535
  if (heads > 65535 || b > 65535) return false;
  *grid = dim3((n + SA_T - 1) / SA_T, heads, b);
  return true;
}

extern "C" int p2pb_softmax_attention_forward(int b, int heads, int dim_head, int n, const float *q, const float *kv,
                                              float *out, float *lse, void *stream) {
  dim3 grid;
  if (b <= 0 || heads <= 0 || n <= 0 || dim_head != LA_D || !q || !kv || !out || !sa_grid(b, heads, n, &grid))
    return P2PB_EINVAL;
  hipLaunchKernelGGL(softmax_attention_fwd_kernel, grid, dim3(SA_T), 0, (hipStream_t)stream, heads, n, q, kv, out, lse);
  return p2pb_launch_status();
}

extern "C" int p2pb_softmax_attention_backward(int b, int heads, int dim_head, int n, const float *q, const float *kv,
                                               const float *out, const float *lse, const float *grad_out, float *grad_q,
                                               float *grad_kv, void *stream) {
  dim3 grid;
  if (b <= 0 || heads <= 0 || n <= 0 || dim_head != LA_D || !q || !kv || !out || !lse || !grad_out || !grad_q || !grad_kv ||
      !sa_grid(b, heads, n, &grid))
    return P2PB_EINVAL;
  hipLaunchKernelGGL(softmax_attention_bwd_dq_kernel, grid, dim3(SA_T), 0, (hipStream_t)stream, heads, n, q, kv, out, lse,
                     grad_out, grad_q);
  int rc = p2pb_launch_status();
  if (rc != 0) return rc;
  hipLaunchKernelGGL(softmax_attention_bwd_dkv_kernel, grid, dim3(SA_T), 0, (hipStream_t)stream, heads, n, q, kv, out, lse,
                     grad_out, grad_kv);
  return p2pb_launch_status();
}
