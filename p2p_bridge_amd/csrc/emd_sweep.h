// emd_sweep.h -- the approximate-matching kernels (metrics/PyTorchEMD/cuda/emd_kernel.cu:33-160) for both of their users:
//   emd.hip         a batch of cloud pairs, the match matrix stored            (EmdBatched)
//   setmetrics.hip  every pair (i, j) of two sets, the cost accumulated level by level, no match matrix   (EmdPairwise)
// The reference runs approxmatch with ONE block per cloud (<<<32,512>>>) and walks the three phases of every annealing level
// behind __syncthreads(); here each phase is its own launch spread over all points (phases are separated by the stream
// order), which keeps every per-thread summation in the reference's ascending order while using the whole chip. Every sweep
// is the same walk: a thread owns one point of one cloud, the OTHER cloud passes through a 1024-record LDS tile of
// (x, y, z, weight), and the thread visits the records in ascending order. The two users differ in where a problem's arrays
// lie (an addressing functor fills an EmdProblem) and in what the match sweep keeps.
#pragma once
#include "common.h"

#define EMD_TILE 1024

// Small batches (evaluation runs one 10k..50k-point cloud at a time) leave a (points / 256) x batch grid far below the
// chip's 256 CUs -- B = 4, N = 8192 is 128 workgroups -- so the inner loop over the OTHER cloud is split over
// blockIdx.y into `chunks` ranges: the PART forms write one partial sum per (chunk, point) and emd_finish_kernel adds
// the partials in ascending chunk order (fixed order: deterministic; the sum is chunk-sequential instead of fully
// sequential: a few ulps per sum, but only harmless when BOTH clouds are split alike -- am_chunk_len below).
// chunks == 1 keeps the single-pass kernels.

struct EmdProblem {
  const float *xyz1, *xyz2;                    // [n][3] sources, [m][3] targets
  float *remainL, *ratioL, *remainR, *ratioR;  // [n], [n], [m], [m]
  float *costk;                                // [n] sum over the levels of d_kl w_kl   (pairwise)
  float *match;                                // [m][n]                                 (batched)
  float *part;                                 // partial sum of chunk c for owned point k: part[c * part_stride + k]
  size_t part_stride;
};

// Problem i of a batch in the reference's scratch layout (emd_kernel.cu:34), array-major:
//   temp = remainL[b][n] | remainR[b][m] | ratioL[b][n] | ratioR[b][m] | partials[chunks][b][max(n, m)]
struct EmdBatched {
  static constexpr bool kChunked = true, kStoreMatch = true, kCost = false;
  const float *xyz1, *xyz2;
  float *temp, *match;
  int b;
  __device__ __forceinline__ EmdProblem operator()(int i, int n, int m) const {
    EmdProblem e;
    e.xyz1 = xyz1 + (size_t)i * n * 3;
    e.xyz2 = xyz2 + (size_t)i * m * 3;
    e.remainL = temp + (size_t)i * n;
    e.remainR = temp + (size_t)b * n + (size_t)i * m;
    e.ratioL = temp + (size_t)b * (n + m) + (size_t)i * n;
    e.ratioR = temp + (size_t)b * (2 * (size_t)n + m) + (size_t)i * m;
    e.costk = nullptr;
    e.match = match + (size_t)i * n * m;
    e.part = temp + (size_t)b * (n + m) * 2 + (size_t)i * max(n, m);
    e.part_stride = (size_t)b * max(n, m);
    return e;
  }
};

// Pair p = p0 + i -> clouds (p / r, p % r) of two sets; the work arrays of pair i of the chunk in flight:
//   remainL[n] | ratioL[n] | costk[n] | remainR[m] | ratioR[m]
struct EmdPairwise {
  static constexpr bool kChunked = false, kStoreMatch = false, kCost = true;
  const float *A, *B;
  float *ws;
  int p0, r;
  __device__ __forceinline__ EmdProblem operator()(int i, int n, int m) const {
    const int p = p0 + i;
    EmdProblem e;
    e.xyz1 = A + (size_t)(p / r) * n * 3;
    e.xyz2 = B + (size_t)(p % r) * m * 3;
    e.remainL = ws + (size_t)i * (3 * (size_t)n + 2 * (size_t)m);
    e.ratioL = e.remainL + n, e.costk = e.ratioL + n, e.remainR = e.costk + n, e.ratioR = e.remainR + m;
    e.match = nullptr, e.part = nullptr, e.part_stride = 0;
    return e;
  }
};

// records [lo, hi) of `other` with weights `w` through the LDS tile; step(l, record) per record, ascending. Every thread of the
// workgroup stages and meets the barriers; a thread that is not `active` visits no record. (The sweep that stores into match
// wants its idle threads out of the record loop as a whole: with the test at the store instead, each step's load of match
// issues behind a branch after the step's arithmetic, not ahead of it, and approxmatch ran 17 % longer at 4 x 8192^2.)
template <class Step>
__device__ __forceinline__ void emd_tile_walk(float4 *buf, const float *other, const float *w, int lo, int hi, bool active,
                                              Step step) {
  for (int l0 = lo; l0 < hi; l0 += EMD_TILE) {
    const int ln = min(EMD_TILE, hi - l0);
    __syncthreads();
    for (int l = threadIdx.x; l < ln; l += 256) {
      const float *q = other + (size_t)(l0 + l) * 3;
      buf[l] = make_float4(q[0], q[1], q[2], w[l0 + l]);
    }
    __syncthreads();
    if (active)
      for (int l = 0; l < ln; ++l) step(l0 + l, buf[l]);
  }
}

// What a sum over the other cloud starts from (single pass, and the finisher of the partials: the partials themselves start
// from 0) and where it goes.
// suml_k = 1e-9 + sum_l exp(level*d_kl) * remainR_l ; ratioL_k = remainL_k / suml_k      (:58-88)
struct EmdRatioL {
  static constexpr float kStart = 1e-9f;
  static constexpr bool kOwnsSource = true;
  static __device__ __forceinline__ void finish(const EmdProblem &e, int k, float suml) {
    e.ratioL[k] = __fdiv_rn(e.remainL[k], suml);
  }
};
// sumr_l = remainR_l * sum_k exp(level*d_kl)*ratioL_k ; consumption ; ratioR ; remainR update   (:90-122)
__device__ __forceinline__ void am_ratio_r_finish(float sumr, float *__restrict__ remainR, float *__restrict__ ratioR) {
  const float rr = *remainR;
  sumr *= rr;
  const float consumption = fminf(__fdiv_rn(rr, sumr + 1e-9f), 1.0f);
  *ratioR = consumption * rr;
  *remainR = fmaxf(0.0f, rr - sumr);
}
struct EmdRatioR {
  static constexpr float kStart = 0.0f;
  static constexpr bool kOwnsSource = false;
  static __device__ __forceinline__ void finish(const EmdProblem &e, int l, float sumr) {
    am_ratio_r_finish(sumr, e.remainR + l, e.ratioR + l);
  }
};
// remainL_k -= sum_l w_kl                                                                        (:124-160)
struct EmdMatched {
  static constexpr float kStart = 0.0f;
  static constexpr bool kOwnsSource = true;
  static __device__ __forceinline__ void finish(const EmdProblem &e, int k, float suml) {
    e.remainL[k] = fmaxf(0.0f, e.remainL[k] - suml);
  }
};

template <class Addr>
__global__ __launch_bounds__(256) void emd_init_kernel(Addr addr, int n, int m, float multiL, float multiR) {
  const EmdProblem e = addr(blockIdx.y, n, m);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) e.remainL[i] = multiL;
  if (Addr::kCost && i < n) e.costk[i] = 0.0f;
  if (i < m) e.remainR[i] = multiR;
}

// Both ratio phases: sum_other exp(level * d) * weight for the owned point. R = EmdRatioL: a source point over the targets
// weighted by remainR; R = EmdRatioR: a target point over the sources weighted by ratioL.
template <class Addr, bool PART, class R>
__global__ __launch_bounds__(256) void emd_ratio_kernel(Addr addr, int n, int m, int chunk, float level) {
  __shared__ float4 buf[EMD_TILE];
  const EmdProblem e = addr(PART ? blockIdx.z : blockIdx.y, n, m);
  const int own_n = R::kOwnsSource ? n : m, other_n = R::kOwnsSource ? m : n;
  const int k = blockIdx.x * 256 + threadIdx.x;
  const bool ok = k < own_n;
  const float *p = (R::kOwnsSource ? e.xyz1 : e.xyz2) + (size_t)(ok ? k : 0) * 3;
  const float x = p[0], y = p[1], z = p[2];
  float sum = PART ? 0.0f : R::kStart;
  const int lo = PART ? blockIdx.y * chunk : 0, hi = PART ? min(other_n, lo + chunk) : other_n;
  emd_tile_walk(buf, R::kOwnsSource ? e.xyz2 : e.xyz1, R::kOwnsSource ? e.remainR : e.ratioL, lo, hi, true,
                [&](int, float4 t) { sum += __expf(level * sqdist3(t.x - x, t.y - y, t.z - z)) * t.w; });
  if (!ok) return;
  if (PART) e.part[blockIdx.y * e.part_stride + k] = sum;
  else R::finish(e, k, sum);
}

// w_kl = exp(level*d_kl)*ratioL_k*ratioR_l ; remainL_k -= sum_l w_kl. STORE: match[l,k] += w_kl (:124-160). COST: matchcost
// (:211-262) is linear in match, which approxmatch only ever adds into, so costk_k += sum_l d_kl w_kl level by level gives the
// cost without the n x m matrix (16 MB per pair at 2048 points, read and written at each of the 10 levels).
template <class Addr, bool PART, bool STORE, bool COST>
__global__ __launch_bounds__(256) void emd_match_kernel(Addr addr, int n, int m, int chunk, float level) {
  __shared__ float4 buf[EMD_TILE];
  const EmdProblem e = addr(PART ? blockIdx.z : blockIdx.y, n, m);
  const int k = blockIdx.x * 256 + threadIdx.x;
  const bool ok = k < n;
  const float *p = e.xyz1 + (size_t)(ok ? k : 0) * 3;
  const float x1 = p[0], y1 = p[1], z1 = p[2];
  const float rl = ok ? e.ratioL[k] : 0.0f;
  float suml = 0.0f, cst = 0.0f;
  const int lo = PART ? blockIdx.y * chunk : 0, hi = PART ? min(m, lo + chunk) : m;
  emd_tile_walk(buf, e.xyz2, e.ratioR, lo, hi, STORE ? ok : true, [&](int l, float4 t) {
    const float d = sqdist3(t.x - x1, t.y - y1, t.z - z1);
    const float w = __expf(level * d) * rl * t.w;
    if (STORE) e.match[(size_t)l * n + k] += w;
    suml += w;
    if (COST) cst += d * w;
  });
  if (!ok) return;
  if (PART) e.part[blockIdx.y * e.part_stride + k] = suml;
  else EmdMatched::finish(e, k, suml);
  if (COST) e.costk[k] += cst;
}

// the partials of one owned point, added in ascending chunk order, into the epilogue of the single-pass kernel
template <class Addr, class R>
__global__ __launch_bounds__(256) void emd_finish_kernel(Addr addr, int n, int m, int chunks) {
  const EmdProblem e = addr(blockIdx.y, n, m);
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= (R::kOwnsSource ? n : m)) return;
  float sum = R::kStart;
  for (int c = 0; c < chunks; ++c) sum += e.part[c * e.part_stride + k];
  R::finish(e, k, sum);
}

// Length of one chunk of a cloud of `len` points: whole LDS tiles where a chunk spans at least one, else whole waves, so that the
// SHORTER cloud is split about as often as the longer one. Both reductions must be chunked alike: a sequential fp32 sum of
// positive terms drops the tails below half an ulp of the running sum, a chunked one keeps more of them. With the sums over
// the targets chunked and the sums over the sources not (1024 x 4096: lc = 4, kc = 1 under whole-tile chunks), the sources
// booked more mass as given than the targets booked as received at every level, and 1.7e-4 of the 4096 units stayed unplaced
// on a few targets: per-target sums short by 4.7e-5 and the cost 1.3e-6 off float64, against 1.4e-6 and 1.9e-7 with kc = 4
// (measured on an MI355X, tests/test_emd_exact_gpu.py; the 1.7e-4 from a CPU restatement of these kernels' arithmetic).
static int am_chunk_len(int len, int chunks) {
  const int per = cdiv(len, chunks), unit = per >= EMD_TILE ? EMD_TILE : 64;
  return (per + unit - 1) / unit * unit;
}

// init and the 10 annealing levels for `count` problems of n sources and m targets; chunks > 1 (Addr::kChunked only) splits
// the other cloud of every sweep and needs the partials behind the problem's arrays
template <class Addr>
static void emd_anneal(Addr addr, int count, int n, int m, int chunks, hipStream_t s) {
  constexpr bool ST = Addr::kStoreMatch, CO = Addr::kCost;
  const float multiL = n >= m ? 1.0f : (float)(m / n), multiR = n >= m ? (float)(n / m) : 1.0f;  // emd_kernel.cu:46-52
  const dim3 gl(cdiv(n, 256), count), gr(cdiv(m, 256), count), t(256);
  hipLaunchKernelGGL(emd_init_kernel<Addr>, dim3(cdiv(n > m ? n : m, 256), count), t, 0, s, addr, n, m, multiL, multiR);
  for (int j = 7; j >= -2; --j) {
    float level = -powf(4.0f, (float)j);
    if (j == -2) level = 0;
    if (chunks == 1) {
      hipLaunchKernelGGL((emd_ratio_kernel<Addr, false, EmdRatioL>), gl, t, 0, s, addr, n, m, m, level);
      hipLaunchKernelGGL((emd_ratio_kernel<Addr, false, EmdRatioR>), gr, t, 0, s, addr, n, m, n, level);
      hipLaunchKernelGGL((emd_match_kernel<Addr, false, ST, CO>), gl, t, 0, s, addr, n, m, m, level);
    } else if constexpr (Addr::kChunked) {
      const int lch = am_chunk_len(m, chunks), kch = am_chunk_len(n, chunks);
      const int lc = cdiv(m, lch), kc = cdiv(n, kch);  // (both <= chunks: the partials fit)
      hipLaunchKernelGGL((emd_ratio_kernel<Addr, true, EmdRatioL>), dim3(gl.x, lc, count), t, 0, s, addr, n, m, lch, level);
      hipLaunchKernelGGL((emd_finish_kernel<Addr, EmdRatioL>), gl, t, 0, s, addr, n, m, lc);
      hipLaunchKernelGGL((emd_ratio_kernel<Addr, true, EmdRatioR>), dim3(gr.x, kc, count), t, 0, s, addr, n, m, kch, level);
      hipLaunchKernelGGL((emd_finish_kernel<Addr, EmdRatioR>), gr, t, 0, s, addr, n, m, kc);
      hipLaunchKernelGGL((emd_match_kernel<Addr, true, ST, CO>), dim3(gl.x, lc, count), t, 0, s, addr, n, m, lch, level);
      hipLaunchKernelGGL((emd_finish_kernel<Addr, EmdMatched>), gl, t, 0, s, addr, n, m, lc);
    }
  }
}
