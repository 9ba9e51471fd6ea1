// pairs.hip -- the device pieces of room training pairs (room_pairs.py): a laser mesh and an iPhone scan -> the
// (noisy patch, aligned clean patch) files the room training reads. Replaces what the reference runs through Open3D's mesh
// sampler, cuML's NearestNeighbors and a Python double loop (data/preprocess_batches.py, data/processing/utils.py):
//   * triangle areas and uniform mesh samples (fp64, one rounding);
//   * K <= 128 nearest clean points of every noisy point, for a ragged batch of patches in one launch;
//   * the greedy unique assignment, computed exactly by deferred acceptance on integer atomicMin;
//   * centre, scale and the assembled output rows.
// No float atomics, no kernel waits on another workgroup: the same inputs give the same bits.
// Contract: include/p2pb_hip.h, "room training pairs".
#include <limits.h>

#include <vector>

#include "common.h"

#include "wave_topk.h"

typedef unsigned long long u64;
#define PAIRS_MAXK 128
#define PAIRS_KNN_TILE 1024  // clean points of one LDS tile (12 KiB)
#define PAIRS_KNN_WAVES 4    // queries of one workgroup
#define PAIRS_WG 1024        // threads of the assignment's workgroup
#define PAIRS_FIN 256        // threads of the finisher's workgroup

// ---- mesh ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pairs_tri_areas_kernel(int nverts, int nfaces, const float *__restrict__ verts,
                                                              const int *__restrict__ faces, double *__restrict__ area,
                                                              int *__restrict__ bad) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= nfaces) return;
  const int ia = faces[(size_t)f * 3], ib = faces[(size_t)f * 3 + 1], ic = faces[(size_t)f * 3 + 2];
  if ((unsigned)ia >= (unsigned)nverts || (unsigned)ib >= (unsigned)nverts || (unsigned)ic >= (unsigned)nverts) {
    area[f] = 0.0;
    *bad = 1;  // (every writer stores the same value)
    return;
  }
  double e1[3], e2[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double pa = (double)verts[(size_t)ia * 3 + a];
    e1[a] = (double)verts[(size_t)ib * 3 + a] - pa;
    e2[a] = (double)verts[(size_t)ic * 3 + a] - pa;
  }
  const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
  area[f] = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
}

__global__ __launch_bounds__(256) void pairs_sample_mesh_kernel(int nverts, int nfaces, int n, const float *__restrict__ verts,
                                                                const float *__restrict__ vcol, const int *__restrict__ faces,
                                                                const double *__restrict__ cdf, const double *__restrict__ u,
                                                                int *__restrict__ face, float *__restrict__ xyz,
                                                                float *__restrict__ rgb) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double target = u[(size_t)i * 3] * cdf[nfaces - 1];
  int lo = 0, hi = nfaces;  // the first f with cdf[f] > target
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    if (cdf[mid] > target) hi = mid; else lo = mid + 1;
  }
  const int f = min(lo, nfaces - 1);
  face[i] = f;
  const int iv[3] = {faces[(size_t)f * 3], faces[(size_t)f * 3 + 1], faces[(size_t)f * 3 + 2]};
  const bool ok = (unsigned)iv[0] < (unsigned)nverts && (unsigned)iv[1] < (unsigned)nverts && (unsigned)iv[2] < (unsigned)nverts;
  const double s = sqrt(u[(size_t)i * 3 + 1]), u2 = u[(size_t)i * 3 + 2];
  const double w0 = 1.0 - s, w1 = s * (1.0 - u2), w2 = s * u2;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float p = NAN, c = NAN;  // (a face that points outside the vertex table: never read, loud in the result)
    if (ok) {
      p = (float)((w0 * (double)verts[(size_t)iv[0] * 3 + a] + w1 * (double)verts[(size_t)iv[1] * 3 + a]) +
                  w2 * (double)verts[(size_t)iv[2] * 3 + a]);
      if (vcol)
        c = (float)((w0 * (double)vcol[(size_t)iv[0] * 3 + a] + w1 * (double)vcol[(size_t)iv[1] * 3 + a]) +
                    w2 * (double)vcol[(size_t)iv[2] * 3 + a]);
    }
    xyz[(size_t)i * 3 + a] = p;
    if (vcol) rgb[(size_t)i * 3 + a] = c;
  }
}

// ---- k-NN ------------------------------------------------------------------------------------------------------------
// A wave's K <= 128 best, as keys (distance bits << 32 | index: distances are >= 0, so the keys order like (distance, index),
// and no two are equal): wave_topk.h's list, two registers per lane.
typedef WaveTopk<u64, PAIRS_MAXK / 64> PairsTopk;

// One wave per query, PAIRS_KNN_WAVES queries of ONE patch per workgroup; the patch's clean points stream through LDS in tiles
// of PAIRS_KNN_TILE (read once per workgroup, coalesced; a wave reads 64 consecutive points of the tile at a stride of three
// words: no bank conflict). Every lane offers one candidate per step; the few below tau are inserted one at a time, in lane
// (= index) order. m >= k is the entry point's to check.
__global__ __launch_bounds__(PAIRS_KNN_WAVES * 64) void pairs_knn_kernel(int s, int k, const float *__restrict__ query,
                                                                         const float *__restrict__ ref,
                                                                         const long long *__restrict__ ref_off,
                                                                         int *__restrict__ idx, float *__restrict__ dist2) {
  __shared__ float tile[PAIRS_KNN_TILE * 3];
  const int p = blockIdx.y, lane = lane_id();
  const int q = blockIdx.x * PAIRS_KNN_WAVES + (int)(threadIdx.x >> 6);
  const bool live = q < s;  // (idle waves still stage tiles and meet the barriers)
  const long long off = ref_off[p];
  const int m = (int)(ref_off[p + 1] - off);
  const float *rp = ref + (size_t)off * 3;
  float qx = 0.0f, qy = 0.0f, qz = 0.0f;
  if (live) {
    const float *qp = query + ((size_t)p * s + q) * 3;
    qx = qp[0], qy = qp[1], qz = qp[2];
  }
  PairsTopk best;
  for (int t0 = 0; t0 < m; t0 += PAIRS_KNN_TILE) {
    const int nt = min(PAIRS_KNN_TILE, m - t0);
    __syncthreads();  // (the previous tile has been read)
    for (int i = threadIdx.x; i < nt * 3; i += PAIRS_KNN_WAVES * 64) tile[i] = rp[(size_t)t0 * 3 + i];
    __syncthreads();
    if (!live) continue;
    for (int j0 = 0; j0 < nt; j0 += 64) {
      const int j = j0 + lane;
      u64 c = ~0ull;
      if (j < nt) {
        const float d = sqdist3(tile[3 * j] - qx, tile[3 * j + 1] - qy, tile[3 * j + 2] - qz);
        c = ((u64)__float_as_uint(d) << 32) | (unsigned)(t0 + j);
      }
      best.offer(c, k, lane);
    }
  }
  if (!live) return;
  const size_t ob = ((size_t)p * s + q) * k;
#pragma unroll
  for (int i = 0; i < PAIRS_MAXK / 64; ++i)
    if (64 * i + lane < k) {
      idx[ob + 64 * i + lane] = (int)(unsigned)best.r[i];
      if (dist2) dist2[ob + 64 * i + lane] = __uint_as_float((unsigned)(best.r[i] >> 32));
    }
}

// ---- unique assignment -----------------------------------------------------------------------------------------------
// Deferred acceptance with a common priority (the lower point index wins), one workgroup per patch. cursor[i] (kept in the
// assign row until the end) = the entry of nn[i] that point i currently proposes to. A round: every point whose cursor is
// below K does atomicMin(owner[target], i); after the barrier a point whose target is owned by a lower index moves its
// cursor on by one. It ends with the first round that moves nobody.
// Why that is the sequential rule: owner[] only ever decreases, and a point leaves a target only when a LOWER index owns it, so
// once owner[t] < i some point below i ends on t -- t is "taken by an earlier point" -- and a point that stays has owner[t]
// == i: every entry before it was taken by earlier points, this one was not. A point whose cursor reaches K holds nothing
// (it only ever left targets that lower indices own) and gets nn[i][0].
// owner is read back with an agent-scope atomic load: the atomics act in L2, a plain load could hit a stale L1 line.
__global__ __launch_bounds__(PAIRS_WG) void pairs_assign_kernel(int s, int k, const int *__restrict__ nn,
                                                               const long long *__restrict__ ref_off, int *owner, int *assign,
                                                               int *__restrict__ unique) {
  __shared__ int moved[2];
  __shared__ int held;
  const int p = blockIdx.x, t = threadIdx.x;
  const long long off = ref_off[p];
  const int m = (int)(ref_off[p + 1] - off);
  int *own = owner + off;
  const int *nnp = nn + (size_t)p * s * k;
  int *cursor = assign + (size_t)p * s;
  for (int j = t; j < m; j += PAIRS_WG) __hip_atomic_store(&own[j], INT_MAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (int i = t; i < s; i += PAIRS_WG) cursor[i] = 0;  // (point i is thread i % PAIRS_WG's alone, in every round)
  if (t == 0) moved[0] = moved[1] = held = 0;
  __threadfence();
  __syncthreads();
  for (int round = 0;; ++round) {
    for (int i = t; i < s; i += PAIRS_WG) {
      const int c = cursor[i];
      if (c < k) {
        const int tg = nnp[(size_t)i * k + c];
        if ((unsigned)tg < (unsigned)m) atomicMin(&own[tg], i);
      }
    }
    __threadfence();
    __syncthreads();
    if (t == 0) moved[(round + 1) & 1] = 0;  // (last read before this barrier, next written after the one below)
    bool mv = false;
    for (int i = t; i < s; i += PAIRS_WG) {
      const int c = cursor[i];
      if (c < k) {
        const int tg = nnp[(size_t)i * k + c];
        if ((unsigned)tg >= (unsigned)m || __hip_atomic_load(&own[tg], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < i) {
          cursor[i] = c + 1;
          mv = true;
        }
      }
    }
    if (mv) moved[round & 1] = 1;
    __syncthreads();
    if (!moved[round & 1]) break;
  }
  int mine = 0;
  for (int i = t; i < s; i += PAIRS_WG) {
    const int c = cursor[i];
    mine += c < k;
    assign[(size_t)p * s + i] = nnp[(size_t)i * k + (c < k ? c : 0)];
  }
  // distinct values = the points that hold a target: holders hold different ones, and a fall-back value nn[i][0] is held
  // (an nn[i][0] outside the patch is held by nobody and not counted: include/p2pb_hip.h)
  if (mine) atomicAdd(&held, mine);
  __syncthreads();
  if (t == 0) unique[p] = held;
}

// ---- finish ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PAIRS_FIN) void pairs_finish_kernel(int s, const float *__restrict__ noisy,
                                                                 const float *__restrict__ noisy_rgb,
                                                                 const float *__restrict__ ref, const float *__restrict__ ref_rgb,
                                                                 const long long *__restrict__ ref_off,
                                                                 const int *__restrict__ assign, float *__restrict__ clean_out,
                                                                 float *__restrict__ noisy_out, float *__restrict__ center,
                                                                 float *__restrict__ scale) {
  __shared__ float tile[PAIRS_FIN * 3];
  __shared__ float cen[3];
  __shared__ float wmax[PAIRS_FIN / 64];
  const int p = blockIdx.x, t = threadIdx.x;
  const float *np_ = noisy + (size_t)p * s * 3;
  // centre: thread a < 3 adds axis a of the rows in index order, PAIRS_FIN rows at a time out of LDS
  double acc = 0.0;
  for (int i0 = 0; i0 < s; i0 += PAIRS_FIN) {
    const int rows = min(PAIRS_FIN, s - i0);
    for (int i = t; i < rows * 3; i += PAIRS_FIN) tile[i] = np_[(size_t)i0 * 3 + i];
    __syncthreads();
    if (t < 3)
      for (int r = 0; r < rows; ++r) acc += (double)tile[r * 3 + t];
    __syncthreads();
  }
  if (t < 3) {
    const float c = (float)(acc / (double)s);
    cen[t] = c;
    center[(size_t)p * 3 + t] = c;
  }
  __syncthreads();
  const float cx = cen[0], cy = cen[1], cz = cen[2];
  float best = 0.0f;
  for (int i = t; i < s; i += PAIRS_FIN) {
    const double dx = (double)(np_[(size_t)i * 3] - cx), dy = (double)(np_[(size_t)i * 3 + 1] - cy),
                 dz = (double)(np_[(size_t)i * 3 + 2] - cz);
    best = fmaxf(best, (float)sqrt((dx * dx + dy * dy) + dz * dz));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = fmaxf(best, __shfl_xor(best, o));
  if ((t & 63) == 0) wmax[t >> 6] = best;
  __syncthreads();
  float sc = wmax[0];
#pragma unroll
  for (int w = 1; w < PAIRS_FIN / 64; ++w) sc = fmaxf(sc, wmax[w]);
  if (t == 0) scale[p] = sc;
  const long long off = ref_off[p];
  const int m = (int)(ref_off[p + 1] - off);
  for (int i = t; i < s; i += PAIRS_FIN) {
    const size_t row = (size_t)p * s + i;
    const int j = assign[row];
    const bool ok = (unsigned)j < (unsigned)m;
    const float *cp = ref + (size_t)(off + (ok ? j : 0)) * 3, *cc = ref_rgb + (size_t)(off + (ok ? j : 0)) * 3;
    const float c[3] = {cx, cy, cz};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      noisy_out[row * 6 + a] = __fdiv_rn(noisy[row * 3 + a] - c[a], sc);
      noisy_out[row * 6 + 3 + a] = noisy_rgb[row * 3 + a];
      clean_out[row * 6 + a] = ok ? __fdiv_rn(cp[a] - c[a], sc) : NAN;
      clean_out[row * 6 + 3 + a] = ok ? cc[a] : NAN;
    }
  }
}

// ---- entry points ----------------------------------------------------------------------------------------------------
// the patch offsets on the host, checked: 0 <= ref_off[0] <= ... <= ref_off[npatch] <= total. Waits for the stream.
static int pairs_offsets(int npatch, int total, const long long *ref_off, hipStream_t st, std::vector<long long> &h) {
  h.resize((size_t)npatch + 1);
  if (hipMemcpyAsync(h.data(), ref_off, h.size() * sizeof(long long), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    const int rc = (int)hipGetLastError();
    return rc ? rc : P2PB_EINVAL;
  }
  if (h[0] < 0 || h[npatch] > total) return P2PB_EINVAL;
  for (int p = 0; p < npatch; ++p)
    if (h[p + 1] < h[p]) return P2PB_EINVAL;
  return 0;
}

extern "C" int p2pb_pairs_tri_areas(int nverts, int nfaces, const float *verts, const int *faces, double *area, int *bad,
                                    void *stream) {
  if (nverts <= 0 || nfaces <= 0 || !verts || !faces || !area || !bad) return P2PB_EINVAL;
  hipLaunchKernelGGL(pairs_tri_areas_kernel, dim3(cdiv(nfaces, 256)), dim3(256), 0, (hipStream_t)stream, nverts, nfaces,
                     verts, faces, area, bad);
  return p2pb_launch_status();
}

extern "C" int p2pb_pairs_sample_mesh(int nverts, int nfaces, int n, const float *verts, const float *vcol, const int *faces,
                                      const double *cdf, const double *u, int *face, float *xyz, float *rgb, void *stream) {
  if (nverts <= 0 || nfaces <= 0 || n <= 0 || !verts || !faces || !cdf || !u || !face || !xyz || (vcol && !rgb))
    return P2PB_EINVAL;
  hipLaunchKernelGGL(pairs_sample_mesh_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, nverts, nfaces, n,
                     verts, vcol, faces, cdf, u, face, xyz, rgb);
  return p2pb_launch_status();
}

extern "C" int p2pb_pairs_knn(int npatch, int s, int k, int total, const float *query, const float *ref,
                              const long long *ref_off, int *idx, float *dist2, void *stream) {
  if (npatch <= 0 || npatch > 65535 || s <= 0 || k < 1 || k > PAIRS_MAXK || total <= 0 || !query || !ref || !ref_off || !idx)
    return P2PB_EINVAL;
  std::vector<long long> h;
  if (const int rc = pairs_offsets(npatch, total, ref_off, (hipStream_t)stream, h)) return rc;
  for (int p = 0; p < npatch; ++p)
    if (h[p + 1] - h[p] < k) return P2PB_EINVAL;
  hipLaunchKernelGGL(pairs_knn_kernel, dim3(cdiv(s, PAIRS_KNN_WAVES), npatch), dim3(PAIRS_KNN_WAVES * 64), 0,
                     (hipStream_t)stream, s, k, query, ref, ref_off, idx, dist2);
  return p2pb_launch_status();
}

extern "C" int p2pb_pairs_unique_assign(int npatch, int s, int k, int total, const int *nn, const long long *ref_off,
                                        int *owner, int *assign, int *unique, void *stream) {
  if (npatch <= 0 || s <= 0 || k < 1 || k > PAIRS_MAXK || total <= 0 || !nn || !ref_off || !owner || !assign || !unique)
    return P2PB_EINVAL;
  std::vector<long long> h;
  if (const int rc = pairs_offsets(npatch, total, ref_off, (hipStream_t)stream, h)) return rc;
  hipLaunchKernelGGL(pairs_assign_kernel, dim3(npatch), dim3(PAIRS_WG), 0, (hipStream_t)stream, s, k, nn, ref_off, owner,
                     assign, unique);
  return p2pb_launch_status();
}

extern "C" int p2pb_pairs_finish(int npatch, int s, int total, const float *noisy, const float *noisy_rgb, const float *ref,
                                 const float *ref_rgb, const long long *ref_off, const int *assign, float *clean_out,
                                 float *noisy_out, float *center, float *scale, void *stream) {
  if (npatch <= 0 || s <= 0 || total <= 0 || !noisy || !noisy_rgb || !ref || !ref_rgb || !ref_off || !assign || !clean_out ||
      !noisy_out || !center || !scale)
    return P2PB_EINVAL;
  std::vector<long long> h;
  if (const int rc = pairs_offsets(npatch, total, ref_off, (hipStream_t)stream, h)) return rc;
  hipLaunchKernelGGL(pairs_finish_kernel, dim3(npatch), dim3(PAIRS_FIN), 0, (hipStream_t)stream, s, noisy, noisy_rgb, ref,
                     ref_rgb, ref_off, assign, clean_out, noisy_out, center, scale);
  return p2pb_launch_status();
}
