// emd.hip -- the two EMD flavours the reference ships.
//   PyTorchEMD approximate matching (metrics/PyTorchEMD/cuda/emd_kernel.cu:33,211,300,347)
//   emd_assignment auction          (metrics/emd_assignment/emd_assignment/emd_cuda.cu:23-226,284)
// The approximate-matching kernels are shared with the set metrics (setmetrics.hip): emd_sweep.h.
#include "emd_sweep.h"
#include <stdlib.h>

// chunks of the inner cloud per launch: enough workgroups for ~4 per CU, chunks of whole LDS tiles of the longer cloud
static int am_chunks(int b, int n, int m) {
  static const long force = p2pb_experiment_long("am_chunks", 0);  // 1: single-pass kernels (A/B and parity experiments)
  if (force == 1) return 1;
  const long base = (long)cdiv(n < m ? n : m, 256) * b;
  const int inner = n > m ? n : m;
  int c = 1;
  while (base * c < 1024 && inner / (c * 2) >= EMD_TILE) c *= 2;
  return c;
}

extern "C" size_t p2pb_approxmatch_temp_floats(int b, int n, int m) {
  const int c = am_chunks(b, n, m);
  return (size_t)b * (n + m) * 2 + (c > 1 ? (size_t)c * b * (n > m ? n : m) : 0);
}

static int approxmatch_impl(int b, int n, int m, const float *xyz1, const float *xyz2, float *match, float *temp,
                            int chunks, void *stream) {
  if (b <= 0 || n <= 0 || m <= 0 || !temp) return P2PB_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  int e = p2pb_zero_async(match, sizeof(float) * (size_t)b * n * m, s);
  if (e != 0) return e;
  emd_anneal(EmdBatched{xyz1, xyz2, temp, match, b}, b, n, m, chunks, s);
  return p2pb_launch_status();
}
// The reference's contract (metrics/PyTorchEMD/cuda/emd_kernel.cu:34): temp = 2 (n + m) b floats. Single-pass kernels, no
// scratch beyond that -- a caller that sizes temp like the reference is always in bounds.
extern "C" int p2pb_approxmatch_forward(int b, int n, int m, const float *xyz1, const float *xyz2, float *match,
                                        float *temp, void *stream) {
  return approxmatch_impl(b, n, m, xyz1, xyz2, match, temp, 1, stream);
}
// The same with an explicit scratch size: temp_floats >= p2pb_approxmatch_temp_floats(b, n, m) lets small batches of large
// clouds split the inner cloud into chunks (partials behind the reference's four arrays: 4 x faster at b = 4, 8192^2);
// a smaller scratch (>= 2 (n + m) b) runs the single-pass kernels; below that P2PB_EINVAL.
extern "C" int p2pb_approxmatch_forward_ws(int b, int n, int m, const float *xyz1, const float *xyz2, float *match,
                                           float *temp, size_t temp_floats, void *stream) {
  if (b <= 0 || n <= 0 || m <= 0 || temp_floats < (size_t)b * (n + m) * 2) return P2PB_EINVAL;
  const int c = am_chunks(b, n, m);
  return approxmatch_impl(b, n, m, xyz1, xyz2, match, temp, temp_floats >= p2pb_approxmatch_temp_floats(b, n, m) ? c : 1, stream);
}

// cost_i = sum_{k,l} d_kl * match[l,k]                                                            (:211-262)
__global__ __launch_bounds__(256) void matchcost_kernel(int n, int m, const float *__restrict__ xyz1,
                                                        const float *__restrict__ xyz2,
                                                        const float *__restrict__ match, float *__restrict__ out) {
  __shared__ float buf[EMD_TILE * 3];
  __shared__ float red[256];
  const int b = blockIdx.y;
  const int k = blockIdx.x * 256 + threadIdx.x;
  const bool ok = k < n;
  const float *p = xyz1 + ((size_t)b * n + (ok ? k : 0)) * 3;
  const float x1 = p[0], y1 = p[1], z1 = p[2];
  const float *mt = match + (size_t)b * n * m;
  float sub = 0;
  for (int l0 = 0; l0 < m; l0 += EMD_TILE) {
    const int ln = min(EMD_TILE, m - l0);
    __syncthreads();
    for (int e = threadIdx.x; e < ln * 3; e += 256) buf[e] = xyz2[((size_t)b * m + l0) * 3 + e];
    __syncthreads();
    if (ok)
      for (int l = 0; l < ln; ++l) {
        const float d = sqdist3(buf[l * 3] - x1, buf[l * 3 + 1] - y1, buf[l * 3 + 2] - z1);
        sub += d * mt[(size_t)(l0 + l) * n + k];
      }
  }
  red[threadIdx.x] = sub;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicAdd(out + b, red[0]);
}

extern "C" int p2pb_matchcost_forward(int b, int n, int m, const float *xyz1, const float *xyz2, const float *match,
                                      float *cost, void *stream) {
  if (b <= 0 || n <= 0 || m <= 0) return P2PB_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  int e = p2pb_zero_async(cost, sizeof(float) * b, s);
  if (e != 0) return e;
  hipLaunchKernelGGL(matchcost_kernel, dim3(cdiv(n, 256), b), dim3(256), 0, s, n, m, xyz1, xyz2, match, cost);
  return p2pb_launch_status();
}

// grad1_l = grad_cost * sum_k 2*match[k,l]*(x1_l - x2_k)                                           (:347-375)
__global__ __launch_bounds__(256) void matchcost_grad1_kernel(int n, int m, const float *__restrict__ grad_cost,
                                                              const float *__restrict__ xyz1,
                                                              const float *__restrict__ xyz2,
                                                              const float *__restrict__ match,
                                                              float *__restrict__ grad1) {
  const int b = blockIdx.y;
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l >= n) return;
  const float *p = xyz1 + ((size_t)b * n + l) * 3;
  const float x1 = p[0], y1 = p[1], z1 = p[2];
  const float *mt = match + (size_t)b * n * m;
  float dx = 0, dy = 0, dz = 0;
  for (int k = 0; k < m; ++k) {
    const float *q = xyz2 + ((size_t)b * m + k) * 3;
    const float d = mt[(size_t)k * n + l] * 2;
    dx += (x1 - q[0]) * d;
    dy += (y1 - q[1]) * d;
    dz += (z1 - q[2]) * d;
  }
  const float gc = grad_cost[b];
  float *g = grad1 + ((size_t)b * n + l) * 3;
  g[0] = dx * gc;
  g[1] = dy * gc;
  g[2] = dz * gc;
}

// grad2_k = grad_cost * sum_j 2*match[k,j]*(x2_k - x1_j) : one workgroup per target point          (:300-345)
__global__ __launch_bounds__(256) void matchcost_grad2_kernel(int n, int m, const float *__restrict__ grad_cost,
                                                              const float *__restrict__ xyz1,
                                                              const float *__restrict__ xyz2,
                                                              const float *__restrict__ match,
                                                              float *__restrict__ grad2) {
  __shared__ float red[3][256];
  const int b = blockIdx.y, k = blockIdx.x;
  const float *q = xyz2 + ((size_t)b * m + k) * 3;
  const float x2 = q[0], y2 = q[1], z2 = q[2];
  const float *row = match + (size_t)b * n * m + (size_t)k * n;
  float sx = 0, sy = 0, sz = 0;
  for (int j = threadIdx.x; j < n; j += 256) {
    const float *p = xyz1 + ((size_t)b * n + j) * 3;
    const float d = row[j] * 2;
    sx += (x2 - p[0]) * d;
    sy += (y2 - p[1]) * d;
    sz += (z2 - p[2]) * d;
  }
  red[0][threadIdx.x] = sx;
  red[1][threadIdx.x] = sy;
  red[2][threadIdx.x] = sz;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      red[0][threadIdx.x] += red[0][threadIdx.x + s];
      red[1][threadIdx.x] += red[1][threadIdx.x + s];
      red[2][threadIdx.x] += red[2][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) grad2[((size_t)b * m + k) * 3 + threadIdx.x] = red[threadIdx.x][0] * grad_cost[b];
}

extern "C" int p2pb_matchcost_backward(int b, int n, int m, const float *grad_cost, const float *xyz1,
                                       const float *xyz2, const float *match, float *grad1, float *grad2,
                                       void *stream) {
  if (b <= 0 || n <= 0 || m <= 0) return P2PB_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(matchcost_grad1_kernel, dim3(cdiv(n, 256), b), dim3(256), 0, s, n, m, grad_cost, xyz1, xyz2, match,
                     grad1);
  hipLaunchKernelGGL(matchcost_grad2_kernel, dim3(m, b), dim3(256), 0, s, n, m, grad_cost, xyz1, xyz2, match, grad2);
  return p2pb_launch_status();
}

// ------------------------------------------------------------------------------------------------
// Auction assignment. The reference spends 7 launches per round (clear / count / scan / compact /
// Bid / GetMax / Assign); here a round is 3 launches: one WAVE per bidder (assigned bidders exit at
// once, so no compaction pass is needed), then GetMax and Assign as in the reference.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float atomic_max_f32(float *address, float val) {  // emd_cuda.cu:10-20
  int ret = __float_as_int(*address);
  while (val > __int_as_float(ret)) {
    int old = ret;
    if ((ret = atomicCAS((int *)address, old, __float_as_int(val))) == old) break;
  }
  return __int_as_float(ret);
}

// the auction's arrays (emd_cuda.cu's names), of the whole batch or of one cloud of it
struct Auction {
  int *assignment, *assignment_inv;
  float *price;
  int *bid;
  float *bid_increments, *max_increments;
  int *max_idx;
  __device__ __forceinline__ Auction cloud(size_t o) const {
    return {assignment + o, assignment_inv + o, price + o, bid + o, bid_increments + o, max_increments + o, max_idx + o};
  }
};

// Bid, one lane: best and runner-up value of bidder `p` over the objects lane, lane + 64, ...; fetch(k) -> (x, y, z, price)
template <class Fetch>
__device__ __forceinline__ void auction_lane_bid(int n, const float *p, Fetch fetch, float &best, float &better, int &best_i) {
  const float x1 = p[0], y1 = p[1], z1 = p[2];
  best = -1e9f, better = -1e9f, best_i = -1;
  for (int k = lane_id(); k < n; k += 64) {
    const float4 q = fetch(k);
    // emd_cuda.cu:146 : `3.0 - sqrtf(..) - price` is evaluated in double (3.0 is a double literal)
    const float d = (float)((3.0 - (double)sqrtf(sqdist3(q.x - x1, q.y - y1, q.z - z1))) - (double)q.w);
    if (d > best) {
      better = best;
      best = d;
      best_i = k;
    } else if (d > better) {
      better = d;
    }
  }
}

// Bid, the wave of bidder j: merge (best, better, best_i) across lanes -- lowest k wins value ties, `better` is the runner-up --
// and place the bid
__device__ __forceinline__ void auction_wave_bid(const Auction &a, int j, float eps, float best, float better, int best_i) {
  for (int off = 32; off > 0; off >>= 1) {
    const float ob = __shfl_xor(best, off), obt = __shfl_xor(better, off);
    const int oi = __shfl_xor(best_i, off);
    const bool take = (ob > best) || (ob == best && oi >= 0 && (best_i < 0 || oi < best_i));
    if (take) {
      better = fmaxf(best, obt);
      best = ob;
      best_i = oi;
    } else {
      better = fmaxf(better, ob);
    }
  }
  if (lane_id() == 0) {
    const float inc = best - better + eps;
    a.bid[j] = best_i;
    a.bid_increments[j] = inc;
    atomic_max_f32(a.max_increments + best_i, inc);
  }
}

// GetMax of unassigned bidder j: whoever bid the object's highest increment (within 1e-6) is its winner
__device__ __forceinline__ void auction_getmax(const Auction &a, int j) {
  const int bid_id = a.bid[j];
  const float bid_inc = a.bid_increments[j];
  const float max_inc = a.max_increments[bid_id];
  if ((double)bid_inc - 1e-6 <= (double)max_inc && (double)max_inc <= (double)bid_inc + 1e-6) a.max_idx[bid_id] = j;
}

// Assign of unassigned bidder j: the winner (in the last round every bidder) takes its object from the previous holder and
// raises the price. Returns the object and its new price, -1 when j did not win.
__device__ __forceinline__ int auction_assign(const Auction &a, int j, int last, float *new_price) {
  const int bid_id = a.bid[j];
  if (!(last || a.max_idx[bid_id] == j)) return -1;
  const float bid_inc = a.bid_increments[j];
  const int ass_inv = a.assignment_inv[bid_id];
  if (!last && ass_inv != -1) a.assignment[ass_inv] = -1;
  a.assignment_inv[bid_id] = j;
  a.assignment[j] = bid_id;
  *new_price = a.price[bid_id] + bid_inc;
  a.price[bid_id] = *new_price;
  a.max_increments[bid_id] = -1e9f;
  return bid_id;
}

__global__ __launch_bounds__(256) void auction_bid_kernel(int n, const float *__restrict__ xyz1,
                                                          const float *__restrict__ xyz2, float eps, Auction batch) {
  const size_t o = (size_t)blockIdx.y * n;
  const Auction a = batch.cloud(o);
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= n || a.assignment[j] != -1) return;
  const float *q = xyz2 + o * 3;
  float best, better;
  int best_i;
  auction_lane_bid(n, xyz1 + (o + j) * 3, [&](int k) { return make_float4(q[k * 3], q[k * 3 + 1], q[k * 3 + 2], a.price[k]); },
                   best, better, best_i);
  auction_wave_bid(a, j, eps, best, better, best_i);
}

__global__ __launch_bounds__(256) void auction_getmax_kernel(int n, Auction batch) {
  const Auction a = batch.cloud((size_t)blockIdx.y * n);
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < n && a.assignment[j] == -1) auction_getmax(a, j);
}

__global__ __launch_bounds__(256) void auction_assign_kernel(int n, Auction batch, int last) {
  const Auction a = batch.cloud((size_t)blockIdx.y * n);
  const int j = blockIdx.x * 256 + threadIdx.x;
  float np;
  if (j < n && a.assignment[j] == -1) auction_assign(a, j, last, &np);
}

__global__ __launch_bounds__(256) void auction_dist_kernel(int n, const float *__restrict__ xyz1,
                                                           const float *__restrict__ xyz2, float *__restrict__ dist,
                                                           const int *__restrict__ assignment) {
  const int b = blockIdx.y;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int k = assignment[(size_t)b * n + j];
  const float *p = xyz1 + ((size_t)b * n + j) * 3, *q = xyz2 + ((size_t)b * n + k) * 3;
  dist[(size_t)b * n + j] = sqdist3(p[0] - q[0], p[1] - q[1], p[2] - q[2]);
}

// Rounds [first, iters) of the auction as ONE launch (round 6): one 1024-thread workgroup per cloud runs the three phases of
// every remaining round itself, separated by workgroup barriers instead of kernel boundaries. After the first few rounds an
// auction round is pure latency -- a few dozen unassigned bidders, three dependent launches (19.7 us per round at 8 x 2048:
// the training alignment's 2.0 ms) -- while the FIRST rounds are n^2 distance evaluations that want the whole chip: the
// launcher runs those as before and hands the tail to this kernel. Objects (x, y, z, price) live in LDS as 16-byte records; the
// unassigned bidders are listed (ascending) at the top of every round, so a bidder that loses its object during Assign bids
// again in the next round -- one of the interleavings the reference's racing Assign kernel can produce. The bid, GetMax and
// Assign steps are the functions the per-round kernels call, and the final state is in the caller's buffers.
// n <= 8192 (LDS: 16 n + 2 n bytes).
#define AUC_T 1024
__global__ __launch_bounds__(AUC_T) void auction_persist_kernel(int n, const float *__restrict__ xyz1,
                                                                const float *__restrict__ xyz2, float eps, Auction batch,
                                                                int first, int iters) {
  extern __shared__ float4 auc_lds[];
  float4 *obj = auc_lds;                             // [n] (x, y, z, price)
  unsigned short *list = (unsigned short *)(obj + n);  // [n] unassigned bidders, ascending
  __shared__ int wcnt[AUC_T / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t o = (size_t)b * n;
  const Auction a = batch.cloud(o);
  for (int k = tid; k < n; k += AUC_T) {
    const float *q = xyz2 + (o + k) * 3;
    obj[k] = make_float4(q[0], q[1], q[2], a.price[k]);
  }
  __syncthreads();
  for (int it = first; it < iters; ++it) {
    const int last = it == iters - 1;
    // ---- the round's unassigned bidders, ascending (ballot + scan; chunks of AUC_T bidders)
    int base = 0;
    for (int j0 = 0; j0 < n; j0 += AUC_T) {
      const int j = j0 + tid;
      const bool un = j < n && a.assignment[j] == -1;
      const unsigned long long m = __ballot(un);
      if (lane == 0) wcnt[wave] = __popcll(m);
      __syncthreads();
      int before = base;
      for (int w = 0; w < wave; ++w) before += wcnt[w];
      if (un) list[before + mbcnt(m)] = (unsigned short)j;
      int all = 0;
      for (int w = 0; w < AUC_T / 64; ++w) all += wcnt[w];
      base += all;
      __syncthreads();
    }
    const int nun = base;  // (workgroup-uniform)
    if (nun == 0) break;   // every bidder holds an object: the remaining rounds change nothing
    // ---- Bid: one wave per unassigned bidder, the objects from the LDS records
    for (int u = wave; u < nun; u += AUC_T / 64) {
      const int j = list[u];
      float best, better;
      int best_i;
      auction_lane_bid(n, xyz1 + (o + j) * 3, [&](int k) { return obj[k]; }, best, better, best_i);
      auction_wave_bid(a, j, eps, best, better, best_i);
    }
    __syncthreads();
    for (int u = tid; u < nun; u += AUC_T) auction_getmax(a, list[u]);
    __syncthreads();
    // ---- Assign; the winner keeps the LDS price in step with the caller's buffer
    for (int u = tid; u < nun; u += AUC_T) {
      float np;
      const int won = auction_assign(a, list[u], last, &np);
      if (won >= 0) obj[won].w = np;
    }
    __syncthreads();
  }
}

extern "C" int p2pb_auction_forward(int b, int n, int m, const float *xyz1, const float *xyz2, float *dist,
                                    int *assignment, float *price, int *assignment_inv, int *bid,
                                    float *bid_increments, float *max_increments, int *unass_idx, int *unass_cnt,
                                    int *unass_cnt_sum, int *cnt_tmp, int *max_idx, float eps, int iters,
                                    void *stream) {
  (void)unass_idx, (void)unass_cnt, (void)unass_cnt_sum, (void)cnt_tmp;  // the compaction pass is not needed here
  if (n != m || b > 512 || n % 128 != 0 || b <= 0 || n <= 0) return -1;  // emd_cuda.cu:236-249
  hipStream_t s = (hipStream_t)stream;
  // the first rounds (n^2 distance evaluations each: the whole chip) as three launches per round, the latency-bound tail as
  // one persistent launch (auction_persist_kernel); P2PB_EXPERIMENT="auction_persist_from=K" moves the hand-over (K >= iters: off)
  const long persist_from = p2pb_experiment_long("auction_persist_from", 10);  // (read per call: tests switch it)
  const int head = (n <= 8192 && persist_from < iters) ? (int)(persist_from < 0 ? 0 : persist_from) : iters;
  const Auction a = {assignment, assignment_inv, price, bid, bid_increments, max_increments, max_idx};
  // The persistent launch takes more LDS than the 64 KB a kernel gets unasked from n = 3712 on. The opt-in holds per device,
  // so it is made at every such call (host-only, one per auction) for the device the call runs on; a refusal is this call's
  // error, before anything is launched.
  const size_t lds = (size_t)n * 18;
  if (head < iters && lds > 64 * 1024 &&
      hipFuncSetAttribute((const void *)auction_persist_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024) !=
          hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  for (int i = 0; i < head; ++i) {
    hipLaunchKernelGGL(auction_bid_kernel, dim3(cdiv(n, 4), b), dim3(256), 0, s, n, xyz1, xyz2, eps, a);
    hipLaunchKernelGGL(auction_getmax_kernel, dim3(cdiv(n, 256), b), dim3(256), 0, s, n, a);
    hipLaunchKernelGGL(auction_assign_kernel, dim3(cdiv(n, 256), b), dim3(256), 0, s, n, a, (int)(i == iters - 1));
  }
  if (head < iters)
    hipLaunchKernelGGL(auction_persist_kernel, dim3(b), dim3(AUC_T), lds, s, n, xyz1, xyz2, eps, a, head, iters);
  hipLaunchKernelGGL(auction_dist_kernel, dim3(cdiv(n, 256), b), dim3(256), 0, s, n, xyz1, xyz2, dist, assignment);
  return p2pb_launch_status() == 0 ? 1 : 0;
}

__global__ __launch_bounds__(256) void auction_grad_kernel(int n, const float *__restrict__ xyz1,
                                                           const float *__restrict__ xyz2,
                                                           const float *__restrict__ grad_dist,
                                                           const int *__restrict__ idx, float *grad_xyz) {
  const int b = blockIdx.y;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int j2 = idx[(size_t)b * n + j];
  const float *p = xyz1 + ((size_t)b * n + j) * 3, *q = xyz2 + ((size_t)b * n + j2) * 3;
  const float g = grad_dist[(size_t)b * n + j] * 2;
  float *o = grad_xyz + ((size_t)b * n + j) * 3;
#pragma unroll
  for (int a = 0; a < 3; ++a) atomicAdd(o + a, g * (p[a] - q[a]));
}

extern "C" int p2pb_auction_backward(int b, int n, const float *xyz1, const float *xyz2, float *gradxyz,
                                     const float *graddist, const int *idx, void *stream) {
  if (b <= 0 || n <= 0) return P2PB_EINVAL;
  hipLaunchKernelGGL(auction_grad_kernel, dim3(cdiv(n, 256), b), dim3(256), 0, (hipStream_t)stream, n, xyz1, xyz2,
                     graddist, idx, gradxyz);
  return p2pb_launch_status() == 0 ? 1 : 0;
}
