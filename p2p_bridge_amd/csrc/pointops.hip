// pointops.hip -- the packed-batch ("offset") operators of the reference's pointops extension
// (PO = third_party/openpoints/cpp/pointops/src; include/p2pb_hip.h, section "packed-batch operators"):
//   p2pb_pointops_knnquery            (PO/knnquery/knnquery_cuda_kernel.cu:65)
//   p2pb_pointops_ballquery           (PO/ballquery/ballquery_cuda_kernel.cu:26)
//   p2pb_pointops_{grouping,interpolation,subtraction,aggregation}_{forward,backward}
// (p2pb_pointops_furthestsampling of the same extension is in fps_ref.hip, with the PointNet++ sampler it shares its kernels
// with.) One packed cloud xyz f32[n,3] with cumulative segment ends offset i32[b]; features point-major f32[n,c]. The caller
// owns every output. Squared distances are sqdist3 (common.h) of query - point.
#include "common.h"
#include "po_segment.h"

typedef unsigned long long u64;  // the k-NN heap's keys

// ------------------------------------------------------------------------------------------------
// segments. Query i belongs to the first segment s with i < new_offset[s]; the search ends in [0, b-1] whatever the array
// holds, ends are clamped to [0, n], an end below its start is an empty segment (po_segment.h).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int po_segment_of(int i, int b, const int *__restrict__ new_offset) {
  int lo = 0, hi = b - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (i < new_offset[mid]) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

__device__ __forceinline__ int po_wave_min(int v) {
#pragma unroll
  for (int d = 32; d; d >>= 1) v = min(v, __shfl_xor(v, d));
  return v;
}
__device__ __forceinline__ int po_wave_max(int v) {
#pragma unroll
  for (int d = 32; d; d >>= 1) v = max(v, __shfl_xor(v, d));
  return v;
}
__device__ __forceinline__ float po_lane_f32(float v, int j) {  // v of lane j (wave-uniform j) in every lane
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), j));
}

// One lane per query, one wave per workgroup. The wave walks the union [lo, hi) of its lanes' segment ranges 64 points at
// a time: each lane loads one point, the wave then takes them one by one out of the registers (v_readlane: the point is
// wave-uniform, no LDS), and each lane masks by its own bounds. hit(k, d2) sees the lane's points in ascending k, each() runs
// behind every point with the whole wave; the walk ends early once done() holds in every lane.
struct PoQuery {
  float x, y, z;
  int start, end;  // the lane's segment; start == end: no query in this lane
  int lo, hi;      // wave-uniform
};
__device__ __forceinline__ PoQuery po_query(int q, int b, int n, int m, const float *__restrict__ new_xyz,
                                            const int *__restrict__ offset, const int *__restrict__ new_offset) {
  PoQuery Q;
  Q.x = Q.y = Q.z = 0.0f;
  Q.start = Q.end = 0;
  if (q < m) {
    Q.x = new_xyz[(size_t)3 * q];
    Q.y = new_xyz[(size_t)3 * q + 1];
    Q.z = new_xyz[(size_t)3 * q + 2];
    po_segment_points(po_segment_of(q, b, new_offset), n, offset, Q.start, Q.end);
  }
  Q.lo = __builtin_amdgcn_readfirstlane(po_wave_min(q < m ? Q.start : n));
  Q.hi = __builtin_amdgcn_readfirstlane(po_wave_max(Q.end));
  return Q;
}
template <class Hit, class Each, class Done>
__device__ __forceinline__ void po_walk(const PoQuery &Q, const float *__restrict__ xyz, Hit &&hit, Each &&each, Done &&done) {
  const int lane = lane_id();
  for (int base = Q.lo; base < Q.hi; base += 64) {
    const int k = min(base + lane, Q.hi - 1);
    const float px = xyz[(size_t)3 * k], py = xyz[(size_t)3 * k + 1], pz = xyz[(size_t)3 * k + 2];
    const int cnt = min(64, Q.hi - base);
    for (int j = 0; j < cnt; ++j) {
      const float d2 = sqdist3(Q.x - po_lane_f32(px, j), Q.y - po_lane_f32(py, j), Q.z - po_lane_f32(pz, j));
      const int kk = base + j;
      if (kk >= Q.start && kk < Q.end) hit(kk, d2);
      each();
    }
    if (__all(done())) break;
  }
}

// ------------------------------------------------------------------------------------------------
// k nearest neighbours, k = nsample <= 100. Each lane keeps its best list as a max-heap of 64-bit keys
// (distance bits << 32 | point index) in LDS, laid out [slot][lane] (8 B per lane and slot: 64 lanes fill two bank rows,
// no conflict), and the distance of the heap's root -- the admission threshold -- in a register: a point that is not
// admitted costs the three differences, the fma chain and one compare. Points arrive in ascending index, so strict '<'
// on the distance is strict '<' on the key and the heap ends holding the nsample smallest keys: equal distances rank by
// ascending index. A heap sort in place orders them; the wave then writes its rows lane-consecutive.
// An admission is a dependent chain of LDS round trips that the whole wave waits for, and the lanes admit at different
// points, so a point that passes the threshold is only appended to a small per-lane list (also [slot][lane] in LDS); when
// any lane's list is full, every lane works its list off, in order and against its current threshold -- the same
// admissions with the same outcome, but the wave stalls once per PO_KNN_BUF of them instead of once each.
// ------------------------------------------------------------------------------------------------
#define PO_KNN_MAX 100
#define PO_KNN_BUF 8
// the heap h[0 .. size) of this lane with its root replaced by v (v <= the old root, or the old root is being removed)
__device__ __forceinline__ void po_heap_replace_root(u64 *h, int size, u64 v) {
  int i = 0;
  for (;;) {
    int c = 2 * i + 1;
    if (c >= size) break;
    u64 kc = h[c * 64];
    if (c + 1 < size) {
      const u64 kr = h[(c + 1) * 64];
      if (kr > kc) {
        kc = kr;
        ++c;
      }
    }
    if (kc <= v) break;
    h[i * 64] = kc;
    i = c;
  }
  h[i * 64] = v;
}

__global__ __launch_bounds__(64) void po_knn_kernel(int b, int n, int m, int ns, const float *__restrict__ xyz,
                                                    const float *__restrict__ new_xyz, const int *__restrict__ offset,
                                                    const int *__restrict__ new_offset, int *__restrict__ idx,
                                                    float *__restrict__ dist2) {
  extern __shared__ u64 po_knn_heap[];  // [ns][64], then the candidate lists [PO_KNN_BUF][64]
  const int lane = lane_id();
  const int q0 = blockIdx.x * 64;
  const PoQuery Q = po_query(q0 + lane, b, n, m, new_xyz, offset, new_offset);
  u64 *h = po_knn_heap + lane;
  // (a segment that ends the cloud and is empty starts at n: its padding index is held inside the cloud)
  const u64 pad = ((u64)__float_as_uint(1e10f) << 32) | (unsigned)min(Q.start, n - 1);
  for (int s = 0; s < ns; ++s) h[s * 64] = pad;
  u64 *cand = po_knn_heap + ns * 64 + lane;
  float thr = 1e10f;
  int ncand = 0;
  auto admit = [&] {
    for (int i = 0; i < ncand; ++i) {
      const u64 v = cand[i * 64];
      if (__uint_as_float((unsigned)(v >> 32)) < thr) {
        po_heap_replace_root(h, ns, v);
        thr = __uint_as_float((unsigned)(h[0] >> 32));
      }
    }
    ncand = 0;
  };
  po_walk(
      Q, xyz,
      [&](int k, float d2) {
        if (d2 < thr) cand[ncand++ * 64] = ((u64)__float_as_uint(d2) << 32) | (unsigned)k;
      },
      [&] {
        if (__any(ncand == PO_KNN_BUF)) admit();
      },
      [] { return false; });
  admit();
  for (int e = ns - 1; e > 0; --e) {  // heap sort: the largest of h[0 .. e] goes to slot e
    const u64 last = h[e * 64];
    h[e * 64] = h[0];
    po_heap_replace_root(h, e, last);
  }
  __syncthreads();
  const int rows = min(64, m - q0);
  const size_t out0 = (size_t)q0 * ns;
  for (int e = lane; e < rows * ns; e += 64) {
    const u64 key = po_knn_heap[(e % ns) * 64 + e / ns];
    idx[out0 + e] = (int)(unsigned)key;
    dist2[out0 + e] = __uint_as_float((unsigned)(key >> 32));
  }
}

extern "C" int p2pb_pointops_knnquery(int b, int n, int m, int nsample, const float *xyz, const float *new_xyz,
                                      const int *offset, const int *new_offset, int *idx, float *dist2, void *stream) {
  if (b < 0 || n < 0 || m < 0 || nsample < 1 || nsample > PO_KNN_MAX) return P2PB_EINVAL;
  if (m == 0) return 0;
  if (b == 0 || n == 0 || !xyz || !new_xyz || !offset || !new_offset || !idx || !dist2) return P2PB_EINVAL;
  hipLaunchKernelGGL(po_knn_kernel, dim3(cdiv(m, 64)), dim3(64), (size_t)(nsample + PO_KNN_BUF) * 64 * sizeof(u64), (hipStream_t)stream, b,
                     n, m, nsample, xyz, new_xyz, offset, new_offset, idx, dist2);
  return p2pb_launch_status();
}

// ------------------------------------------------------------------------------------------------
// ball query on the same walk: a lane counts its hits and writes them to its row as they come; the walk ends once every
// lane of the wave has nsample of them. The slots behind the last hit get the first one; a query without a hit writes
// nothing.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void po_ballquery_kernel(int b, int n, int m, float r2, int ns,
                                                          const float *__restrict__ xyz, const float *__restrict__ new_xyz,
                                                          const int *__restrict__ offset,
                                                          const int *__restrict__ new_offset, int *__restrict__ idx) {
  const int q = blockIdx.x * 64 + lane_id();
  const PoQuery Q = po_query(q, b, n, m, new_xyz, offset, new_offset);
  int *o = idx + (size_t)min(q, m - 1) * ns;  // (a lane without a query has an empty range and never writes)
  int cnt = 0, first = 0;
  po_walk(
      Q, xyz,
      [&](int k, float d2) {
        if (d2 < r2 && cnt < ns) {
          if (cnt == 0) first = k;
          o[cnt++] = k;
        }
      },
      [] {}, [&] { return cnt >= ns || Q.start == Q.end; });
  if (cnt > 0)
    for (int s = cnt; s < ns; ++s) o[s] = first;
}

extern "C" int p2pb_pointops_ballquery(int b, int n, int m, float radius, int nsample, const float *xyz,
                                       const float *new_xyz, const int *offset, const int *new_offset, int *idx,
                                       void *stream) {
  if (b < 0 || n < 0 || m < 0 || nsample < 1) return P2PB_EINVAL;
  if (m == 0) return 0;
  if (b == 0 || n == 0 || !xyz || !new_xyz || !offset || !new_offset || !idx) return P2PB_EINVAL;
  const float r2 = radius * radius;  // the float product of PO/ballquery/ballquery_cuda_kernel.cu
  hipLaunchKernelGGL(po_ballquery_kernel, dim3(cdiv(m, 64)), dim3(64), 0, (hipStream_t)stream, b, n, m, r2, nsample, xyz,
                     new_xyz, offset, new_offset, idx);
  return p2pb_launch_status();
}

// ------------------------------------------------------------------------------------------------
// the arithmetic operators: one thread per element of the widest operand, channels fastest, so rows of c floats are read
// and written lane-consecutive. Element counts are 64-bit. The scatter-adds are global_atomic_add_f32 in no fixed order.
// ------------------------------------------------------------------------------------------------
#define PO_THREADS 256
// total = a * b * c elements, one thread each -> 1 with the grid, 0 for nothing to do, P2PB_EINVAL for a negative size or
// more elements than a grid holds
static inline int po_grid(int a, int b, int c, long &total, unsigned &grid) {
  if (a < 0 || b < 0 || c < 0) return P2PB_EINVAL;
  const long ab = (long)a * b, limit = (long)0x7fffffff * PO_THREADS;
  total = 0;
  if (ab == 0 || c == 0) return 0;
  if (c > limit / ab) return P2PB_EINVAL;
  total = ab * c;
  grid = cdiv(total, PO_THREADS);
  return 1;
}
#define PO_ELEMENT(e, total)                                           \
  const long e = (long)blockIdx.x * PO_THREADS + (long)threadIdx.x;    \
  if (e >= (total)) return

template <bool GRAD>  // rows = m * nsample rows of c floats: out[row] = in[idx[row]] | in[idx[row]] += out[row]
__global__ __launch_bounds__(PO_THREADS) void po_grouping_kernel(long total, int c, const int *__restrict__ idx,
                                                                 const float *__restrict__ src, float *dst) {
  PO_ELEMENT(e, total);
  const long row = e / c;
  const int ch = (int)(e - row * c);
  if (GRAD) atomicAdd(dst + (size_t)idx[row] * c + ch, src[e]);
  else dst[e] = src[(size_t)idx[row] * c + ch];
}

extern "C" int p2pb_pointops_grouping_forward(int m, int nsample, int c, const float *input, const int *idx, float *output,
                                              void *stream) {
  long total;
  unsigned grid;
  const int rc = po_grid(m, nsample, c, total, grid);
  if (rc <= 0) return rc;
  if (!input || !idx || !output) return P2PB_EINVAL;
  hipLaunchKernelGGL(po_grouping_kernel<false>, dim3(grid), dim3(PO_THREADS), 0, (hipStream_t)stream, total, c, idx, input,
                     output);
  return p2pb_launch_status();
}

extern "C" int p2pb_pointops_grouping_backward(int n, int m, int nsample, int c, const float *grad_output, const int *idx,
                                               float *grad_input, void *stream) {
  long total;
  unsigned grid;
  const int rc = n < 0 ? P2PB_EINVAL : po_grid(m, nsample, c, total, grid);
  if (rc <= 0) return rc;
  if (n == 0 || !grad_output || !idx || !grad_input || p2pb_deterministic()) return P2PB_EINVAL;
  hipLaunchKernelGGL(po_grouping_kernel<true>, dim3(grid), dim3(PO_THREADS), 0, (hipStream_t)stream, total, c, idx,
                     grad_output, grad_input);
  return p2pb_launch_status();
}

// thread (row, ch) of n rows: forward dst[row] = fma chain over the row's k (idx, weight) pairs, starting from dst[row];
// gradient: src[row] * w_i added at idx_i
template <bool GRAD>
__global__ __launch_bounds__(PO_THREADS) void po_interpolation_kernel(long total, int c, int k, const float *__restrict__ src,
                                                                      const int *__restrict__ idx,
                                                                      const float *__restrict__ weight, float *dst) {
  PO_ELEMENT(e, total);
  const long row = e / c;
  const int ch = (int)(e - row * c);
  const int *id = idx + row * k;
  const float *w = weight + row * k;
  if (GRAD) {
    const float g = src[e];
    for (int i = 0; i < k; ++i) atomicAdd(dst + (size_t)id[i] * c + ch, g * w[i]);
  } else {
    float acc = dst[e];
    for (int i = 0; i < k; ++i) acc = __fmaf_rn(src[(size_t)id[i] * c + ch], w[i], acc);
    dst[e] = acc;
  }
}

extern "C" int p2pb_pointops_interpolation_forward(int n, int c, int k, const float *input, const int *idx,
                                                   const float *weight, float *output, void *stream) {
  long total;
  unsigned grid;
  const int rc = k < 0 ? P2PB_EINVAL : po_grid(n, c, 1, total, grid);
  if (rc <= 0 || k == 0) return rc < 0 ? rc : 0;
  if (!input || !idx || !weight || !output) return P2PB_EINVAL;
  hipLaunchKernelGGL(po_interpolation_kernel<false>, dim3(grid), dim3(PO_THREADS), 0, (hipStream_t)stream, total, c, k, input,
                     idx, weight, output);
  return p2pb_launch_status();
}

extern "C" int p2pb_pointops_interpolation_backward(int n, int c, int k, const float *grad_output, const int *idx,
                                                    const float *weight, float *grad_input, void *stream) {
  long total;
  unsigned grid;
  const int rc = k < 0 ? P2PB_EINVAL : po_grid(n, c, 1, total, grid);
  if (rc <= 0 || k == 0) return rc < 0 ? rc : 0;
  if (!grad_output || !idx || !weight || !grad_input || p2pb_deterministic()) return P2PB_EINVAL;
  hipLaunchKernelGGL(po_interpolation_kernel<true>, dim3(grid), dim3(PO_THREADS), 0, (hipStream_t)stream, total, c, k,
                     grad_output, idx, weight, grad_input);
  return p2pb_launch_status();
}

// thread (row, s, ch): output = input1[row] - input2[idx[row, s]]
__global__ __launch_bounds__(PO_THREADS) void po_subtraction_forward_kernel(long total, int c, int ns,
                                                                            const float *__restrict__ input1,
                                                                            const float *__restrict__ input2,
                                                                            const int *__restrict__ idx,
                                                                            float *__restrict__ output) {
  PO_ELEMENT(e, total);
  const long rs = e / c;
  const int ch = (int)(e - rs * c);
  output[e] = input1[(rs / ns) * c + ch] - input2[(size_t)idx[rs] * c + ch];
}
// thread (row, s, ch): -grad_output added to grad_input2 at idx[row, s]
__global__ __launch_bounds__(PO_THREADS) void po_subtraction_scatter_kernel(long total, int c,
                                                                            const float *__restrict__ grad_output,
                                                                            const int *__restrict__ idx, float *grad_input2) {
  PO_ELEMENT(e, total);
  const long rs = e / c;
  atomicAdd(grad_input2 + (size_t)idx[rs] * c + (int)(e - rs * c), -grad_output[e]);
}
// thread (row, ch): grad_input1[row] += grad_output[row, s] for s ascending
__global__ __launch_bounds__(PO_THREADS) void po_subtraction_rowsum_kernel(long total, int c, int ns,
                                                                           const float *__restrict__ grad_output,
                                                                           float *__restrict__ grad_input1) {
  PO_ELEMENT(e, total);
  const long row = e / c;
  const int ch = (int)(e - row * c);
  const float *g = grad_output + row * ns * c + ch;
  float acc = grad_input1[e];
  for (int s = 0; s < ns; ++s) acc += g[(size_t)s * c];
  grad_input1[e] = acc;
}

extern "C" int p2pb_pointops_subtraction_forward(int n, int nsample, int c, const float *input1, const float *input2,
                                                 const int *idx, float *output, void *stream) {
  long total;
  unsigned grid;
  const int rc = po_grid(n, nsample, c, total, grid);
  if (rc <= 0) return rc;
  if (!input1 || !input2 || !idx || !output) return P2PB_EINVAL;
  hipLaunchKernelGGL(po_subtraction_forward_kernel, dim3(grid), dim3(PO_THREADS), 0, (hipStream_t)stream, total, c, nsample,
                     input1, input2, idx, output);
  return p2pb_launch_status();
}

extern "C" int p2pb_pointops_subtraction_backward(int n, int nsample, int c, const int *idx, const float *grad_output,
                                                  float *grad_input1, float *grad_input2, void *stream) {
  long total, rows;
  unsigned grid, rgrid;
  const int rc = po_grid(n, nsample, c, total, grid);
  if (rc <= 0) return rc;
  if (!idx || !grad_output || !grad_input1 || (grad_input2 && p2pb_deterministic())) return P2PB_EINVAL;
  (void)po_grid(n, c, 1, rows, rgrid);
  hipLaunchKernelGGL(po_subtraction_rowsum_kernel, dim3(rgrid), dim3(PO_THREADS), 0, (hipStream_t)stream, rows, c, nsample,
                     grad_output, grad_input1);
  if (grad_input2)
    hipLaunchKernelGGL(po_subtraction_scatter_kernel, dim3(grid), dim3(PO_THREADS), 0, (hipStream_t)stream, total, c,
                       grad_output, idx, grad_input2);
  return p2pb_launch_status();
}

// thread (row, ch): output[row, ch] = fma chain over s of (input[idx_s, ch] + position[row, s, ch]) * weight[row, s, ch mod w_c]
__global__ __launch_bounds__(PO_THREADS) void po_aggregation_forward_kernel(long total, int c, int ns, int w_c,
                                                                            const float *__restrict__ input,
                                                                            const float *__restrict__ position,
                                                                            const float *__restrict__ weight,
                                                                            const int *__restrict__ idx,
                                                                            float *__restrict__ output) {
  PO_ELEMENT(e, total);
  const long row = e / c;
  const int ch = (int)(e - row * c);
  const int *id = idx + row * ns;
  const float *p = position + row * ns * c + ch;
  const float *w = weight + row * ns * w_c + ch % w_c;
  float acc = output[e];
  for (int s = 0; s < ns; ++s)
    acc = __fmaf_rn(input[(size_t)id[s] * c + ch] + p[(size_t)s * c], w[(size_t)s * w_c], acc);
  output[e] = acc;
}
// thread (row, s, ch): grad_position = g w (written), the same added to grad_input at idx (when there is one)
__global__ __launch_bounds__(PO_THREADS) void po_aggregation_grad_kernel(long total, int c, int ns, int w_c,
                                                                         const float *__restrict__ weight,
                                                                         const int *__restrict__ idx,
                                                                         const float *__restrict__ grad_output,
                                                                         float *grad_input, float *__restrict__ grad_position) {
  PO_ELEMENT(e, total);
  const long rs = e / c;
  const int ch = (int)(e - rs * c);
  const float gw = grad_output[(rs / ns) * c + ch] * weight[rs * w_c + ch % w_c];
  grad_position[e] = gw;
  if (grad_input) atomicAdd(grad_input + (size_t)idx[rs] * c + ch, gw);
}
// thread (row, s, j): grad_weight[row, s, j] += g (input + position) over ch = j, j + w_c, ... ascending
__global__ __launch_bounds__(PO_THREADS) void po_aggregation_wgrad_kernel(long total, int c, int ns, int w_c,
                                                                          const float *__restrict__ input,
                                                                          const float *__restrict__ position,
                                                                          const int *__restrict__ idx,
                                                                          const float *__restrict__ grad_output,
                                                                          float *__restrict__ grad_weight) {
  PO_ELEMENT(e, total);
  const long rs = e / w_c;
  const int j = (int)(e - rs * w_c);
  const float *g = grad_output + (rs / ns) * c;
  const float *in = input + (size_t)idx[rs] * c;
  const float *p = position + rs * c;
  float acc = grad_weight[e];
  for (int ch = j; ch < c; ch += w_c) acc += g[ch] * (in[ch] + p[ch]);
  grad_weight[e] = acc;
}

extern "C" int p2pb_pointops_aggregation_forward(int n, int nsample, int c, int w_c, const float *input,
                                                 const float *position, const float *weight, const int *idx, float *output,
                                                 void *stream) {
  long total;
  unsigned grid;
  if (nsample < 0 || w_c < 0) return P2PB_EINVAL;
  const int rc = po_grid(n, c, 1, total, grid);
  if (rc <= 0 || nsample == 0) return rc < 0 ? rc : 0;
  if (w_c == 0 || c % w_c || !input || !position || !weight || !idx || !output) return P2PB_EINVAL;
  hipLaunchKernelGGL(po_aggregation_forward_kernel, dim3(grid), dim3(PO_THREADS), 0, (hipStream_t)stream, total, c, nsample,
                     w_c, input, position, weight, idx, output);
  return p2pb_launch_status();
}

extern "C" int p2pb_pointops_aggregation_backward(int n, int nsample, int c, int w_c, const float *input,
                                                  const float *position, const float *weight, const int *idx,
                                                  const float *grad_output, float *grad_input, float *grad_position,
                                                  float *grad_weight, void *stream) {
  long total, wtotal;
  unsigned grid, wgrid;
  if (w_c < 0) return P2PB_EINVAL;
  const int rc = po_grid(n, nsample, c, total, grid);
  if (rc <= 0) return rc;
  if (w_c == 0 || c % w_c || !input || !position || !weight || !idx || !grad_output || !grad_position || !grad_weight ||
      (grad_input && p2pb_deterministic()))
    return P2PB_EINVAL;
  hipLaunchKernelGGL(po_aggregation_grad_kernel, dim3(grid), dim3(PO_THREADS), 0, (hipStream_t)stream, total, c, nsample, w_c,
                     weight, idx, grad_output, grad_input, grad_position);
  (void)po_grid(n, nsample, w_c, wtotal, wgrid);
  hipLaunchKernelGGL(po_aggregation_wgrad_kernel, dim3(wgrid), dim3(PO_THREADS), 0, (hipStream_t)stream, wtotal, c, nsample,
                     w_c, input, position, idx, grad_output, grad_weight);
  return p2pb_launch_status();
}
