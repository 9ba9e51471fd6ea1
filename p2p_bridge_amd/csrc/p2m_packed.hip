// p2m_packed.hip -- point <-> mesh distances as a LOSS: packed batches, faces and edges, forward and backward.
//
// Replaces the eight pytorch3d._C operators of metrics/p2m.py ({point_face, face_point, point_edge, edge_point}_dist_{forward,
// backward}); contract: include/p2pb_hip.h, "point-to-mesh, packed batches with gradients". p2m.hip keeps the one-pair,
// no-gradient form the evaluation metrics call.
//   A QUERY is a point or a primitive, a TARGET the other side; a primitive is a triangle (9 floats) or a segment (6).
//   forward : grid (ceil(max_queries / 256), n examples); one thread per query of example blockIdx.y, that example's targets
//             streamed through LDS in tiles of 256 (scalar stores, broadcast reads), running (min, first packed index) -- the
//             loop of point_face_kernel / face_point_kernel (p2m.hip) with a first index on both sides.
//   backward: one thread per query recomputes its pair (p2m_grad.h: the forward's own branch decisions) and stores its own row;
//             the target rows are fp32 atomic adds into a zeroed tensor, or in deterministic mode one wave per target over the
//             caller's target -> queries lists, a fixed order and one store per row.
// Bound: VALU (~60 FLOP per pair) forward; the backward is one gather and a few hundred FLOP per query.
#include "common.h"

#include "p2m_grad.h"  // p2m_geom.h (V3, the pair functions) and their gradients

#define P2M_TILE 256

__device__ __forceinline__ V3 load3(const float *q) { return {q[0], q[1], q[2]}; }
__device__ __forceinline__ void store3(float *q, V3 v) {
  q[0] = v.x;
  q[1] = v.y;
  q[2] = v.z;
}
__device__ __forceinline__ void atomic_add3(float *q, V3 v) {
  atomicAdd(q, v.x);
  atomicAdd(q + 1, v.y);
  atomicAdd(q + 2, v.z);
}

// a primitive of PV vertices and the pair function that goes with it
template <int PV>
struct Prim {
  V3 v[PV];
};
template <int PV>
__device__ __forceinline__ Prim<PV> load_prim(const float *q) {
  Prim<PV> r;
#pragma unroll
  for (int k = 0; k < PV; ++k) r.v[k] = load3(q + 3 * k);
  return r;
}
__device__ __forceinline__ float pair_d2(V3 p, const Prim<3> &t, float min_area) {
  return point_triangle_d2(p, t.v[0], t.v[1], t.v[2], min_area);
}
__device__ __forceinline__ float pair_d2(V3 p, const Prim<2> &s, float) { return point_segment_d2(p, s.v[0], s.v[1]); }

// gradient rows of one pair: the point's and the primitive's PV vertices'
template <int PV>
struct PairGrad {
  V3 p, v[PV];
};
__device__ __forceinline__ PairGrad<3> pair_grad(V3 p, const Prim<3> &t, float min_area, float g) {
  const TriGrad r = point_triangle_grad(p, t.v[0], t.v[1], t.v[2], min_area, g);
  return {r.p, {r.v0, r.v1, r.v2}};
}
__device__ __forceinline__ PairGrad<2> pair_grad(V3 p, const Prim<2> &s, float, float g) {
  const SegGrad r = point_segment_grad(p, s.v[0], s.v[1], g);
  return {r.p, {r.v0, r.v1}};
}

// [first[b], first[b+1]) of example b, the last one up to `total`, clamped into [0, total] (a bad index is never followed)
__device__ __forceinline__ void example_range(const long long *first, int b, int n, int total, int &lo, int &hi) {
  long long a = first[b], e = b + 1 < n ? first[b + 1] : (long long)total;
  a = a < 0 ? 0 : (a > total ? total : a);
  e = e < a ? a : (e > total ? total : e);
  lo = (int)a;
  hi = (int)e;
}

// QP: the queries are the points (targets: primitives of PV vertices); else the queries are the primitives (targets: points)
template <bool QP, int PV>
__global__ __launch_bounds__(256) void p2m_packed_forward_kernel(int n, int np, int ns, const float *__restrict__ pts,
                                                                 const long long *__restrict__ pts_first,
                                                                 const float *__restrict__ prims,
                                                                 const long long *__restrict__ prims_first, float min_area,
                                                                 float *__restrict__ dist, long long *__restrict__ idx) {
  constexpr int TW = QP ? 3 * PV : 3;  // floats per target
  __shared__ float tile[P2M_TILE * TW];
  const int b = blockIdx.y;
  int p_lo, p_hi, s_lo, s_hi;
  example_range(pts_first, b, n, np, p_lo, p_hi);
  example_range(prims_first, b, n, ns, s_lo, s_hi);
  const int q_lo = QP ? p_lo : s_lo, q_hi = QP ? p_hi : s_hi, t_lo = QP ? s_lo : p_lo, t_hi = QP ? s_hi : p_hi;
  const long long i0 = (long long)q_lo + (long long)blockIdx.x * 256;
  if (i0 >= q_hi) return;  // the whole workgroup is past its example's end: out before any barrier
  const bool ok = i0 + threadIdx.x < q_hi;
  const int i = ok ? (int)(i0 + threadIdx.x) : q_lo;  // (an idle lane computes on the example's first query)
  V3 p = {0.0f, 0.0f, 0.0f};
  Prim<PV> me;
  if constexpr (QP)
    p = load3(pts + (size_t)i * 3);
  else
    me = load_prim<PV>(prims + (size_t)i * 3 * PV);
  const float *__restrict__ tsrc = QP ? prims : pts;
  float best = 3.4e38f;
  long long bi = t_lo < t_hi ? t_lo : -1;  // (as p2m.hip: the example's first target unless one is nearer than 3.4e38)
  for (int t0 = t_lo; t0 < t_hi; t0 += P2M_TILE) {
    const int cnt = min(P2M_TILE, t_hi - t0);
    __syncthreads();
    for (int e = threadIdx.x; e < cnt * TW; e += 256) tile[e] = tsrc[(size_t)t0 * TW + e];
    __syncthreads();
    for (int k = 0; k < cnt; ++k) {
      float d;
      if constexpr (QP)
        d = pair_d2(p, load_prim<PV>(tile + TW * k), min_area);
      else
        d = pair_d2(load3(tile + 3 * k), me, min_area);
      if (d < best) {  // first minimum in packed index order
        best = d;
        bi = t0 + k;
      }
    }
  }
  if (ok) {
    dist[i] = best;
    idx[i] = bi;
  }
}

// one thread per query: its own gradient row stored, the target's rows added (ATOMIC) or left to the target kernel
template <bool QP, int PV, bool ATOMIC>
__global__ __launch_bounds__(256) void p2m_packed_backward_query_kernel(int np, int ns, const float *__restrict__ pts,
                                                                        const float *__restrict__ prims,
                                                                        const long long *__restrict__ idx,
                                                                        const float *__restrict__ grad_dist, float min_area,
                                                                        float *__restrict__ grad_pts,
                                                                        float *__restrict__ grad_prims) {
  const int nq = QP ? np : ns, nt = QP ? ns : np;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  const long long t = idx[q];
  const bool chosen = t >= 0 && t < nt;
  PairGrad<PV> r;
  r.p = P2M_V3_ZERO;
#pragma unroll
  for (int k = 0; k < PV; ++k) r.v[k] = P2M_V3_ZERO;
  const int ip = QP ? q : (int)t, is = QP ? (int)t : q;
  if (chosen) r = pair_grad(load3(pts + (size_t)ip * 3), load_prim<PV>(prims + (size_t)is * 3 * PV), min_area, grad_dist[q]);
  if constexpr (QP) {
    store3(grad_pts + (size_t)q * 3, r.p);
    if (ATOMIC && chosen) {
#pragma unroll
      for (int k = 0; k < PV; ++k) atomic_add3(grad_prims + ((size_t)is * PV + k) * 3, r.v[k]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < PV; ++k) store3(grad_prims + ((size_t)q * PV + k) * 3, r.v[k]);
    if (ATOMIC && chosen) atomic_add3(grad_pts + (size_t)ip * 3, r.p);
  }
}

// sum over the wave in a fixed tree (lanes L, L ^ 32, then ^ 16 ... ^ 1): every lane ends with the same total
__device__ __forceinline__ float wave_sum_tree(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// deterministic target rows: one wave per target walks order[start[t] .. start[t+1]) in ascending position, lanes strided
template <bool QP, int PV>
__global__ __launch_bounds__(256) void p2m_packed_backward_target_kernel(int np, int ns, const float *__restrict__ pts,
                                                                         const float *__restrict__ prims,
                                                                         const float *__restrict__ grad_dist, float min_area,
                                                                         const long long *__restrict__ order,
                                                                         const long long *__restrict__ start,
                                                                         float *__restrict__ grad_pts,
                                                                         float *__restrict__ grad_prims) {
  constexpr int TW = QP ? 3 * PV : 3;  // floats per target row
  const int nq = QP ? np : ns, nt = QP ? ns : np;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);  // wave-uniform
  if (t >= nt) return;
  long long lo = start[t], hi = start[t + 1];
  lo = lo < 0 ? 0 : (lo > nq ? nq : lo);
  hi = hi < lo ? lo : (hi > nq ? nq : hi);
  float acc[TW];
#pragma unroll
  for (int e = 0; e < TW; ++e) acc[e] = 0.0f;
  for (long long j = lo + lane_id(); j < hi; j += 64) {
    const long long q = order[j];
    if (q < 0 || q >= nq) continue;
    const int ip = QP ? (int)q : t, is = QP ? t : (int)q;
    const PairGrad<PV> r =
        pair_grad(load3(pts + (size_t)ip * 3), load_prim<PV>(prims + (size_t)is * 3 * PV), min_area, grad_dist[q]);
    if constexpr (QP) {
#pragma unroll
      for (int k = 0; k < PV; ++k) {
        acc[3 * k] += r.v[k].x;
        acc[3 * k + 1] += r.v[k].y;
        acc[3 * k + 2] += r.v[k].z;
      }
    } else {
      acc[0] += r.p.x;
      acc[1] += r.p.y;
      acc[2] += r.p.z;
    }
  }
#pragma unroll
  for (int e = 0; e < TW; ++e) acc[e] = wave_sum_tree(acc[e]);
  float *__restrict__ row = (QP ? grad_prims : grad_pts) + (size_t)t * TW;
  if (lane_id() == 0) {
#pragma unroll
    for (int e = 0; e < TW; ++e) row[e] = acc[e];
  }
}

// kind -> f(queries are points, vertices per primitive)
template <class F>
static inline int for_p2m_kind(int kind, F &&f) {
  switch (kind) {
    case P2PB_P2M_POINT_FACE: return f(std::true_type{}, std::integral_constant<int, 3>{});
    case P2PB_P2M_FACE_POINT: return f(std::false_type{}, std::integral_constant<int, 3>{});
    case P2PB_P2M_POINT_EDGE: return f(std::true_type{}, std::integral_constant<int, 2>{});
    case P2PB_P2M_EDGE_POINT: return f(std::false_type{}, std::integral_constant<int, 2>{});
  }
  return P2PB_EINVAL;
}

extern "C" int p2pb_p2m_packed_forward(int kind, int n, int np, int ns, int max_queries, const float *points,
                                       const long long *points_first_idx, const float *prims,
                                       const long long *prims_first_idx, float min_triangle_area, float *dist, long long *idx,
                                       void *stream) {
  if (n <= 0 || n > 65535 || np <= 0 || ns <= 0 || max_queries <= 0) return P2PB_EINVAL;
  if (!points || !points_first_idx || !prims || !prims_first_idx || !dist || !idx) return P2PB_EINVAL;
  return for_p2m_kind(kind, [&](auto qp, auto pv) {
    hipLaunchKernelGGL((p2m_packed_forward_kernel<decltype(qp)::value, decltype(pv)::value>), dim3(cdiv(max_queries, 256), n),
                       dim3(256), 0, (hipStream_t)stream, n, np, ns, points, points_first_idx, prims, prims_first_idx,
                       min_triangle_area, dist, idx);
    return p2pb_launch_status();
  });
}

extern "C" int p2pb_p2m_packed_backward(int kind, int np, int ns, const float *points, const float *prims, const long long *idx,
                                        const float *grad_dist, float min_triangle_area, const long long *order,
                                        const long long *start, float *grad_points, float *grad_prims, void *stream) {
  if (np <= 0 || ns <= 0) return P2PB_EINVAL;
  if (!points || !prims || !idx || !grad_dist || !grad_points || !grad_prims) return P2PB_EINVAL;
  const bool det = p2pb_deterministic();
  if (det && (!order || !start)) return P2PB_EINVAL;
  return for_p2m_kind(kind, [&](auto qp, auto pv) {
    constexpr bool QP = decltype(qp)::value;
    constexpr int PV = decltype(pv)::value;
    const int nq = QP ? np : ns, nt = QP ? ns : np;
    if (!det) {
      hipLaunchKernelGGL((p2m_packed_backward_query_kernel<QP, PV, true>), dim3(cdiv(nq, 256)), dim3(256), 0, (hipStream_t)stream,
                         np, ns, points, prims, idx, grad_dist, min_triangle_area, grad_points, grad_prims);
      return p2pb_launch_status();
    }
    hipLaunchKernelGGL((p2m_packed_backward_query_kernel<QP, PV, false>), dim3(cdiv(nq, 256)), dim3(256), 0, (hipStream_t)stream,
                       np, ns, points, prims, idx, grad_dist, min_triangle_area, grad_points, grad_prims);
    hipLaunchKernelGGL((p2m_packed_backward_target_kernel<QP, PV>), dim3(cdiv(nt, 4)), dim3(256), 0, (hipStream_t)stream, np, ns,
                       points, prims, grad_dist, min_triangle_area, order, start, grad_points, grad_prims);
    return p2pb_launch_status();
  });
}
