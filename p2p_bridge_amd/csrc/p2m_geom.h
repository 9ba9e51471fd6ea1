// p2m_geom.h -- the point <-> triangle pair function of the P2M metric, stated ONCE for p2m.hip (every pair) and
// p2m_grid.hip (the pairs a grid search cannot rule out). It restates pytorch3d/csrc/utils/geometry_utils.cuh
// (PointTriangle3DistanceForward, IsInsideTriangle, BarycentricCoords3Forward, PointLine3DistanceForward, kEpsilon = 1e-8):
// see the header of p2m.hip. Plain fp32, no contraction (the library is built with -ffp-contract=off): both files compute
// the same bits for the same (point, triangle).
#pragma once

#define P2M_EPS 1e-8f

struct V3 {
  float x, y, z;
};
__device__ __forceinline__ V3 sub3(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float dot3(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross3(V3 a, V3 b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

__device__ __forceinline__ float point_segment_d2(V3 p, V3 v0, V3 v1) {
  const V3 d = sub3(v1, v0);
  const float l2 = dot3(d, d);
  if (l2 <= P2M_EPS) {
    const V3 q = sub3(p, v1);
    return dot3(q, q);
  }
  float t = dot3(d, sub3(p, v0)) / l2;
  t = fminf(fmaxf(t, 0.0f), 1.0f);
  const V3 q = {p.x - (v0.x + t * d.x), p.y - (v0.y + t * d.y), p.z - (v0.z + t * d.z)};
  return dot3(q, q);
}

__device__ __forceinline__ float point_triangle_d2(V3 p, V3 v0, V3 v1, V3 v2, float min_area) {
  V3 n = cross3(sub3(v2, v0), sub3(v1, v0));
  const float nn = sqrtf(dot3(n, n));
  const float inv = 1.0f / (nn + P2M_EPS);
  n = {n.x * inv, n.y * inv, n.z * inv};
  const float t = dot3(sub3(v0, p), n);
  const V3 p0 = {p.x + t * n.x, p.y + t * n.y, p.z + t * n.z};
  bool inside = false;
  if (0.5f * nn >= min_area) {  // AreaOfTriangle = |cross| / 2
    const V3 e0 = sub3(v1, v0), e1 = sub3(v2, v0), e2 = sub3(p0, v0);
    const float d00 = dot3(e0, e0), d01 = dot3(e0, e1), d11 = dot3(e1, e1), d20 = dot3(e2, e0), d21 = dot3(e2, e1);
    const float denom = d00 * d11 - d01 * d01 + P2M_EPS;
    const float w1 = (d11 * d20 - d01 * d21) / denom, w2 = (d00 * d21 - d01 * d20) / denom;
    const float w0 = 1.0f - w1 - w2;
    inside = (0.0f <= w0 && w0 <= 1.0f) && (0.0f <= w1 && w1 <= 1.0f) && (0.0f <= w2 && w2 <= 1.0f);
  }
  if (inside) return t * t;
  return fminf(fminf(point_segment_d2(p, v0, v1), point_segment_d2(p, v0, v2)), point_segment_d2(p, v1, v2));
}
