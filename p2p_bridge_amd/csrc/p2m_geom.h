// p2m_geom.h -- the point <-> triangle pair function of the P2M metric, stated ONCE for p2m.hip (every pair),
// p2m_grid.hip (the pairs a grid search cannot rule out) and p2m_packed.hip (packed batches, segments, gradients). It restates
// pytorch3d/csrc/utils/geometry_utils.cuh
// (PointTriangle3DistanceForward, IsInsideTriangle, BarycentricCoords3Forward, PointLine3DistanceForward, kEpsilon = 1e-8):
// see the header of p2m.hip. Plain fp32, no contraction (the library is built with -ffp-contract=off): all files compute
// the same bits for the same (point, triangle).
// segment_foot / triangle_foot hold the arithmetic and the branch decisions; point_segment_d2 / point_triangle_d2 turn them into
// the distance, the gradient functions of p2m_grad.h into its derivative FOR THE BRANCH TAKEN -- one statement of every
// expression and every comparison, so a gradient can never sit on another branch than its forward value.
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

// d = v1 - v0, l2 = |d|^2; l2 <= P2M_EPS: the segment counts as the point v1 (t_raw = t = 0 unused), q = p - v1; else t_raw the
// foot's parameter, t its clamp to [0, 1], q = p - (v0 + t d). The squared distance is |q|^2.
struct SegFoot {
  V3 d, q;
  float l2, t_raw, t;
};
__device__ __forceinline__ SegFoot segment_foot(V3 p, V3 v0, V3 v1) {
  SegFoot s;
  const V3 d = sub3(v1, v0);
  const float l2 = dot3(d, d);
  s.d = d;
  s.l2 = l2;
  if (l2 <= P2M_EPS) {
    const V3 q = sub3(p, v1);
    s.q = q;
    s.t_raw = s.t = 0.0f;
    return s;
  }
  float t = dot3(d, sub3(p, v0)) / l2;
  s.t_raw = t;
  t = fminf(fmaxf(t, 0.0f), 1.0f);
  const V3 q = {p.x - (v0.x + t * d.x), p.y - (v0.y + t * d.y), p.z - (v0.z + t * d.z)};
  s.q = q;
  s.t = t;
  return s;
}

__device__ __forceinline__ float point_segment_d2(V3 p, V3 v0, V3 v1) {
  const SegFoot s = segment_foot(p, v0, v1);
  return dot3(s.q, s.q);
}

// c = (v2 - v0) x (v1 - v0), nn = |c|, n = c / (nn + eps), t = (v0 - p) . n; inside: the area is at least min_area and the
// barycentric weights of p + t n all lie in [0, 1] -- then the squared distance is t^2, else the nearest of the three sides.
struct TriFoot {
  V3 c, n;
  float nn, t;
  bool inside;
};
__device__ __forceinline__ TriFoot triangle_foot(V3 p, V3 v0, V3 v1, V3 v2, float min_area) {
  TriFoot f;
  V3 n = cross3(sub3(v2, v0), sub3(v1, v0));
  f.c = n;
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
  f.n = n;
  f.nn = nn;
  f.t = t;
  f.inside = inside;
  return f;
}

__device__ __forceinline__ float point_triangle_d2(V3 p, V3 v0, V3 v1, V3 v2, float min_area) {
  const TriFoot f = triangle_foot(p, v0, v1, v2, min_area);
  if (f.inside) return f.t * f.t;
  return fminf(fminf(point_segment_d2(p, v0, v1), point_segment_d2(p, v0, v2)), point_segment_d2(p, v1, v2));
}
