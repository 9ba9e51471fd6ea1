// p2m_grad.h -- the gradients of the two pair functions of p2m_geom.h, for p2m_packed.hip. Each takes the branch decisions from
// the forward's own segment_foot / triangle_foot (same fp32 values, same comparisons) and returns the exact derivative of the
// forward EXPRESSION of that branch times g = d loss / d dist. Selections are constants: `inside`, the first minimum of the three
// sides in the order (v0v1, v0v2, v1v2), the clamp of t, the l2 <= eps test.
//   segment, l2 <= eps     : f = |p - v1|^2                         -> p and v1 only
//   segment, t clamped     : f = |p - v0|^2 (t = 0) or |p - (v0 + 1 d)|^2 = |p - v1|^2 (t = 1) -> p and that end point only
//   segment, interior      : f = |q|^2, q = p - v0 - t d, t = d.(p - v0) / d.d, through t (q.d is a rounding residual there, not 0)
//   triangle, inside       : f = t^2, t = (v0 - p).n, n = c / (|c| + eps), c = (v2 - v0) x (v1 - v0), through n and c
// Finite inputs give finite gradients: every division is by l2 > eps, |c| + eps or |c| > 0; a zero distance or |c| == 0 gives
// exact zeros (the factor that vanishes multiplies before anything divides, or the term is branched away).
#pragma once

#include "p2m_geom.h"

__device__ __forceinline__ V3 scale3(float s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ V3 add3(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 neg3(V3 a) { return {-a.x, -a.y, -a.z}; }
#define P2M_V3_ZERO (V3{0.0f, 0.0f, 0.0f})

struct SegGrad {
  V3 p, v0, v1;
};
__device__ __forceinline__ SegGrad point_segment_grad(V3 p, V3 v0, V3 v1, float g) {
  const SegFoot s = segment_foot(p, v0, v1);
  const V3 gq = scale3(2.0f * g, s.q);  // d f / d q
  if (s.l2 <= P2M_EPS) return {gq, P2M_V3_ZERO, neg3(gq)};
  if (!(s.t_raw > 0.0f)) return {gq, neg3(gq), P2M_V3_ZERO};  // the clamp's fmaxf sends a NaN to 0 as well
  if (s.t_raw >= 1.0f) return {gq, P2M_V3_ZERO, neg3(gq)};
  // q = p - v0 - t d: dq = dp - (1 - t) dv0 - t dv1 - d dt, so f' = gq.dq with gq.d = a * l2 carried by
  // dt = (d.dp - (w + (1 - 2t) d).dv0 + (w - 2t d).dv1) / l2, w = p - v0
  const float t = s.t;
  const float a = dot3(gq, s.d) / s.l2;
  const V3 w = sub3(p, v0);
  SegGrad r;
  r.p = sub3(gq, scale3(a, s.d));
  r.v0 = add3(scale3(t - 1.0f, gq), scale3(a, add3(w, scale3(1.0f - 2.0f * t, s.d))));
  r.v1 = sub3(scale3(-t, gq), scale3(a, sub3(w, scale3(2.0f * t, s.d))));
  return r;
}

struct TriGrad {
  V3 p, v0, v1, v2;
};
__device__ __forceinline__ TriGrad point_triangle_grad(V3 p, V3 v0, V3 v1, V3 v2, float min_area, float g) {
  const TriFoot f = triangle_foot(p, v0, v1, v2, min_area);
  if (f.inside) {
    const float gt = 2.0f * g * f.t;  // d f / d t
    TriGrad r = {scale3(-gt, f.n), scale3(gt, f.n), P2M_V3_ZERO, P2M_V3_ZERO};
    if (f.nn > 0.0f) {
      // n = c / (nn + eps): dn = (dc - chat (chat.dc) nn / (nn + eps)) / (nn + eps), chat = c / nn, and chat nn / (nn + eps) = n
      const V3 gn = scale3(gt, sub3(v0, p));
      const V3 chat = {f.c.x / f.nn, f.c.y / f.nn, f.c.z / f.nn};
      const V3 gc = scale3(1.0f / (f.nn + P2M_EPS), sub3(gn, scale3(dot3(f.n, gn), chat)));
      // c = a x b, a = v2 - v0, b = v1 - v0: gc.(da x b) = da.(b x gc), gc.(a x db) = db.(gc x a)
      const V3 ga = cross3(sub3(v1, v0), gc), gb = cross3(gc, sub3(v2, v0));
      r.v2 = ga;
      r.v1 = gb;
      r.v0 = sub3(r.v0, add3(ga, gb));
    }
    return r;
  }
  const float d01 = point_segment_d2(p, v0, v1), d02 = point_segment_d2(p, v0, v2), d12 = point_segment_d2(p, v1, v2);
  int side = 0;  // the first minimum, as fminf(fminf(d01, d02), d12) keeps it
  float best = d01;
  if (d02 < best) {
    best = d02;
    side = 1;
  }
  if (d12 < best) side = 2;
  if (side == 0) {
    const SegGrad s = point_segment_grad(p, v0, v1, g);
    return {s.p, s.v0, s.v1, P2M_V3_ZERO};
  }
  if (side == 1) {
    const SegGrad s = point_segment_grad(p, v0, v2, g);
    return {s.p, s.v0, P2M_V3_ZERO, s.v1};
  }
  const SegGrad s = point_segment_grad(p, v1, v2, g);
  return {s.p, P2M_V3_ZERO, s.v0, s.v1};
}
