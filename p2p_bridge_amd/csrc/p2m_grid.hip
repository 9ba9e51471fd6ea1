// p2m_grid.hip -- the point <-> triangle-mesh distances of p2m.hip for room-sized inputs: the same (dist, idx), bit for bit
// and ties included, from an exact search over a uniform grid instead of every pair. Python side: metrics.TriangleGrid.
// Contract: include/p2pb_hip.h, "point-to-mesh grid"; the argument for every bound below: DESIGN.md, "Point-to-mesh grid".
//
// Exactness rests on three things. (1) The pair function is p2m_geom.h's, the one p2m.hip runs: a pair that is evaluated
// gives the brute force's bits. (2) A pair is skipped only when a LOWER BOUND on that function -- as written in fp32, not on
// the geometric distance -- exceeds the running best: classify gives every prunable triangle a box B and a factor c with
//     point_triangle_d2(p, tri) >= c^2 * dist(p, B)^2 * (1 - 1e-5)   for every p with |p|_inf <= mag,
// where B holds the vertices, the corners of the ENLARGED triangle inside which the function returns the plane distance
// (the +1e-8 of the barycentric denominator scales the weights by denom / (denom + 1e-8)), and an absolute pad for the
// fp32 closest point; c < 1 because the unit normal is n / (|n| + 1e-8). Triangles without such a finite box are tested
// against everything. (3) The minimum is lexicographic in (distance, index) and the stopping test is STRICT, so the lowest
// index among equal distances wins whatever the visiting order and however often a triangle is met.
// The grid is cell_grid.h's sorted cell keys, the one scan.hip searches: the points' keys come from p2pb_scan_cell_keys.
#include "common.h"

#include "cell_grid.h"
#include "p2m_geom.h"

#define PG_MAX_RING 8
#define PG_PAD_SCALE 1.9073486e-6f  // 2^-19: pad = mag * 2^-19 >= 16 ulp of any coordinate within mag

__device__ __forceinline__ V3 load3(const float *__restrict__ p) { return {p[0], p[1], p[2]}; }

// (distance, index) lexicographic minimum: the brute force's "first minimum in index order" for any visiting order
__device__ __forceinline__ void pg_take(float &best, int &bi, float d, int i) {
  if (d < best || (d == best && i < bi)) {
    best = d;
    bi = i;
  }
}

// every unvisited box / point lies at least this far away after ring rho around cells of magnitude <= cmax: the grid's ring
// bound, less the pad, times the factor c
__device__ __forceinline__ float pg_reach(int rho, float cmax, float cell, float pad, float shrink) {
  return (cell_ring_bound(rho, cmax, cell) - pad) * shrink;
}

// strict: an unvisited candidate AT the bound may tie with the best and carry a lower index. reach > 1e-15 keeps its
// square a normal number (the relative margins mean nothing among denormals).
__device__ __forceinline__ bool pg_final(float best, float reach) {
  return reach > 1e-15f && best < reach * reach * 0.99999f;
}

// ---- per-triangle class and box ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pg_classify_kernel(int nt, const float *__restrict__ tris, float min_area, float mag,
                                                          float *__restrict__ box, float *__restrict__ shrink,
                                                          unsigned char *__restrict__ cls) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nt) return;
  const float *q = tris + (size_t)t * 9;
  const V3 v0 = load3(q), v1 = load3(q + 3), v2 = load3(q + 6);
  bool ok = true;
#pragma unroll
  for (int e = 0; e < 9; ++e) ok = ok && fabsf(q[e]) <= mag;  // (NaN and inf fail)
  const float pad = mag * PG_PAD_SCALE;
  float lo[3] = {fminf(v0.x, fminf(v1.x, v2.x)), fminf(v0.y, fminf(v1.y, v2.y)), fminf(v0.z, fminf(v1.z, v2.z))};
  float hi[3] = {fmaxf(v0.x, fmaxf(v1.x, v2.x)), fmaxf(v0.y, fmaxf(v1.y, v2.y)), fmaxf(v0.z, fmaxf(v1.z, v2.z))};
  float c = 1.0f;
  // the expressions of point_triangle_d2, in its order
  const V3 n = cross3(sub3(v2, v0), sub3(v1, v0));
  const float nn = sqrtf(dot3(n, n));
  if (!(0.5f * nn < min_area) && ok) {  // inside test enabled (or undecidable: then not prunable)
    const V3 e0 = sub3(v1, v0), e1 = sub3(v2, v0);
    const float d00 = dot3(e0, e0), d01 = dot3(e0, e1), d11 = dot3(e1, e1);
    const float prod = d00 * d11, graw = prod - d01 * d01;
    // well conditioned: the fp32 Gram determinant is within 1e-3 of the exact one; |n| >= 1e-7 keeps c >= 0.9
    ok = 0.5f * nn >= min_area && nn >= 1e-7f && graw > 0.0f && graw >= 1e-3f * prod;
    if (ok) {
      const float k = (graw + P2M_EPS) / graw;  // the enlargement about v0
      const float cond = prod / graw, smin = sqrtf(fminf(d00, d11)), smax = sqrtf(fmaxf(d00, d11));
      // relative widening of the inside region by the roundings of the weights: of the dot products with p0 - v0 at the
      // region's rim (first term) and of p0 - v0 itself, normal included (second term); DESIGN.md derives both
      const float delta = 3.8146973e-6f * k * (smax / smin) * cond + 8.0f * pad * cond * sqrtf(cond) / smin;
      const float kp = k * (1.0f + delta) * 1.001f + 1e-3f;
      ok = delta <= 1.0f && kp <= 1e6f;
      if (ok) {
        const float ea[3] = {e0.x, e0.y, e0.z}, eb[3] = {e1.x, e1.y, e1.z}, o[3] = {v0.x, v0.y, v0.z};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const float pa = o[a] + kp * ea[a], pb = o[a] + kp * eb[a];
          lo[a] = fminf(lo[a], fminf(pa, pb));
          hi[a] = fmaxf(hi[a], fmaxf(pa, pb));
        }
        c = nn / (nn + P2M_EPS) * 0.999f;
      }
    }
  }
  const float ext = fmaxf(hi[0] - lo[0], fmaxf(hi[1] - lo[1], hi[2] - lo[2]));
  const float grow = pad + 1e-5f * ext;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] -= grow;
    hi[a] += grow;
    ok = ok && fabsf(lo[a]) < INFINITY && fabsf(hi[a]) < INFINITY;
    box[(size_t)t * 6 + a] = lo[a];
    box[(size_t)t * 6 + 3 + a] = hi[a];
  }
  shrink[t] = ok ? c : 1.0f;
  cls[t] = ok ? 0 : 1;
}

// the cells a prunable box overlaps; false: outside the key range
__device__ __forceinline__ bool pg_box_cells(const float *__restrict__ b, float cell, int (&lo)[3], int (&hi)[3]) {
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    bool o0, o1;
    lo[a] = cell_of(b[a], cell, &o0);
    hi[a] = cell_of(b[3 + a], cell, &o1);
    ok = ok && o0 && o1 && lo[a] <= hi[a];
  }
  return ok;
}

__global__ __launch_bounds__(256) void pg_count_kernel(int nt, const unsigned char *__restrict__ cls,
                                                       const float *__restrict__ box, float cell, int cap,
                                                       int *__restrict__ counts, unsigned char *__restrict__ wide) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nt) return;
  int n = 0;
  if (cls[t] == 0) {
    int lo[3], hi[3];
    if (pg_box_cells(box + (size_t)t * 6, cell, lo, hi)) {
      const long long m = (long long)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1);  // (< 2^63)
      if (m <= cap) n = (int)m;
    }
  }
  counts[t] = n;
  wide[t] = n == 0 ? 1 : 0;
}

__global__ __launch_bounds__(256) void pg_fill_kernel(int nt, const int *__restrict__ counts,
                                                      const long long *__restrict__ offsets, const float *__restrict__ box,
                                                      float cell, long long total, long long *__restrict__ keys,
                                                      int *__restrict__ ids) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nt) return;
  const int n = counts[t];
  if (n <= 0) return;
  int lo[3], hi[3];
  if (!pg_box_cells(box + (size_t)t * 6, cell, lo, hi)) return;  // (counts[t] > 0 says it did not)
  long long w = offsets[t];
  const long long end = w + n;
  for (int x = lo[0]; x <= hi[0]; ++x)
    for (int y = lo[1]; y <= hi[1]; ++y)
      for (int z = lo[2]; z <= hi[2]; ++z) {
        if (w < 0 || w >= end || w >= total) return;  // never leaves the triangle's own slots, whatever counts says
        keys[w] = cell_key(x, y, z);
        ids[w] = t;
        ++w;
      }
}

// ---- the ring walk -------------------------------------------------------------------------------------------------------
// Ring rho around the cell box [lo, hi] (a point: lo == hi) is the box grown by rho cells on every side. visit(s, e) is
// called for each run [s, e) of the sorted keys[0..n) that ring rho ADDS to the cube of ring rho - 1, which has been searched:
// a whole column on the rim, of an inner column only the two end cells. Cells beyond the key range hold nothing.
template <class Visit>
__device__ __forceinline__ void pg_ring_runs(const long long *__restrict__ keys, int n, const int (&lo)[3], const int (&hi)[3],
                                             int rho, Visit visit) {
  const int z0 = max(lo[2] - rho, -CELL_KEY_HALF), z1 = min(hi[2] + rho, CELL_KEY_HALF - 1);
  for (int x = max(lo[0] - rho, -CELL_KEY_HALF); x <= min(hi[0] + rho, CELL_KEY_HALF - 1); ++x)
    for (int y = max(lo[1] - rho, -CELL_KEY_HALF); y <= min(hi[1] + rho, CELL_KEY_HALF - 1); ++y) {
      const bool inner = rho > 1 && x > lo[0] - rho && x < hi[0] + rho && y > lo[1] - rho && y < hi[1] + rho;
      for (int part = 0; part < (inner ? 2 : 1); ++part) {
        const int za = inner ? (part ? hi[2] + rho : lo[2] - rho) : z0, zb = inner ? za : z1;
        if (za < -CELL_KEY_HALF || zb >= CELL_KEY_HALF) continue;
        int s, e;
        cell_column(keys, n, x, y, za, zb, s, e);
        visit(s, e);
      }
    }
}

// ---- point -> face -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pg_point_face_kernel(int np, int nt, int ninc, int nwide, int max_ring,
                                                            const float *__restrict__ pts, const float *__restrict__ tris,
                                                            float min_area, const long long *__restrict__ keys,
                                                            const int *__restrict__ ids, const int *__restrict__ wide_ids,
                                                            float cell, float mag, float shrink, float *__restrict__ dist,
                                                            int *__restrict__ idx, unsigned char *__restrict__ unresolved) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= np) return;
  const V3 p = load3(pts + (size_t)i * 3);
  bool okx, oky, okz;
  const int c[3] = {cell_of(p.x, cell, &okx), cell_of(p.y, cell, &oky), cell_of(p.z, cell, &okz)};
  if (!(okx && oky && okz && fabsf(p.x) <= mag && fabsf(p.y) <= mag && fabsf(p.z) <= mag)) {
    unresolved[i] = 1;  // not finite, beyond the coordinates the bounds hold for: brute-force semantics by the fallback
    return;
  }
  float best = 3.4e38f;
  int bi = 0;
  const auto test = [&](int t) {  // (an id outside the mesh is never read through)
    if (t < 0 || t >= nt) return;
    const float *q = tris + (size_t)t * 9;
    pg_take(best, bi, point_triangle_d2(p, load3(q), load3(q + 3), load3(q + 6), min_area), t);
  };
  for (int w = 0; w < nwide; ++w) test(wide_ids[w]);
  bool done = ninc == 0;  // every triangle was wide: all of them have been tested
  const float cmax = (float)max(max(abs(c[0]), abs(c[1])), abs(c[2])), pad = mag * PG_PAD_SCALE;
  for (int rho = 1; rho <= max_ring && !done; ++rho) {
    pg_ring_runs(keys, ninc, c, c, rho, [&](int s, int e) {  // (the point's cell as a box of one cell)
      for (int j = s; j < e; ++j) test(ids[j]);
    });
    done = pg_final(best, pg_reach(rho, cmax, cell, pad, shrink));
  }
  unresolved[i] = done ? 0 : 1;
  if (done) {
    dist[i] = best;
    idx[i] = bi;
  }
}

// ---- face -> point -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pg_face_point_kernel(int ns, int nt, int nextra, int max_ring, int max_cols,
                                                            const float *__restrict__ spts, const int *__restrict__ order,
                                                            const long long *__restrict__ keys,
                                                            const float *__restrict__ extra,
                                                            const int *__restrict__ extra_idx,
                                                            const float *__restrict__ tris, float min_area,
                                                            const unsigned char *__restrict__ cls,
                                                            const float *__restrict__ box, float cell, float mag,
                                                            float shrink, float *__restrict__ dist, int *__restrict__ idx,
                                                            unsigned char *__restrict__ unresolved) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nt) return;
  int lo[3], hi[3];
  if (cls[t] != 0 || !pg_box_cells(box + (size_t)t * 6, cell, lo, hi)) {
    unresolved[t] = 1;
    return;
  }
  const float *q = tris + (size_t)t * 9;
  const V3 v0 = load3(q), v1 = load3(q + 3), v2 = load3(q + 6);
  float best = 3.4e38f;
  int bi = 0;
  for (int j = 0; j < nextra; ++j) pg_take(best, bi, point_triangle_d2(load3(extra + (size_t)j * 3), v0, v1, v2, min_area), extra_idx[j]);
  bool done = ns == 0;
  float cmax = 0.0f;
#pragma unroll
  for (int a = 0; a < 3; ++a) cmax = fmaxf(cmax, (float)max(abs(lo[a]), abs(hi[a])));
  const float pad = mag * PG_PAD_SCALE;
  for (int rho = 1; rho <= max_ring && !done; ++rho) {
    const long long cols = (long long)(hi[0] - lo[0] + 1 + 2 * rho) * (hi[1] - lo[1] + 1 + 2 * rho);
    if (cols > max_cols) break;  // a broad box: the fallback walks the cloud
    pg_ring_runs(keys, ns, lo, hi, rho, [&](int s, int e) {
      for (int j = s; j < e; ++j) pg_take(best, bi, point_triangle_d2(load3(spts + (size_t)j * 3), v0, v1, v2, min_area), order[j]);
    });
    done = pg_final(best, pg_reach(rho, cmax, cell, pad, shrink));
  }
  unresolved[t] = done ? 0 : 1;
  if (done) {
    dist[t] = best;
    idx[t] = bi;
  }
}

// ---- fallback: listed queries against the whole other side -----------------------------------------------------------------
// one wave per query: every lane takes the candidates lane, lane + 64, ... in ascending order (first minimum of its own),
// then the lanes' (distance, index) pairs are reduced lexicographically: the brute force's first minimum
__device__ __forceinline__ void pg_wave_min(float &best, int &bi) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ob = __shfl_xor(best, off);
    const int oi = __shfl_xor(bi, off);
    pg_take(best, bi, ob, oi);
  }
}

// FACE_QUERY: the listed queries are triangles and the candidates the points; otherwise the other way round
template <bool FACE_QUERY>
__global__ __launch_bounds__(256) void pg_subset_kernel(int nq, const int *__restrict__ qidx, int np, int nt,
                                                        const float *__restrict__ pts, const float *__restrict__ tris,
                                                        float min_area, float *__restrict__ dist, int *__restrict__ idx) {
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= nq) return;
  const int q = qidx[w];
  if (q < 0 || q >= (FACE_QUERY ? nt : np)) return;
  V3 p, v0, v1, v2;  // the query's own side is read once, the other per candidate
  const auto point = [&](int i) { p = load3(pts + (size_t)i * 3); };
  const auto face = [&](int t) { const float *f = tris + (size_t)t * 9; v0 = load3(f), v1 = load3(f + 3), v2 = load3(f + 6); };
  if (FACE_QUERY) face(q); else point(q);
  float best = 3.4e38f;
  int bi = 0;
  for (int c = lane_id(); c < (FACE_QUERY ? np : nt); c += 64) {
    if (FACE_QUERY) point(c); else face(c);
    const float d = point_triangle_d2(p, v0, v1, v2, min_area);
    if (d < best) {
      best = d;
      bi = c;
    }
  }
  pg_wave_min(best, bi);
  if (lane_id() == 0) {
    dist[q] = best;
    idx[q] = bi;
  }
}

// ---- entry points --------------------------------------------------------------------------------------------------------
static inline bool pg_pos(float v) { return v > 0.0f && v < INFINITY; }

extern "C" int p2pb_p2m_grid_classify(int nt, const float *tris, float min_triangle_area, float mag, float *box,
                                      float *shrink, unsigned char *cls, void *stream) {
  if (nt <= 0 || !tris || !box || !shrink || !cls || !pg_pos(mag)) return P2PB_EINVAL;
  hipLaunchKernelGGL(pg_classify_kernel, dim3(cdiv(nt, 256)), dim3(256), 0, (hipStream_t)stream, nt, tris,
                     min_triangle_area, mag, box, shrink, cls);
  return p2pb_launch_status();
}

extern "C" int p2pb_p2m_grid_count(int nt, const unsigned char *cls, const float *box, float cell, int cap, int *counts,
                                   unsigned char *wide, void *stream) {
  if (nt <= 0 || cap < 1 || !cls || !box || !counts || !wide || !pg_pos(cell)) return P2PB_EINVAL;
  hipLaunchKernelGGL(pg_count_kernel, dim3(cdiv(nt, 256)), dim3(256), 0, (hipStream_t)stream, nt, cls, box, cell, cap, counts,
                     wide);
  return p2pb_launch_status();
}

extern "C" int p2pb_p2m_grid_fill(int nt, const int *counts, const long long *offsets, const float *box, float cell,
                                  long long total, long long *keys, int *ids, void *stream) {
  if (nt <= 0 || total <= 0 || total >= (1LL << 31) || !counts || !offsets || !box || !keys || !ids || !pg_pos(cell))
    return P2PB_EINVAL;
  hipLaunchKernelGGL(pg_fill_kernel, dim3(cdiv(nt, 256)), dim3(256), 0, (hipStream_t)stream, nt, counts, offsets, box, cell,
                     total, keys, ids);
  return p2pb_launch_status();
}

extern "C" int p2pb_p2m_grid_point_face(int np, int nt, int ninc, int nwide, int max_ring, const float *points,
                                        const float *tris, float min_triangle_area, const long long *keys, const int *ids,
                                        const int *wide_ids, float cell, float mag, float shrink, float *dist, int *idx,
                                        unsigned char *unresolved, void *stream) {
  if (np <= 0 || nt <= 0 || ninc < 0 || nwide < 0 || max_ring < 1 || max_ring > PG_MAX_RING || !points || !tris || !dist ||
      !idx || !unresolved || (ninc > 0 && (!keys || !ids)) || (nwide > 0 && !wide_ids) || !pg_pos(cell) || !pg_pos(mag) ||
      !(shrink > 0.0f && shrink <= 1.0f))
    return P2PB_EINVAL;
  hipLaunchKernelGGL(pg_point_face_kernel, dim3(cdiv(np, 256)), dim3(256), 0, (hipStream_t)stream, np, nt, ninc, nwide,
                     max_ring, points, tris, min_triangle_area, keys, ids, wide_ids, cell, mag, shrink, dist, idx, unresolved);
  return p2pb_launch_status();
}

extern "C" int p2pb_p2m_grid_face_point(int ns, int nt, int nextra, int max_ring, int max_cols, const float *sorted_points,
                                        const int *order, const long long *sorted_keys, const float *extra,
                                        const int *extra_idx, const float *tris, float min_triangle_area,
                                        const unsigned char *cls, const float *box, float cell, float mag, float shrink,
                                        float *dist, int *idx, unsigned char *unresolved, void *stream) {
  if (ns < 0 || nt <= 0 || nextra < 0 || max_ring < 1 || max_ring > PG_MAX_RING || max_cols < 1 ||
      (ns > 0 && (!sorted_points || !order || !sorted_keys)) || (nextra > 0 && (!extra || !extra_idx)) || !tris || !cls ||
      !box || !dist || !idx || !unresolved || !pg_pos(cell) || !pg_pos(mag) || !(shrink > 0.0f && shrink <= 1.0f))
    return P2PB_EINVAL;
  hipLaunchKernelGGL(pg_face_point_kernel, dim3(cdiv(nt, 256)), dim3(256), 0, (hipStream_t)stream, ns, nt, nextra, max_ring,
                     max_cols, sorted_points, order, sorted_keys, extra, extra_idx, tris, min_triangle_area, cls, box, cell, mag,
                     shrink, dist, idx, unresolved);
  return p2pb_launch_status();
}

extern "C" int p2pb_p2m_point_face_subset(int nq, const int *qidx, int np, int nt, const float *points, const float *tris,
                                          float min_triangle_area, float *dist, int *idx, void *stream) {
  if (nq <= 0 || np <= 0 || nt <= 0 || !qidx || !points || !tris || !dist || !idx) return P2PB_EINVAL;
  hipLaunchKernelGGL(pg_subset_kernel<false>, dim3(cdiv(nq, 4)), dim3(256), 0, (hipStream_t)stream, nq, qidx, np, nt,
                     points, tris, min_triangle_area, dist, idx);
  return p2pb_launch_status();
}

extern "C" int p2pb_p2m_face_point_subset(int nq, const int *qidx, int np, int nt, const float *points, const float *tris,
                                          float min_triangle_area, float *dist, int *idx, void *stream) {
  if (nq <= 0 || np <= 0 || nt <= 0 || !qidx || !points || !tris || !dist || !idx) return P2PB_EINVAL;
  hipLaunchKernelGGL(pg_subset_kernel<true>, dim3(cdiv(nq, 4)), dim3(256), 0, (hipStream_t)stream, nq, qidx, np, nt,
                     points, tris, min_triangle_area, dist, idx);
  return p2pb_launch_status();
}
