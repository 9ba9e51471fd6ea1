// imgfeat.hip -- image features onto a scan (the reference's data/processing/image_features.py): which points a frame sees,
// the fp16 running mean of the frames' feature rows per point, and one round of the in-place median fill of the unobserved
// points. Python side: p2p_bridge_amd/image_features.py. Everything here is deterministic: integer atomics only where the
// result does not depend on their order, no float atomics.
#include "common.h"

#include <limits.h>

namespace {

// ---- visibility -------------------------------------------------------------------------------------------------------
// The reference walks the points of a frame in ascending index with a depth buffer and keeps point i iff its depth is
// STRICTLY below the smallest depth an EARLIER point left in its pixel (image_features.py:176-188): the valid points are
// the records of the running minimum of each pixel's list in index order. Stated per point,
//     valid(i) = inside(i) and depth(i) < min { depth(j) : j < i, inside(j), pixel(j) == pixel(i) }
// is a function of the SET of (index, depth) pairs of the pixel, so the order in which the lists are filled cannot reach
// the result. Passes: project + count (integer atomics), exclusive scan per frame, fill, resolve (one wave per pixel).

// workspace: depth f64[b*n] | pix i32[b*n] | list i32[b*n] | cnt i32[b*P] | cur i32[b*P]
struct VisWs {
  double *depth;
  int *pix, *list, *cnt, *cur;
};
static inline VisWs vis_ws(void *ws, size_t bn, size_t bp) {
  VisWs w;
  w.depth = (double *)ws;
  w.pix = (int *)(w.depth + bn);
  w.list = w.pix + bn;
  w.cnt = w.list + bn;
  w.cur = w.cnt + bp;
  return w;
}

// fp64 in a fixed order, no contraction: (m0*x + m1*y) + m2*z
__device__ __forceinline__ double row3(const double *__restrict__ m, double x, double y, double z) {
  return (m[0] * x + m[1] * y) + m[2] * z;
}

__global__ __launch_bounds__(256) void vis_project_kernel(int n, int width, int height, double min_depth, double max_depth,
                                                          const double *__restrict__ points, const double *__restrict__ rot,
                                                          const double *__restrict__ trans, const double *__restrict__ cam,
                                                          unsigned char *__restrict__ valid, int *__restrict__ xy,
                                                          double *__restrict__ depth, int *__restrict__ pix,
                                                          int *__restrict__ cnt) {
  const int f = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double *r = rot + (size_t)f * 9, *t = trans + (size_t)f * 3, *k = cam + (size_t)f * 9;
  const double px = points[(size_t)i * 3], py = points[(size_t)i * 3 + 1], pz = points[(size_t)i * 3 + 2];
  const double cx = row3(r, px, py, pz) + t[0], cy = row3(r + 3, px, py, pz) + t[1], cz = row3(r + 6, px, py, pz) + t[2];
  const double u = row3(k, cx, cy, cz), v = row3(k + 3, cx, cy, cz), w = row3(k + 6, cx, cy, cz);
  const double x = u / w, y = v / w;  // IEEE divides
  // the bounds are decided in floating point BEFORE any conversion: trunc(x) is in [0, width) exactly when -1 < x < width; a
  // NaN, an infinity or a coordinate beyond the int range fails a comparison and never becomes a pixel
  const bool inside = x > -1.0 && x < (double)width && y > -1.0 && y < (double)height && w > min_depth && w < max_depth;
  const size_t o = (size_t)f * n + i;
  int xi = -1, yi = -1, p = -1;
  if (inside) {
    xi = (int)x;  // truncation toward zero: x in (-1, 0) is column 0, like the reference's int(x)
    yi = (int)y;
    p = yi * width + xi;
    atomicAdd(cnt + (size_t)f * width * height + p, 1);
  }
  xy[o * 2] = xi;
  xy[o * 2 + 1] = yi;
  pix[o] = p;
  depth[o] = w;
  valid[o] = 0;  // (the resolve pass sets the records)
}

// exclusive scan of one frame's pixel counts by one 1024-thread workgroup: cur[p] = first list slot of pixel p
__global__ __launch_bounds__(1024) void vis_scan_kernel(int npix, const int *__restrict__ cnt, int *__restrict__ cur) {
  __shared__ int wsum[16];
  const int t = threadIdx.x;
  const int *c = cnt + (size_t)blockIdx.x * npix;
  int *o = cur + (size_t)blockIdx.x * npix;
  const int per = (npix + 1023) / 1024;
  const int beg = min(t * per, npix), end = min(beg + per, npix);
  int s = 0;
  for (int p = beg; p < end; ++p) s += c[p];
  int inc = s;
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(inc, d);
    if ((t & 63) >= d) inc += y;
  }
  if ((t & 63) == 63) wsum[t >> 6] = inc;
  __syncthreads();
  int run = inc - s;
  for (int w = 0; w < (t >> 6); ++w) run += wsum[w];
  for (int p = beg; p < end; ++p) {
    const int x = c[p];
    o[p] = run;
    run += x;
  }
}

__global__ __launch_bounds__(256) void vis_fill_kernel(int n, int npix, const int *__restrict__ pix, int *__restrict__ cur,
                                                       int *__restrict__ list) {
  const int f = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int p = pix[(size_t)f * n + i];
  if (p < 0) return;
  const int pos = atomicAdd(cur + (size_t)f * npix + p, 1);  // pos < n: the counts of a frame sum to at most n
  list[(size_t)f * n + pos] = i;
}

// one wave per pixel. Up to 64 points: (index, depth) sit in the lanes and pass through lane broadcasts. Longer lists: 64
// points at a time against the whole list through wave-uniform loads, len^2 / 64 steps per wave (a list of 5000: 4e5).
__global__ __launch_bounds__(256) void vis_resolve_kernel(int n, int npix, const int *__restrict__ cnt,
                                                          const int *__restrict__ cur, const int *__restrict__ list,
                                                          const double *__restrict__ depth, unsigned char *__restrict__ valid) {
  const int f = blockIdx.y;
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= npix) return;
  const int cn = cnt[(size_t)f * npix + p];
  if (cn == 0) return;
  const int lane = lane_id();
  const int *seg = list + (size_t)f * n + (cur[(size_t)f * npix + p] - cn);  // cur is the segment's end after the fill
  const double *dep = depth + (size_t)f * n;
  unsigned char *out = valid + (size_t)f * n;
  if (cn <= 64) {
    const int mine = lane < cn ? seg[lane] : INT_MAX;
    const double d = lane < cn ? dep[mine] : 0.0;
    double m = __builtin_huge_val();
    for (int j = 0; j < cn; ++j) {
      const int oi = __shfl(mine, j);
      const double od = __shfl(d, j);
      if (oi < mine) m = fmin(m, od);
    }
    if (lane < cn) out[mine] = d < m;
    return;
  }
  for (int l0 = 0; l0 < cn; l0 += 64) {
    const int l = l0 + lane;
    const int mine = l < cn ? seg[l] : -1;
    const double d = l < cn ? dep[mine] : 0.0;
    double m = __builtin_huge_val();
    for (int j = 0; j < cn; ++j) {
      const int oi = seg[j];  // wave-uniform address
      const double od = dep[oi];
      if (oi < mine) m = fmin(m, od);
    }
    if (l < cn) out[mine] = d < m;
  }
}

// ---- fusion -----------------------------------------------------------------------------------------------------------
// mean += (new - mean) / count per frame in order, every operator one fp32 evaluation rounded to fp16 (torch's fp16 tensor
// arithmetic, image_features.py:269-277): d = f16(f32(new) - f32(mean)), q = f16(f32(d) / f32(count)), mean = f16(f32(mean) +
// f32(q)); the count goes to fp32, never to fp16 (2049 is not an fp16 number).
typedef _Float16 f16v8 __attribute__((ext_vector_type(8)));
template <int VEC>
struct F16Vec;
template <>
struct F16Vec<8> {
  typedef f16v8 T;
};
template <>
struct F16Vec<1> {
  typedef _Float16 T;
};

__device__ __forceinline__ _Float16 mean_step(_Float16 m, _Float16 nw, float fc) {
  const _Float16 d = (_Float16)((float)nw - (float)m);
  const _Float16 q = (_Float16)((float)d / fc);
  return (_Float16)((float)m + (float)q);
}
__device__ __forceinline__ void mean_step_v(f16v8 &m, const f16v8 &nw, float fc) {
#pragma unroll
  for (int e = 0; e < 8; ++e) m[e] = mean_step(m[e], nw[e], fc);
}
__device__ __forceinline__ void mean_step_v(_Float16 &m, const _Float16 &nw, float fc) { m = mean_step(m, nw, fc); }

// A workgroup holds `ppb` whole points, `lanes` consecutive threads per point running along the channels (VEC fp16 per thread
// and step). All threads of a point sit in one workgroup, so the barrier below orders their reads of count[p] before the one
// write. Frames are taken four at a time: the (up to) four gathered rows are requested before the dependent arithmetic starts.
template <int VEC>
__global__ __launch_bounds__(256) void fuse_kernel(int b, int n, int c, int hmap, int wmap, int lanes, int ppb,
                                                   const _Float16 *__restrict__ maps, const unsigned char *__restrict__ valid,
                                                   const int *__restrict__ xy, _Float16 *__restrict__ mean,
                                                   int *__restrict__ count) {
  typedef typename F16Vec<VEC>::T V;
  const int lp = (int)threadIdx.x / lanes, lv = (int)threadIdx.x % lanes;
  const long p = (long)blockIdx.x * ppb + lp;
  const bool act = lp < ppb && p < n;
  const int cnt0 = act ? count[p] : 0;
  __syncthreads();
  if (!act) return;
  const int nvec = c / VEC;
  int cnt = cnt0;
  for (int v = lv; v < nvec; v += lanes) {
    V *mp = (V *)(mean + (size_t)p * c) + v;
    V m = *mp;
    cnt = cnt0;
    for (int f0 = 0; f0 < b; f0 += 4) {
      bool ok[4];
      V row[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int f = f0 + u;
        ok[u] = f < b && valid[(size_t)f * n + p] != 0;
        if (ok[u]) {
          const size_t o = ((size_t)f * n + p) * 2;
          const int x = min(max(xy[o], 0), wmap - 1), y = min(max(xy[o + 1], 0), hmap - 1);
          row[u] = *((const V *)(maps + (((size_t)f * hmap + y) * wmap + x) * c) + v);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (ok[u]) {
          ++cnt;
          mean_step_v(m, row[u], (float)cnt);
        }
    }
    if (cnt != cnt0) *mp = m;  // (a point no frame of this batch saw keeps its row: nothing to write)
  }
  if (lv == 0 && cnt != cnt0) count[p] = cnt;
}

// ---- fusion from the coarse grid --------------------------------------------------------------------------------------
// The DINO branch of the reference upsamples the [h, w] patch grid to the frame's (H, W) with bilinear interpolation
// (image_features.py:110) and then reads one pixel per visible point. The value of that map at one pixel is a function of four
// grid rows, so it is formed here, per point, and the map (37.7 MB per 192 x 256 frame of 384 channels) never exists.
// Contract (include/p2pb_hip.h): per axis src = max((dst + 0.5) * (in / out) - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1, in - 1),
// l1 = src - i0, l0 = 1 - l1; value = ly0 * (lx0*a + lx1*b) + ly1 * (lx0*c + lx1*d), each operator one fp32 operation (the file is
// compiled with -ffp-contract=off), one rounding to fp16.
struct Lin {
  int i0, i1;
  float l0, l1;
};
__device__ __forceinline__ Lin lin_axis(int dst, int in, int out) {
  const float scale = (float)in / (float)out;
  const float src = fmaxf(((float)dst + 0.5f) * scale - 0.5f, 0.0f);
  Lin r;
  r.i0 = min((int)src, in - 1);  // (src >= 0: truncation is floor; src < in - 0.5 for every dst < out, the min guards memory)
  r.i1 = min(r.i0 + 1, in - 1);
  r.l1 = src - (float)r.i0;
  r.l0 = 1.0f - r.l1;
  return r;
}
__device__ __forceinline__ _Float16 bilerp(_Float16 a, _Float16 b, _Float16 c, _Float16 d, const Lin &lx, const Lin &ly) {
  const float top = lx.l0 * (float)a + lx.l1 * (float)b;
  const float bot = lx.l0 * (float)c + lx.l1 * (float)d;
  return (_Float16)(ly.l0 * top + ly.l1 * bot);
}
__device__ __forceinline__ f16v8 bilerp_v(const f16v8 &a, const f16v8 &b, const f16v8 &c, const f16v8 &d, const Lin &lx,
                                          const Lin &ly) {
  f16v8 r;
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = bilerp(a[e], b[e], c[e], d[e], lx, ly);
  return r;
}
__device__ __forceinline__ _Float16 bilerp_v(const _Float16 &a, const _Float16 &b, const _Float16 &c, const _Float16 &d,
                                             const Lin &lx, const Lin &ly) {
  return bilerp(a, b, c, d, lx, ly);
}
// vector v of the sampled row of one frame's grid g f16[h,w,c] at pixel (x, y) of the (out_h, out_w) map, coordinates clamped
template <int VEC>
__device__ __forceinline__ typename F16Vec<VEC>::T grid_row(const _Float16 *__restrict__ g, int h, int w, int c, int out_h,
                                                           int out_w, int x, int y, int v) {
  typedef typename F16Vec<VEC>::T V;
  const Lin lx = lin_axis(min(max(x, 0), out_w - 1), w, out_w), ly = lin_axis(min(max(y, 0), out_h - 1), h, out_h);
  const V *r0 = (const V *)(g + (size_t)ly.i0 * w * c), *r1 = (const V *)(g + (size_t)ly.i1 * w * c);
  const size_t nvec = (size_t)(c / VEC);
  return bilerp_v(r0[lx.i0 * nvec + v], r0[lx.i1 * nvec + v], r1[lx.i0 * nvec + v], r1[lx.i1 * nvec + v], lx, ly);
}

// one thread per (frame, point, vector of channels)
template <int VEC>
__global__ __launch_bounds__(256) void sample_grid_kernel(long total, int n, int c, int h, int w, int out_h, int out_w,
                                                          const _Float16 *__restrict__ grid, const int *__restrict__ xy,
                                                          _Float16 *__restrict__ out) {
  typedef typename F16Vec<VEC>::T V;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int nvec = c / VEC;
  const int v = (int)(e % nvec);
  const long fp = e / nvec;  // frame * n + point
  const long f = fp / n;
  *((V *)(out + (size_t)fp * c) + v) =
      grid_row<VEC>(grid + (size_t)f * h * w * c, h, w, c, out_h, out_w, xy[(size_t)fp * 2], xy[(size_t)fp * 2 + 1], v);
}

// fuse_kernel with the gathered map row replaced by the sampled grid row: same decomposition, same three roundings per frame
template <int VEC>
__global__ __launch_bounds__(256) void fuse_grid_kernel(int b, int n, int c, int h, int w, int out_h, int out_w, int lanes, int ppb,
                                                        const _Float16 *__restrict__ grid, const unsigned char *__restrict__ valid,
                                                        const int *__restrict__ xy, _Float16 *__restrict__ mean,
                                                        int *__restrict__ count) {
  typedef typename F16Vec<VEC>::T V;
  const int lp = (int)threadIdx.x / lanes, lv = (int)threadIdx.x % lanes;
  const long p = (long)blockIdx.x * ppb + lp;
  const bool act = lp < ppb && p < n;
  const int cnt0 = act ? count[p] : 0;
  __syncthreads();
  if (!act) return;
  const int nvec = c / VEC;
  int cnt = cnt0;
  for (int v = lv; v < nvec; v += lanes) {
    V *mp = (V *)(mean + (size_t)p * c) + v;
    V m = *mp;
    cnt = cnt0;
    for (int f0 = 0; f0 < b; f0 += 2) {
      bool ok[2];
      V row[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int f = f0 + u;
        ok[u] = f < b && valid[(size_t)f * n + p] != 0;
        if (ok[u]) {
          const size_t o = ((size_t)f * n + p) * 2;
          row[u] = grid_row<VEC>(grid + (size_t)f * h * w * c, h, w, c, out_h, out_w, xy[o], xy[o + 1], v);
        }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u)
        if (ok[u]) {
          ++cnt;
          mean_step_v(m, row[u], (float)cnt);
        }
    }
    if (cnt != cnt0) *mp = m;
  }
  if (lv == 0 && cnt != cnt0) count[p] = cnt;
}

// ---- fill -------------------------------------------------------------------------------------------------------------
// The reference fills the unobserved points in ascending index, in place (image_features.py:314-324): point i takes the
// per-channel median of the rows of its k nearest points that are not all-zero AT THAT MOMENT -- observed points, and unobserved
// points j < i with their FILLED rows. One round of that as a wavefront: a point is ready when every unobserved neighbour below
// it was finished in an EARLIER round (done_round in [1, round)); a value written during this round reads as "not finished"
// whichever way the race falls, and rows are only read once their writer's launch is over. One wave per unobserved point.
template <int KMAX>
__global__ __launch_bounds__(64) void fill_round_kernel(int n, int c, int k, const int *__restrict__ missing,
                                                        const int *__restrict__ nbr, const int *__restrict__ count,
                                                        _Float16 *__restrict__ feat, int *__restrict__ done_round, int round,
                                                        int *__restrict__ remaining) {
  const int mi = blockIdx.x;
  const int i = missing[mi];
  if (i < 0 || i >= n) return;
  if (__atomic_load_n(done_round + i, __ATOMIC_RELAXED) != 0) return;
  const int lane = lane_id();
  int nb = lane < k ? nbr[(size_t)mi * k + lane] : -1;
  bool use = false, blocked = false;
  if (nb >= 0 && nb < n && nb != i) {
    if (count[nb] > 0) {
      use = true;
    } else if (nb < i) {  // (an unobserved point above i is still zero when the reference reaches i: it never contributes)
      const int dr = __atomic_load_n(done_round + nb, __ATOMIC_RELAXED);
      if (dr != 0 && dr < round)
        use = true;
      else
        blocked = true;
    }
  }
  if (__ballot(blocked) != 0ull) return;  // not ready in this round
  // the rows that contribute and are not all-zero (+0 / -0), in neighbour order: lane t keeps the t-th
  const unsigned long long usemask = __ballot(use);
  int kept = 0, mykept = 0;
  for (int j = 0; j < k; ++j) {
    if (!((usemask >> j) & 1ull)) continue;
    const int r = __shfl(nb, j);
    const unsigned short *row = (const unsigned short *)feat + (size_t)r * c;
    unsigned bits = 0;
    for (int ch = lane; ch < c; ch += 64) bits |= row[ch] & 0x7fffu;
    if (__ballot(bits != 0u) != 0ull) {
      if (lane == kept) mykept = r;
      ++kept;
    }
  }
  int kidx[KMAX];
#pragma unroll
  for (int t = 0; t < KMAX; ++t) kidx[t] = __shfl(mykept, t);
  const int lo_rank = (kept - 1) / 2, hi_rank = kept / 2;
  for (int ch0 = 0; ch0 < c; ch0 += 64) {
    const int ch = ch0 + lane;
    const bool a = ch < c;
    float v[KMAX];
    bool nan = false;
#pragma unroll
    for (int t = 0; t < KMAX; ++t) {
      v[t] = (a && t < kept) ? (float)feat[(size_t)kidx[t] * c + ch] : 0.0f;
      nan |= v[t] != v[t];
    }
    float lo = 0.0f, hi = 0.0f;
#pragma unroll
    for (int s = 0; s < KMAX; ++s) {
      if (s < kept) {
        int rank = 0;
#pragma unroll
        for (int t = 0; t < KMAX; ++t)
          if (t < kept) rank += (v[t] < v[s] || (v[t] == v[s] && t < s)) ? 1 : 0;
        if (rank == lo_rank) lo = v[s];
        if (rank == hi_rank) hi = v[s];
      }
    }
    // median: the mean of the two middle values (the same value twice for an odd count) in fp32, one rounding to fp16;
    // no row left: zeros; a NaN among the values: NaN, like np.median
    float res = kept > 0 ? (lo + hi) * 0.5f : 0.0f;
    if (nan) res = __builtin_nanf("");
    if (a) feat[(size_t)i * c + ch] = (_Float16)res;
  }
  if (lane == 0) {
    __atomic_store_n(done_round + i, round, __ATOMIC_RELAXED);
    atomicSub(remaining, 1);
  }
}

}  // namespace

extern "C" size_t p2pb_imgfeat_visibility_ws_bytes(int b, int n, int width, int height) {
  if (b <= 0 || n <= 0 || width <= 0 || height <= 0) return 0;
  const size_t bn = (size_t)b * n, bp = (size_t)b * width * height;
  return bn * (sizeof(double) + 2 * sizeof(int)) + bp * 2 * sizeof(int);
}

extern "C" int p2pb_imgfeat_visibility(int b, int n, const double *points, const double *rotation, const double *translation,
                                       const double *camera, int width, int height, double min_depth, double max_depth,
                                       unsigned char *valid, int *xy, void *ws, void *stream) {
  if (b <= 0 || n <= 0 || width <= 0 || height <= 0 || b > 65535) return P2PB_EINVAL;
  if (!points || !rotation || !translation || !camera || !valid || !xy || !ws) return P2PB_EINVAL;
  if ((size_t)width * height > (size_t)INT_MAX || (size_t)b * n > (size_t)INT_MAX) return P2PB_EINVAL;
  if (((size_t)ws & 7) != 0) return P2PB_EINVAL;
  const int npix = width * height;
  const size_t bn = (size_t)b * n, bp = (size_t)b * npix;
  hipStream_t s = (hipStream_t)stream;
  const VisWs w = vis_ws(ws, bn, bp);
  int rc = p2pb_zero_async(w.cnt, bp * sizeof(int), s);
  if (rc) return rc;
  hipLaunchKernelGGL(vis_project_kernel, dim3(cdiv(n, 256), b), dim3(256), 0, s, n, width, height, min_depth, max_depth, points,
                     rotation, translation, camera, valid, xy, w.depth, w.pix, w.cnt);
  hipLaunchKernelGGL(vis_scan_kernel, dim3(b), dim3(1024), 0, s, npix, w.cnt, w.cur);
  hipLaunchKernelGGL(vis_fill_kernel, dim3(cdiv(n, 256), b), dim3(256), 0, s, n, npix, w.pix, w.cur, w.list);
  hipLaunchKernelGGL(vis_resolve_kernel, dim3(cdiv(npix, 4), b), dim3(256), 0, s, n, npix, w.cnt, w.cur, w.list, w.depth, valid);
  return p2pb_launch_status();
}

template <int VEC>
static int fuse_launch(int b, int n, int c, int hmap, int wmap, const _Float16 *maps, const unsigned char *valid, const int *xy,
                       _Float16 *mean, int *count, hipStream_t s) {
  const int nvec = c / VEC;
  const int lanes = nvec < 256 ? nvec : 256;
  const int ppb = 256 / lanes;
  hipLaunchKernelGGL(fuse_kernel<VEC>, dim3(cdiv(n, ppb)), dim3(256), 0, s, b, n, c, hmap, wmap, lanes, ppb, maps, valid, xy, mean,
                     count);
  return p2pb_launch_status();
}

extern "C" int p2pb_imgfeat_fuse(int b, int n, int c, int hmap, int wmap, const void *maps, const unsigned char *valid,
                                 const int *xy, void *mean, int *count, void *stream) {
  if (b <= 0 || n <= 0 || c <= 0 || hmap <= 0 || wmap <= 0) return P2PB_EINVAL;
  if (!maps || !valid || !xy || !mean || !count) return P2PB_EINVAL;
  if ((size_t)b * n > (size_t)INT_MAX) return P2PB_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const bool vec = c % 8 == 0 && (((size_t)maps | (size_t)mean) & 15) == 0;  // 16-byte rows at 16-byte addresses
  return vec ? fuse_launch<8>(b, n, c, hmap, wmap, (const _Float16 *)maps, valid, xy, (_Float16 *)mean, count, s)
             : fuse_launch<1>(b, n, c, hmap, wmap, (const _Float16 *)maps, valid, xy, (_Float16 *)mean, count, s);
}

static bool grid_args_ok(int b, int n, int c, int h, int w, int out_h, int out_w) {
  if (b <= 0 || n <= 0 || c <= 0 || h <= 0 || w <= 0 || out_h <= 0 || out_w <= 0) return false;
  return (size_t)b * n <= (size_t)INT_MAX && (size_t)h * w <= (size_t)INT_MAX / 2;
}

extern "C" int p2pb_imgfeat_sample_grid(int b, int n, int c, int h, int w, int out_h, int out_w, const void *grid, const int *xy,
                                        void *out, void *stream) {
  if (!grid_args_ok(b, n, c, h, w, out_h, out_w) || !grid || !xy || !out) return P2PB_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const bool vec = c % 8 == 0 && (((size_t)grid | (size_t)out) & 15) == 0;
  const long total = (long)b * n * (vec ? c / 8 : c);
  if (total / 256 >= (long)INT_MAX) return P2PB_EINVAL;
  if (vec)
    hipLaunchKernelGGL(sample_grid_kernel<8>, dim3(cdiv(total, 256)), dim3(256), 0, s, total, n, c, h, w, out_h, out_w,
                       (const _Float16 *)grid, xy, (_Float16 *)out);
  else
    hipLaunchKernelGGL(sample_grid_kernel<1>, dim3(cdiv(total, 256)), dim3(256), 0, s, total, n, c, h, w, out_h, out_w,
                       (const _Float16 *)grid, xy, (_Float16 *)out);
  return p2pb_launch_status();
}

template <int VEC>
static int fuse_grid_launch(int b, int n, int c, int h, int w, int out_h, int out_w, const _Float16 *grid,
                            const unsigned char *valid, const int *xy, _Float16 *mean, int *count, hipStream_t s) {
  const int nvec = c / VEC;
  const int lanes = nvec < 256 ? nvec : 256;
  const int ppb = 256 / lanes;
  hipLaunchKernelGGL(fuse_grid_kernel<VEC>, dim3(cdiv(n, ppb)), dim3(256), 0, s, b, n, c, h, w, out_h, out_w, lanes, ppb, grid,
                     valid, xy, mean, count);
  return p2pb_launch_status();
}

extern "C" int p2pb_imgfeat_fuse_grid(int b, int n, int c, int h, int w, int out_h, int out_w, const void *grid,
                                      const unsigned char *valid, const int *xy, void *mean, int *count, void *stream) {
  if (!grid_args_ok(b, n, c, h, w, out_h, out_w) || !grid || !valid || !xy || !mean || !count) return P2PB_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const bool vec = c % 8 == 0 && (((size_t)grid | (size_t)mean) & 15) == 0;
  return vec ? fuse_grid_launch<8>(b, n, c, h, w, out_h, out_w, (const _Float16 *)grid, valid, xy, (_Float16 *)mean, count, s)
             : fuse_grid_launch<1>(b, n, c, h, w, out_h, out_w, (const _Float16 *)grid, valid, xy, (_Float16 *)mean, count, s);
}

extern "C" int p2pb_imgfeat_fill_round(int m, int n, int c, int k, const int *missing, const int *nbr, const int *count,
                                       void *feat, int *done_round, int round, int *remaining, void *stream) {
  if (m <= 0 || n <= 0 || c <= 0 || k <= 0 || k > 32 || k > n || m > n || round <= 0) return P2PB_EINVAL;
  if (!missing || !nbr || !count || !feat || !done_round || !remaining) return P2PB_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (k <= 16)
    hipLaunchKernelGGL(fill_round_kernel<16>, dim3(m), dim3(64), 0, s, n, c, k, missing, nbr, count, (_Float16 *)feat, done_round,
                       round, remaining);
  else
    hipLaunchKernelGGL(fill_round_kernel<32>, dim3(m), dim3(64), 0, s, n, c, k, missing, nbr, count, (_Float16 *)feat, done_round,
                       round, remaining);
  return p2pb_launch_status();
}
