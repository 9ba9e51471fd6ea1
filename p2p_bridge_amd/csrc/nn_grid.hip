// nn_grid.hip -- the exact NEAREST point of a whole cloud with its index, for 10^6 .. 10^7 queries: the room-size form of
// chamfer.hip's nm_distance_kernel (every pair of two clouds). The search is knn_grid.hip's -- rings of cells over SORTED CELL
// KEYS (cell_grid.h), keys (distance bits << 32 | original row) -- at k = 1, where a wave and a 64-wide best-list per query
// are the wrong shape: the nearest point is ONE running u64 minimum in ONE lane, so a query is a lane here, not a wave.
//
// Why the result is knn_grid's at k = 1, and nm_distance_kernel's, bit for bit ("Grid nearest point / Chamfer"):
//   * ties. The key of a (point, query) pair is (bits of sqdist3(point - query) << 32) | the point's ORIGINAL row: the keys of
//     one query are all different and ordered by (distance, row), and their minimum does not depend on the order of the
//     visit. It is the brute force's "first strict minimum": the lowest row among the nearest.
//   * finality. Ring rho is final when the best distance <= cell_ring_bound(rho, cmax, cell)^2 * 0.999999, knn_grid_kernel's
//     expression with the best distance in tau's place: every unvisited point is STRICTLY farther, so none can tie.
//   * a minimum is idempotent: ring rho walks the whole cube of (2 rho + 1)^3 cells again and nothing restarts.
// Lanes are independent (no cross-lane traffic, no LDS, no atomics), so WHICH queries share a wave -- the caller's qidx order
// -- cannot change a bit; it decides only whether neighbouring lanes search the same key ranges and read the same lines.
// Every output is one plain vector store by the lane that owns the query. Contract: include/p2pb_hip.h, "grid nearest point".
#include "common.h"

#include "cell_grid.h"

typedef unsigned long long u64;

__device__ __forceinline__ u64 nn_grid_key(float d, int row) { return ((u64)__float_as_uint(d) << 32) | (unsigned)row; }

// One lane per query qidx[w] (qidx NULL: query w). Ring rho = 1..max_ring: for every x of the cube the SLAB (x, y0..y1, z0..z1)
// is one contiguous run of the sorted keys, found by two binary searches over all n keys; the columns of the slab are runs
// inside it, in ascending y, each found by cell_column over what is left of the slab (a handful of keys: the long, dependent
// searches are 2 per x instead of 2 per column). Every loop is bounded by max_ring or by n.
__global__ __launch_bounds__(256) void nn_grid_kernel(int nq, int n, int max_ring, const int *__restrict__ qidx,
                                                      const float *__restrict__ query, const float *__restrict__ pts,
                                                      const long long *__restrict__ keys, const int *__restrict__ rows,
                                                      float cell, float *__restrict__ dist2, int *__restrict__ idx,
                                                      unsigned char *__restrict__ unresolved) {
  const int w = blockIdx.x * 256 + threadIdx.x;
  if (w >= nq) return;
  const int q = qidx ? qidx[w] : w;
  const float qx = query[(size_t)q * 3], qy = query[(size_t)q * 3 + 1], qz = query[(size_t)q * 3 + 2];
  bool okx, oky, okz;
  const int cx = cell_of(qx, cell, &okx), cy = cell_of(qy, cell, &oky), cz = cell_of(qz, cell, &okz);
  bool done = false;
  u64 best = ~0ull;
  if (okx && oky && okz) {
    const float cmax = (float)max(max(abs(cx), abs(cy)), abs(cz));
    for (int rho = 1; rho <= max_ring && !done; ++rho) {
      const int x0 = max(cx - rho, -CELL_KEY_HALF), x1 = min(cx + rho, CELL_KEY_HALF - 1);
      const int y0 = max(cy - rho, -CELL_KEY_HALF), y1 = min(cy + rho, CELL_KEY_HALF - 1);
      const int z0 = max(cz - rho, -CELL_KEY_HALF), z1 = min(cz + rho, CELL_KEY_HALF - 1);
      for (int x = x0; x <= x1; ++x) {
        int s = cell_lower_bound(keys, 0, n, cell_key(x, y0, z0));
        const int slab_end = cell_lower_bound(keys, s, n, cell_key(x, y1, z1) + 1);
        for (int y = y0; y <= y1 && s < slab_end; ++y) {
          int a, e;  // the column's run, relative to s
          cell_column(keys + s, slab_end - s, x, y, z0, z1, a, e);
          for (int j = s + a; j < s + e; ++j) {
            const u64 c = nn_grid_key(sqdist3(pts[(size_t)j * 3] - qx, pts[(size_t)j * 3 + 1] - qy, pts[(size_t)j * 3 + 2] - qz),
                                      rows[j]);
            best = c < best ? c : best;
          }
          s += e;  // (the next column's keys are all larger)
        }
      }
      const float reach = cell_ring_bound(rho, cmax, cell);
      // (nothing seen yet: the distance bits of ~0 are a NaN, and the ring is not final)
      done = reach > 0.0f && best != ~0ull && __uint_as_float((unsigned)(best >> 32)) <= reach * reach * 0.999999f;
    }
  }
  unresolved[q] = done ? 0 : 1;
  if (done) {
    dist2[q] = __uint_as_float((unsigned)(best >> 32));
    idx[q] = (int)(unsigned)best;
  }
}

// ---- entry point -------------------------------------------------------------------------------------------------------
extern "C" int p2pb_nn_grid(int nq, int n, int max_ring, const int *qidx, const float *query, const float *sorted_points,
                            const long long *sorted_keys, const int *rows, float cell, float *dist2, int *idx,
                            unsigned char *unresolved, void *stream) {
  if (nq <= 0 || n <= 0 || max_ring < 1 || max_ring > 16 || !query || !sorted_points || !sorted_keys || !rows || !dist2 ||
      !idx || !unresolved || !(cell > 0.0f) || !(cell < INFINITY))
    return P2PB_EINVAL;
  hipLaunchKernelGGL(nn_grid_kernel, dim3(cdiv(nq, 256)), dim3(256), 0, (hipStream_t)stream, nq, n, max_ring, qidx, query,
                     sorted_points, sorted_keys, rows, cell, dist2, idx, unresolved);
  return p2pb_launch_status();
}
