// voxel_common.h -- what the three stages of the point <-> voxel kernels share (voxel_coords.hip: coordinates and the
// per-voxel sorted point lists; voxel_gather.hip: the feature gathers; devoxelize.hip: trilinear devoxelize).
// All of these are HBM-bound: the dominant traffic is the dense [C, r^3] grid (written once by voxelize including its
// zeros, read once by devoxelize); the N x (3+C) point tensor is read with lane-consecutive (coalesced) accesses, the
// grid is written lane-consecutive over the voxel index.
#pragma once
#include "common.h"

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
// a store through a pointer of this address space is a ds_write; a volatile store through a generic pointer is a flat_store
#define P2PB_LDS __attribute__((address_space(3)))

// The workspace of p2pb_voxel_sort, int[b*r^3 + 3*b*n + b]:
//   cur   [b][r^3] exclusive prefix of cnt; after the fill it points at each voxel's segment END
//   list  [b][n]   point ids grouped by voxel, order inside a voxel arbitrary
//   slist [b][n]   the same segments, ids ascending
//   occ   [b][n]   compacted list of the non-empty voxels (nocc[b] entries)
//   nocc  [b]
struct VoxWs {
  int *cur, *list, *slist, *occ, *nocc;
};

// carves `ws` (may be null: size only) into *w and returns the size in bytes -- the one statement of the layout
static inline size_t vox_ws_carve(const void *ws, int b, int n, int r3, VoxWs *w) {
  const size_t nv = (size_t)b * r3, np = (size_t)b * n;
  if (ws) {
    w->cur = (int *)ws;
    w->list = w->cur + nv;
    w->slist = w->list + np;
    w->occ = w->slist + np;
    w->nocc = w->occ + np;
  }
  return sizeof(int) * (nv + 3 * np + (size_t)b);
}
