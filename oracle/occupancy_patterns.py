"""Synthetic voxel occupancies for the sparse voxel convolutions, and the sets the kernels derive from an occupancy, computed
plainly with torch on the CPU (never the product).

A cloud that went through voxel_coords(normalize=True) lies inside the sphere inscribed in the grid: no occupied voxel on a grid
edge or corner, no full brick, whatever per-brick counts the sphere happens to give. patterns(r) gives occupancies that reach
those regimes on purpose -- tests/test_occupancy_patterns.py states what the set must cover (per-brick counts 0, 1..31, 32,
32k, 32k +- 1, 256; all 27 boundary classes both inside D1 and outside D2) and fails when a changed pattern loses some of it.

Conventions (csrc/conv3d_lists.hip): a grid is indexed [d, h, w] as cnt.view(B, r, r, r) is; bricks are 4 x 8 x 8 voxels in
(bd, bh, bw) order, a voxel's local id is (ld*8 + lh)*8 + lw; the boundary class of a voxel is (cd*3 + ch)*3 + cw with
c = 0 on the low face, 2 on the high face, 1 between."""
from collections import OrderedDict, namedtuple

import torch
import torch.nn.functional as F

RESOLUTIONS = (8, 16, 32)
BERNOULLI = (0.003, 0.05, 0.5)
# generator seed of the Bernoulli patterns per resolution, chosen so that the whole set meets tests/test_occupancy_patterns.py (at
# r = 8 the two bricks of most seeds give no whole number of tiles between 32 and 256 under D1; bern0.05 of this one gives 192)
BERNOULLI_SEED = {8: 65, 16: 3, 32: 0}

Sets = namedtuple("Sets", "d1 d2 counts active cls")


def patterns(r):
    """name -> bool[r, r, r]"""
    r = int(r)
    assert r in RESOLUTIONS
    z = lambda: torch.zeros(r, r, r, dtype=torch.bool)
    out = OrderedDict()
    out["full"] = torch.ones(r, r, r, dtype=torch.bool)
    p = z()
    for d in (0, r - 1):
        for h in (0, r - 1):
            for w in (0, r - 1):
                p[d, h, w] = True
    out["corners"] = p
    p = z()
    m = r // 2
    for axis in range(3):
        for side in (0, r - 1):
            v = [m, m, m]
            v[axis] = side
            p[tuple(v)] = True
    out["faces"] = p
    p = z()
    p[0, 0, m] = p[r - 1, m, 0] = p[m, r - 1, r - 1] = True
    out["edges"] = p
    p = z()
    p[1, 1, 1] = True
    out["single_111"] = p
    gen = torch.Generator().manual_seed(BERNOULLI_SEED[r])  # one generator per r, drawn in this order
    for q in BERNOULLI:
        out[f"bern{q:g}"] = torch.rand(r, r, r, generator=gen) < q
    p = z()
    p[::2, ::2, ::2] = True
    out["checker2"] = p
    if r >= 16:
        p = z()
        p[3, 7, 7] = True  # the last voxel of brick 0: its D1 spills into 8 bricks
        out["brick_corner"] = p
        p = z()
        p[:, :, 7] = True
        out["wall_w7"] = p
        p = z()
        p[:, :, 6] = True
        out["wall_w6"] = p
        p = z()
        p[5:7, 9:12, 9:12] = True
        out["interior_box"] = p
    return out


def dilate(s):
    """bool[B, r, r, r] -> every voxel with a set voxel in its 3x3x3 window (nothing outside the grid is set)"""
    return F.max_pool3d(s[:, None].float(), 3, 1, 1)[:, 0] > 0


def to_bricks(s):
    """[B, r, r, r] -> [B, NBRICK, 256]: bricks in (bd, bh, bw) order, local id (ld*8 + lh)*8 + lw"""
    b, r = s.shape[0], s.shape[1]
    return s.reshape(b, r // 4, 4, r // 8, 8, r // 8, 8).permute(0, 1, 3, 5, 2, 4, 6).reshape(b, -1, 256)


def boundary_classes(r):
    """int64[r, r, r]: (cd*3 + ch)*3 + cw"""
    c = torch.ones(r, dtype=torch.int64)
    c[0], c[r - 1] = 0, 2
    return (c[:, None, None] * 3 + c[None, :, None]) * 3 + c[None, None, :]


def reference_sets(occ_b):
    """occ_b bool[B, r, r, r] -> Sets(
         d1, d2   bool[B, r, r, r]: dilate(occ, 1), dilate(d1, 1),
         counts   int64[2, B, NBRICK]: voxels of d1 / d2 per brick,
         active   bool[2, B, NBRICK]: an occupied voxel within brick +- 1 / brick +- 2 (the bricks the first / second
                  convolution of the list-driven form computes),
         cls      int64[r, r, r]: boundary class of every voxel)"""
    occ_b = occ_b.bool()
    b, r = occ_b.shape[0], occ_b.shape[1]
    d1 = dilate(occ_b)
    d2 = dilate(d1)
    counts = torch.stack([to_bricks(d1).sum(-1), to_bricks(d2).sum(-1)])
    o = occ_b[:, None].float()
    act = [F.max_pool3d(o, (4 + 2 * k, 8 + 2 * k, 8 + 2 * k), (4, 8, 8), k).reshape(b, -1) > 0 for k in (1, 2)]
    return Sets(d1, d2, counts, torch.stack(act), boundary_classes(r))
