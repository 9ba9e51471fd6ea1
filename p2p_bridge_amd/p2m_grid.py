"""Exact grid search for the point <-> triangle-mesh distances (csrc/p2m_grid.hip): `TriangleGrid` holds the per-mesh index,
`plan_triangle_grid` chooses its parameters. The results are those of the brute-force kernels of csrc/p2m.hip bit for bit,
ties included ("Point-to-mesh grid"); `metrics.point_face_distance(..., method="grid")` is the public door.

Workspace, the stated constant: at most INCIDENCES_PER_TRIANGLE (8) (cell, triangle) incidences per triangle on average
-- the build doubles the cell edge rather than exceed it -- i.e. about 140 bytes per triangle resident (box 24, factor 4,
class / wide 2, count 4, offset 8, 8 x (key 8 + id 4)) and under 500 during torch's sort of the keys; 24 bytes per point
resident in face -> point (key 8, sorted copy 12, index 4), under 60 during the sort.
"""
import ctypes
import math
from typing import NamedTuple

import torch

from .cell_grid import KEY_HALF, sorted_cells  # (KEY_HALF: the planner's test holds the plan to the key range)
INCIDENCES_PER_TRIANGLE = 8
MAG_MIN, MAG_MAX = 1e-6, 1e6  # coordinates the kernels' fp32 bounds are argued for (no overflow in |cross|^2, no denormals)


class GridPlan(NamedTuple):
    usable: bool  # False: not finite, or mag above MAG_MAX: the index runs the brute force
    mag: float  # every coordinate the grid handles is within +-mag; the kernels' absolute rounding pad is mag * 2^-19
    cell: float  # cell edge
    max_ring: int  # rings searched before a query goes to the fallback
    cap: int  # a triangle whose box overlaps more cells is tested against everything ("broad")
    max_cols: int  # face -> point: a ring of more columns than this sends the triangle to the fallback
    max_incidences: int  # the build enlarges the cell until the incidences fit


def plan_triangle_grid(lo, hi, n_tris, median_extent):
    """lo, hi: the mesh's bounding box (3 floats each), n_tris its triangle count, median_extent the median over the prunable
    triangles of the longest edge of their conservative box. A pure function of these numbers.
    cell = max(2 * median_extent, longest box edge / 2048, mag / 2^18): a typical box then overlaps 1-2 cells per axis (about
    3.4 cells), a point within one cell edge of the surface is final after ring 1, the grid is never finer than the key range
    allows (|coordinate / cell| <= 2^18 << 2^20) nor absurdly finer than the mesh."""
    lo, hi = [float(v) for v in lo], [float(v) for v in hi]
    n_tris, median_extent = int(n_tris), float(median_extent)
    finite = all(math.isfinite(v) for v in lo + hi) and math.isfinite(median_extent)
    reach = max([abs(v) for v in lo + hi]) if finite else math.inf
    mag = max(4.0 * reach, MAG_MIN)
    usable = finite and mag <= MAG_MAX and n_tris > 0
    if not usable:
        mag = MAG_MAX if not (mag <= MAG_MAX) else mag
    extent = max(h - l for l, h in zip(lo, hi)) if finite else 0.0
    cell = max(2.0 * max(median_extent, 0.0) if finite else 0.0, extent / 2048.0, mag / (1 << 18))
    return GridPlan(usable, mag, cell, 4, 64, 128, INCIDENCES_PER_TRIANGLE * max(n_tris, 0) + 1024)


def workspace_bound_bytes(n_points, n_tris):
    """the resident bytes the index and one face -> point query may hold (module docstring); monotone in both counts"""
    plan_inc = INCIDENCES_PER_TRIANGLE * int(n_tris) + 1024
    return 42 * int(n_tris) + 12 * plan_inc + 24 * int(n_points)


def _f32(v):
    return ctypes.c_float(float(v)).value


class TriangleGrid:
    """The grid index of one mesh: tris f32[T,3,3] on the GPU. Built once, queried for any number of clouds.

        g = TriangleGrid(tris, min_triangle_area)
        dist, idx = g.point_face(points)                  # == metrics.point_face_distance(points, tris, min_triangle_area)
        dist, idx, stats = g.face_point(points, return_stats=True)

    stats: {"fallback": queries that the rings left to the brute-force fallback, "queries": their total, "broad": triangles
    whose box overlaps more than the cap of cells, "unbounded": triangles without a finite box, "incidences", "cell"}."""

    def __init__(self, tris, min_triangle_area=5e-3):
        from ._lib import call, check, ptr, stream_ptr

        tris = tris.contiguous()
        check(tris, torch.float32, "tris")
        if tris.dim() != 3 or tris.shape[1:] != (3, 3) or tris.shape[0] == 0:
            raise ValueError("tris must be f32[T,3,3] with T >= 1")
        self.tris, self.min_triangle_area = tris, float(min_triangle_area)
        T, dev = tris.shape[0], tris.device
        self.n_tris = T
        flat = tris.reshape(-1, 3)
        fin = torch.isfinite(flat).all(dim=1)
        if bool(fin.any()):
            good = flat[fin]
            lo, hi = good.min(dim=0).values.tolist(), good.max(dim=0).values.tolist()
        else:
            lo, hi = [0.0] * 3, [0.0] * 3
        plan = plan_triangle_grid(lo, hi, T, 0.0)
        self.box = torch.empty(T, 6, dtype=torch.float32, device=dev)
        self.shrink_t = torch.empty(T, dtype=torch.float32, device=dev)
        self.cls = torch.empty(T, dtype=torch.uint8, device=dev)
        self.keys = self.ids = self.wide_ids = None
        self.n_inc = self.n_wide = self.n_broad = 0
        self.n_unbounded = T
        self.shrink = 1.0
        self.plan = plan
        if not plan.usable:
            return
        call("p2pb_p2m_grid_classify", int(T), ptr(tris), float(min_triangle_area), float(plan.mag), ptr(self.box),
             ptr(self.shrink_t), ptr(self.cls), stream_ptr())
        prunable = self.cls == 0
        self.n_unbounded = T - int(prunable.sum())
        med = 0.0
        if self.n_unbounded < T:
            ext = (self.box[:, 3:] - self.box[:, :3]).max(dim=1).values[prunable]
            med = float(ext.median())
            self.shrink = float(self.shrink_t.min())
        plan = plan_triangle_grid(lo, hi, T, med)
        counts = torch.empty(T, dtype=torch.int32, device=dev)
        wide = torch.empty(T, dtype=torch.uint8, device=dev)
        cell = plan.cell
        for _ in range(24):  # enlarge the cell rather than exceed the workspace bound
            call("p2pb_p2m_grid_count", int(T), ptr(self.cls), ptr(self.box), float(cell), int(plan.cap), ptr(counts), ptr(wide),
                 stream_ptr())
            total = int(counts.sum(dtype=torch.int64))
            if total <= plan.max_incidences:
                break
            cell *= 2.0
        else:
            raise RuntimeError("TriangleGrid: the incidences do not fit the workspace bound at any cell edge")
        self.plan = plan._replace(cell=_f32(cell), mag=_f32(plan.mag))  # the fp32 values the kernels see
        self.n_inc = total
        self.wide_ids = wide.nonzero().flatten().to(torch.int32)
        self.n_wide = int(self.wide_ids.numel())
        self.n_broad = self.n_wide - self.n_unbounded
        if total > 0:
            offsets = torch.cumsum(counts, 0, dtype=torch.int64) - counts
            keys = torch.empty(total, dtype=torch.int64, device=dev)
            ids = torch.empty(total, dtype=torch.int32, device=dev)
            call("p2pb_p2m_grid_fill", int(T), ptr(counts), ptr(offsets), ptr(self.box), float(self.plan.cell),
                 total, ptr(keys), ptr(ids), stream_ptr())
            self.keys, perm = torch.sort(keys)
            self.ids = ids[perm].contiguous()

    # ---- queries -----------------------------------------------------------------------------------------------------
    def _stats(self, fallback, queries):
        return {"fallback": int(fallback), "queries": int(queries), "broad": self.n_broad, "unbounded": self.n_unbounded,
                "incidences": self.n_inc, "cell": self.plan.cell}

    def _points(self, points):
        from ._lib import check

        points = points.contiguous()
        check(points, torch.float32, "points")
        if points.dim() != 2 or points.shape[1] != 3 or points.shape[0] == 0:
            raise ValueError("points must be f32[P,3] with P >= 1")
        if points.device != self.tris.device:
            raise ValueError("points and the mesh index live on different devices")
        return points

    def _brute(self, fn, points, n_out):
        from ._lib import call, ptr, stream_ptr

        d = torch.empty(n_out, dtype=torch.float32, device=points.device)
        idx = torch.empty(n_out, dtype=torch.int32, device=points.device)
        call(fn, int(points.shape[0]), int(self.n_tris), ptr(points), ptr(self.tris), float(self.min_triangle_area), ptr(d),
             ptr(idx), stream_ptr())
        return d, idx

    def _finish(self, which, points, d, idx, unresolved, return_stats):
        """the fallback: the queries the rings left, against the whole other side; most of them -> the brute-force kernel"""
        from ._lib import call, ptr, stream_ptr

        n = d.shape[0]
        left = unresolved.nonzero().flatten().to(torch.int32)
        nleft = int(left.numel())
        if 2 * nleft > n:
            d, idx = self._brute("p2pb_point_face_dist" if which == 0 else "p2pb_face_point_dist", points, n)
        elif nleft:
            call("p2pb_p2m_point_face_subset" if which == 0 else "p2pb_p2m_face_point_subset", int(nleft), ptr(left),
                 int(points.shape[0]), int(self.n_tris), ptr(points), ptr(self.tris), float(self.min_triangle_area), ptr(d),
                 ptr(idx), stream_ptr())
        out = (d, idx.long())
        return out + (self._stats(nleft, n),) if return_stats else out

    def point_face(self, points, return_stats=False):
        """-> (squared distance of every point to its closest triangle [P], its index i64[P]) [, stats]"""
        from ._lib import call, ptr, stream_ptr

        points = self._points(points)
        P, dev = points.shape[0], points.device
        if not self.plan.usable:
            d, idx = self._brute("p2pb_point_face_dist", points, P)
            return (d, idx.long(), self._stats(P, P)) if return_stats else (d, idx.long())
        d = torch.empty(P, dtype=torch.float32, device=dev)
        idx = torch.empty(P, dtype=torch.int32, device=dev)
        unresolved = torch.empty(P, dtype=torch.uint8, device=dev)
        pl = self.plan
        call("p2pb_p2m_grid_point_face", int(P), int(self.n_tris), int(self.n_inc), int(self.n_wide), int(pl.max_ring), ptr(points),
             ptr(self.tris), float(self.min_triangle_area), ptr(self.keys), ptr(self.ids),
             ptr(self.wide_ids if self.n_wide else None), float(pl.cell), float(pl.mag), float(self.shrink), ptr(d), ptr(idx),
             ptr(unresolved), stream_ptr())
        return self._finish(0, points, d, idx, unresolved, return_stats)

    def face_point(self, points, return_stats=False):
        """-> (squared distance of every triangle to its closest point [T], that point's index i64[T]) [, stats]"""
        from ._lib import call, ptr, stream_ptr

        points = self._points(points)
        T, dev = self.n_tris, points.device
        if not self.plan.usable:
            d, idx = self._brute("p2pb_face_point_dist", points, T)
            return (d, idx.long(), self._stats(T, T)) if return_stats else (d, idx.long())
        pl = self.plan
        inside = (points.abs() <= pl.mag).all(dim=1)  # (NaN fails) |p / cell| <= 2^18: inside the key range
        sel = inside.nonzero().flatten()
        out_idx = (~inside).nonzero().flatten().to(torch.int32)
        ns, nextra = int(sel.numel()), int(out_idx.numel())
        if 2 * nextra > points.shape[0]:  # most of the cloud is outside the grid: every triangle would walk it anyway
            d, idx = self._brute("p2pb_face_point_dist", points, T)
            return (d, idx.long(), self._stats(T, T)) if return_stats else (d, idx.long())
        spts = order = skeys = extra = None
        if ns:
            spts, skeys, order = sorted_cells(points[sel].contiguous(), float(pl.cell), RuntimeError(
                "TriangleGrid: a point within the coordinate bound fell outside the key range"), ids=sel.to(torch.int32))
        if nextra:
            extra = points[out_idx.long()].contiguous()
        d = torch.empty(T, dtype=torch.float32, device=dev)
        idx = torch.empty(T, dtype=torch.int32, device=dev)
        unresolved = torch.empty(T, dtype=torch.uint8, device=dev)
        call("p2pb_p2m_grid_face_point", int(ns), int(T), int(nextra), int(pl.max_ring), int(pl.max_cols), ptr(spts), ptr(order),
             ptr(skeys), ptr(extra), ptr(out_idx if nextra else None), ptr(self.tris), float(self.min_triangle_area),
             ptr(self.cls), ptr(self.box), float(pl.cell), float(pl.mag), float(self.shrink), ptr(d), ptr(idx), ptr(unresolved),
             stream_ptr())
        return self._finish(1, points, d, idx, unresolved, return_stats)
