"""Exact k nearest neighbours with their indices over a whole cloud, k <= 128: csrc/knn_grid.hip on the sorted cell-key grid
of cell_grid.py. The room-size form of denoise.knn_points (csrc/knn.hip: one workgroup and 4 n bytes of scratch per query):

    PointGrid(ref, k_hint, cell=None)        the grid of one reference cloud, built once
    PointGrid.knn(query, k)                  -> (dist2 f32[nq,k] ascending, idx i64[nq,k]), ties by ascending index
    PointGrid.nearest(query, order=None)     -> (dist2 f32[nq], idx i64[nq]): knn(query, 1) from csrc/nn_grid.hip, one lane
                                             per query; the room-size form of csrc/chamfer.hip (metrics.chamfer_grid)
    knn(query, ref, k, cell=None)            the one-shot form

The results are those of p2pb_knn_points bit for bit, ties included: both keep the k smallest keys (bits of sqdist3 << 32 |
index), which are all different, so the order in which the grid visits points cannot matter, and a ring of cells is final only
when every unvisited point is strictly farther than the k-th kept one ("Grid k-NN"). Stages: rings on the fitted
grid; what is left repeats on grids 4x and 16x coarser (isolated points); the rest walk the whole cloud. The ring count, level
count and pair threshold are scan_fusion.knn_kth_distance's. CUDA tensors only: there is no CPU path."""
import torch

from . import cell_grid
from ._lib import call, ptr, stream_ptr
from .scan_fusion import KNN_BRUTE_PAIRS, KNN_LEVELS, KNN_RINGS, _cuda, _grid, _knn_fit

F32, I32, U8 = torch.float32, torch.int32, torch.uint8
MAX_K = 128


def _k(k, what):
    k = int(k)
    if k > MAX_K:
        raise ValueError(f'{what}: k={k} exceeds {MAX_K}, the grid search\'s limit; use knn_points(method="brute")')
    if k < 1:
        raise ValueError(f"{what}: k={k} must be in [1, {MAX_K}]")
    return k


class PointGrid:
    """ref f32[n,3] (CUDA, contiguous) sorted by cell key. cell=None: the edge is fitted to the density as
    scan_fusion.knn_kth_distance fits it (the cell of the median point holds about k_hint/2 points); an explicit edge is taken
    as it is. NaN or inf in ref, or a cell index outside [-2^20, 2^20): ValueError."""

    def __init__(self, ref, k_hint, cell=None):
        k_hint = _k(k_hint, "PointGrid")
        _cuda(ref, F32, (None, 3), "ref")
        if ref.shape[0] == 0:
            raise ValueError("PointGrid: ref has no points")
        self.ref = ref
        if cell is None:
            level = _knn_fit(ref, k_hint, "PointGrid")
        else:
            level = _grid(ref, cell, "PointGrid")
        self.cell = level[3]
        self._levels = [self._level(*level)]

    @staticmethod
    def _level(pts, skeys, perm, cell):
        return pts, skeys, perm.to(I32), cell

    def level(self, i):
        """(sorted points, sorted keys, rows i32[n], cell edge) of the grid 4^i times coarser than the first; built on first
        use and kept"""
        while len(self._levels) <= i:
            self._levels.append(self._level(*_grid(self.ref, self._levels[-1][3] * 4.0, "PointGrid")))
        return self._levels[i]

    def _search(self, query, k):
        """-> dist2 f32[nq,k], idx i32[nq,k], stats"""
        k = _k(k, "PointGrid.knn")
        _cuda(query, F32, (None, 3), "query")
        ref = self.ref
        if query.device != ref.device:
            raise RuntimeError("PointGrid.knn: query and ref must be on one device")
        nq, n, dev = query.shape[0], ref.shape[0], ref.device
        if k > n:
            raise ValueError(f"PointGrid.knn: k={k} exceeds the {n} points of ref")
        if nq * k >= 2 ** 31:
            raise ValueError(f"PointGrid.knn: {nq} queries x k={k} is 2^31 or more")
        dist2 = torch.empty(nq, k, dtype=F32, device=dev)
        idx = torch.empty(nq, k, dtype=I32, device=dev)
        stats = {"ring": [0] * KNN_LEVELS, "brute": 0}
        if nq == 0:
            return dist2, idx, stats
        unresolved = torch.empty(nq, dtype=U8, device=dev)
        left = None  # the queries still open, i32 ascending (None: all)
        for lv in range(KNN_LEVELS):
            pts, skeys, rows, cell = self.level(lv)
            open_ = nq if left is None else left.numel()
            call("p2pb_knn_grid", open_, n, k, KNN_RINGS, ptr(left), ptr(query), ptr(pts), ptr(skeys), ptr(rows), cell,
                 ptr(dist2), ptr(idx), ptr(unresolved), stream_ptr())
            if left is None:
                left = torch.nonzero(unresolved).flatten().to(I32)
            else:
                left = left[unresolved[left.long()] != 0].contiguous()
            stats["ring"][lv] = open_ - left.numel()
            if left.numel() == 0 or left.numel() * n <= KNN_BRUTE_PAIRS:
                break
        if left.numel():
            call("p2pb_knn_grid_brute", left.numel(), n, k, ptr(left), ptr(query), ptr(ref), ptr(dist2), ptr(idx),
                 stream_ptr())
            stats["brute"] = left.numel()
        return dist2, idx, stats

    def knn(self, query, k, return_stats=False):
        """query f32[nq,3] -> (dist2 f32[nq,k] ascending, idx i64[nq,k] rows of ref, ties by ascending index); with
        return_stats also {"ring": [queries resolved by the rings of each level], "brute": queries left to the full walk}.
        1 <= k <= min(n, 128), whatever k_hint was (it only sets the cell edge)."""
        dist2, idx, stats = self._search(query, k)
        return (dist2, idx.long(), stats) if return_stats else (dist2, idx.long())

    def _nearest(self, query, order):
        """-> dist2 f32[nq], idx i32[nq], stats. order: None, or an i32 permutation of the queries that the CALLER answers
        for (an index outside [0, nq) would be followed)"""
        _cuda(query, F32, (None, 3), "query")
        ref = self.ref
        if query.device != ref.device:
            raise RuntimeError("PointGrid.nearest: query and ref must be on one device")
        nq, n, dev = query.shape[0], ref.shape[0], ref.device
        dist2 = torch.empty(nq, dtype=F32, device=dev)
        idx = torch.empty(nq, dtype=I32, device=dev)
        stats = {"ring": [0] * KNN_LEVELS, "brute": 0}
        if nq == 0:
            return dist2, idx, stats
        unresolved = torch.empty(nq, dtype=U8, device=dev)
        left = cell_grid.query_order(query, self.cell) if order is None else order  # the queries still open, in lane order
        for lv in range(KNN_LEVELS):
            pts, skeys, rows, cell = self.level(lv)
            open_ = left.numel()
            call("p2pb_nn_grid", open_, n, KNN_RINGS, ptr(left), ptr(query), ptr(pts), ptr(skeys), ptr(rows), cell, ptr(dist2),
                 ptr(idx), ptr(unresolved), stream_ptr())
            left = left[unresolved[left.long()] != 0].contiguous()
            stats["ring"][lv] = open_ - left.numel()
            if left.numel() == 0 or left.numel() * n <= KNN_BRUTE_PAIRS:
                break
        if left.numel():
            call("p2pb_knn_grid_brute", left.numel(), n, 1, ptr(left), ptr(query), ptr(ref), ptr(dist2), ptr(idx), stream_ptr())
            stats["brute"] = left.numel()
        return dist2, idx, stats

    def nearest(self, query, order=None, return_stats=False):
        """query f32[nq,3] -> (dist2 f32[nq], idx i64[nq]): knn(query, 1) with the last axis squeezed, bit for bit (the lowest
        row among equally near points), from csrc/nn_grid.hip: one lane per query and one running minimum instead of a wave
        and its best-list. Stages and stats as knn. order: an i32[nq] permutation of the queries that decides only which
        queries sit in neighbouring lanes -- not a bit of the result depends on it; None: the queries sorted by their cell key
        at this grid's edge (those outside the key range last). Hand in a spatially coherent one where it is already at hand,
        such as the sorted rows of the queries' own PointGrid."""
        if order is not None:
            _cuda(query, F32, (None, 3), "query")
            nq = query.shape[0]
            _cuda(order, I32, (nq,), "order")
            if order.device != self.ref.device:
                raise RuntimeError("PointGrid.nearest: order and ref must be on one device")
            rows = order.long()
            seen = torch.zeros(nq + 1, dtype=torch.bool, device=order.device)  # (slot nq: the rows outside [0, nq))
            seen[torch.where((rows < 0) | (rows >= nq), nq, rows)] = True
            if bool(seen[nq]) or not bool(seen[:nq].all()):
                raise ValueError("PointGrid.nearest: order must be a permutation of the query rows")
        dist2, idx, stats = self._nearest(query, order)
        return (dist2, idx.long(), stats) if return_stats else (dist2, idx.long())


def knn(query, ref, k, cell=None):
    """PointGrid(ref, k, cell).knn(query, k) -> (dist2 f32[nq,k], idx i64[nq,k])"""
    return PointGrid(ref, k, cell).knn(query, k)
