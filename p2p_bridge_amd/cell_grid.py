"""The host side of csrc/cell_grid.h: a cloud as a uniform grid = its points sorted by the packed key of their cell.
Used by scan_fusion (radius counts, k-th neighbour distances, voxel keys), p2m_grid (face -> point) and knn_grid (k nearest
neighbours with indices, through scan_fusion's grid helpers; the lane order of its nearest-point queries)."""
import torch

from ._lib import call, ptr, stream_ptr

KEY_HALF = 1 << 20  # cell indices lie in [-2^20, 2^20): include/p2pb_hip.h, "scan fusion"


def _keys(xyz, cell):
    n = xyz.shape[0]
    keys = torch.empty(n, dtype=torch.int64, device=xyz.device)
    bad = torch.zeros(1, dtype=torch.int32, device=xyz.device)
    call("p2pb_scan_cell_keys", n, ptr(xyz), cell, ptr(keys), ptr(bad), stream_ptr())
    return keys, bad


def cell_keys(xyz, cell, refuse):
    """packed cell keys i64[n] of xyz f32[n,3] (contiguous, n >= 1) at the fp32 cell edge `cell`; raises the exception
    `refuse` when a coordinate is NaN or a cell index leaves the key range"""
    keys, bad = _keys(xyz, cell)
    if int(bad.item()):
        raise refuse
    return keys


def query_order(xyz, cell):
    """the rows of xyz f32[n,3] (n >= 1) sorted by their cell key at the edge `cell`, i32[n]: neighbours in this order are
    neighbours in space, which is all the order is for (knn_grid.PointGrid.nearest). Rows with a NaN or a cell index outside
    the key range go last; equal keys keep their order"""
    keys, _ = _keys(xyz, cell)
    # the quotient of cell_grid.h (a tensor divisor: torch multiplies by the reciprocal of a plain number). A quotient that
    # differed by an ulp would only move a row within the order
    quot = torch.floor(xyz / torch.full((1,), cell, dtype=xyz.dtype, device=xyz.device))
    inside = ((quot >= -float(KEY_HALF)) & (quot < float(KEY_HALF))).all(1)
    keys = torch.where(inside, keys, torch.full_like(keys, torch.iinfo(torch.int64).max))
    return torch.sort(keys, stable=True)[1].to(torch.int32)


def sorted_cells(xyz, cell, refuse, ids=None):
    """cell_keys, sorted -> (points sorted by cell key f32[n,3], sorted keys i64[n], the sorted points' rows in xyz i64[n], or
    ids[those rows] when the rows carry ids of their own); equal keys keep their order"""
    keys, bad = _keys(xyz, cell)
    skeys, perm = torch.sort(keys, stable=True)
    pts, rows = xyz[perm].contiguous(), perm if ids is None else ids[perm].contiguous()
    if int(bad.item()):  # (read back last: the sort and the gathers are queued by then)
        raise refuse
    return pts, skeys, rows
