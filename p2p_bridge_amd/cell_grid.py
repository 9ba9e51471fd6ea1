"""The host side of csrc/cell_grid.h: a cloud as a uniform grid = its points sorted by the packed key of their cell.
Used by scan_fusion (radius counts, k-th neighbour distances, voxel keys), p2m_grid (face -> point) and knn_grid (k nearest
neighbours with indices, through scan_fusion's grid helpers)."""
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


def sorted_cells(xyz, cell, refuse, ids=None):
    """cell_keys, sorted -> (points sorted by cell key f32[n,3], sorted keys i64[n], the sorted points' rows in xyz i64[n], or
    ids[those rows] when the rows carry ids of their own); equal keys keep their order"""
    keys, bad = _keys(xyz, cell)
    skeys, perm = torch.sort(keys, stable=True)
    pts, rows = xyz[perm].contiguous(), perm if ids is None else ids[perm].contiguous()
    if int(bad.item()):  # (read back last: the sort and the gathers are queued by then)
        raise refuse
    return pts, skeys, rows
