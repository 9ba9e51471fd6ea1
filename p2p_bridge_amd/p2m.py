"""Point <-> mesh distances as a loss: the reference's metrics/p2m.py on csrc/p2m_packed.hip.

    from p2p_bridge_amd.p2m import point_mesh_face_distance_custom, point_mesh_edge_distance, Meshes, Pointclouds

Same names, positional signatures and return values as metrics/p2m.py: four autograd Functions over packed batches
(`point_face_distance`, `face_point_distance`, `point_edge_distance`, `edge_point_distance`: squared distances with gradients
to the points and to the triangles / segments) and the two batched losses built on them. pytorch3d is a pip dependency of the
reference and absent here: the pair functions restate its published geometry (csrc/p2m_geom.h, pinned against oracle/), the
losses are duck-typed on the accessors they call, and `Meshes` / `Pointclouds` below provide exactly those accessors.
`metrics.point_face_distance` / `face_point_distance` stay the one-pair, no-gradient forms the evaluation metrics use.

Inside `p2p_bridge_amd.deterministic()` the target rows of every backward pass are summed in a fixed order (one wave per
target over lists built here with a stable sort); outside it they are fp32 atomic adds. Contract: include/p2pb_hip.h,
"point-to-mesh, packed batches with gradients".
"""

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ._lib import ask, call, check, ptr, stream_ptr

_DEFAULT_MIN_TRIANGLE_AREA: float = 5e-3

# include/p2pb_hip.h P2PB_P2M_*: (kind, queries are the points, vertices per primitive)
_POINT_FACE, _FACE_POINT, _POINT_EDGE, _EDGE_POINT = (0, True, 3), (1, False, 3), (2, True, 2), (3, False, 2)


def _check_pair(kind, points, prims):
    check(points, torch.float32, "points")
    check(prims, torch.float32, "tris" if kind[2] == 3 else "segms")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be [P, 3], got {tuple(points.shape)}")
    if prims.dim() != 3 or tuple(prims.shape[1:]) != (kind[2], 3):
        raise ValueError(f"{'tris' if kind[2] == 3 else 'segms'} must be [S, {kind[2]}, 3], got {tuple(prims.shape)}")
    if prims.device != points.device:
        raise RuntimeError("points and primitives must be on the same device")
    if points.shape[0] == 0 or prims.shape[0] == 0:
        raise ValueError("an example with no points or no primitives has no distance")


def _check_first(first, total, name, device):
    """first i64[N] on the device: ascending, every example non-empty and inside [0, total) -> the examples' counts (host)"""
    check(first, torch.int64, name)
    if first.dim() != 1 or first.shape[0] == 0 or first.device != device:
        raise ValueError(f"{name} must be i64[N] on the tensors' device, N >= 1")
    f = first.tolist() + [total]
    if f[0] != 0:
        raise ValueError(f"{name}[0] must be 0, got {f[0]}")
    counts = [b - a for a, b in zip(f[:-1], f[1:])]
    if min(counts) <= 0:
        raise ValueError(f"{name} = {f[:-1]} with {total} rows: every example needs at least one row (counts {counts})")
    return counts


def _forward(kind, points, points_first_idx, prims, prims_first_idx, max_queries, min_triangle_area):
    _check_pair(kind, points, prims)
    np_, ns = points.shape[0], prims.shape[0]
    cp = _check_first(points_first_idx, np_, "points_first_idx", points.device)
    cs = _check_first(prims_first_idx, ns, "tris_first_idx" if kind[2] == 3 else "segms_first_idx", points.device)
    if len(cp) != len(cs):
        raise ValueError(f"{len(cp)} examples of points, {len(cs)} of primitives")
    max_queries = int(max_queries)
    if max_queries < max(cp if kind[1] else cs):
        raise ValueError(f"max = {max_queries} is below the largest example's {max(cp if kind[1] else cs)} queries: their "
                         "distances would be left unwritten")
    nq = np_ if kind[1] else ns
    dists = torch.empty(nq, dtype=torch.float32, device=points.device)
    idxs = torch.empty(nq, dtype=torch.int64, device=points.device)
    call("p2pb_p2m_packed_forward", kind[0], len(cp), np_, ns, max_queries, ptr(points), ptr(points_first_idx), ptr(prims),
         ptr(prims_first_idx), min_triangle_area, ptr(dists), ptr(idxs), stream_ptr())
    return dists, idxs


def _backward(kind, points, prims, idxs, grad_dists, min_triangle_area):
    _check_pair(kind, points, prims)
    check(idxs, torch.int64, "idxs"), check(grad_dists, torch.float32, "grad_dists")
    np_, ns = points.shape[0], prims.shape[0]
    nq, nt = (np_, ns) if kind[1] else (ns, np_)
    if tuple(idxs.shape) != (nq,) or tuple(grad_dists.shape) != (nq,):
        raise ValueError(f"idxs and grad_dists must be [{nq}], got {tuple(idxs.shape)} and {tuple(grad_dists.shape)}")
    order = start = None
    if ask("p2pb_get_deterministic"):
        # target -> queries lists (plumbing): the queries sorted by their target, ties in ascending query index, and where every
        # target's run begins. The kernel then WRITES every target row, so nothing is zero-filled.
        sorted_idx, order = torch.sort(idxs, stable=True)
        start = torch.searchsorted(sorted_idx, torch.arange(nt + 1, dtype=torch.int64, device=idxs.device)).contiguous()
        grad_points, grad_prims = torch.empty_like(points), torch.empty_like(prims)
    elif kind[1]:
        grad_points, grad_prims = torch.empty_like(points), torch.zeros_like(prims)
    else:
        grad_points, grad_prims = torch.zeros_like(points), torch.empty_like(prims)
    call("p2pb_p2m_packed_backward", kind[0], np_, ns, ptr(points), ptr(prims), ptr(idxs), ptr(grad_dists), min_triangle_area,
         ptr(order), ptr(start), ptr(grad_points), ptr(grad_prims), stream_ptr())
    return grad_points, grad_prims


class _PointFaceDistance(Function):
    """dists[p] = squared distance of points[p] to the closest triangle of its example (pytorch3d point_face_dist_*)"""

    @staticmethod
    def forward(ctx, points, points_first_idx, tris, tris_first_idx, max_points,
                min_triangle_area=_DEFAULT_MIN_TRIANGLE_AREA):
        dists, idxs = _forward(_POINT_FACE, points, points_first_idx, tris, tris_first_idx, max_points, min_triangle_area)
        ctx.save_for_backward(points, tris, idxs)
        ctx.min_triangle_area = min_triangle_area
        return dists

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_dists):
        points, tris, idxs = ctx.saved_tensors
        grad_points, grad_tris = _backward(_POINT_FACE, points, tris, idxs, grad_dists.contiguous(), ctx.min_triangle_area)
        return grad_points, None, grad_tris, None, None, None


class _FacePointDistance(Function):
    """dists[t] = squared distance of tris[t] to the closest point of its example (pytorch3d face_point_dist_*)"""

    @staticmethod
    def forward(ctx, points, points_first_idx, tris, tris_first_idx, max_tris,
                min_triangle_area=_DEFAULT_MIN_TRIANGLE_AREA):
        dists, idxs = _forward(_FACE_POINT, points, points_first_idx, tris, tris_first_idx, max_tris, min_triangle_area)
        ctx.save_for_backward(points, tris, idxs)
        ctx.min_triangle_area = min_triangle_area
        return dists

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_dists):
        points, tris, idxs = ctx.saved_tensors
        grad_points, grad_tris = _backward(_FACE_POINT, points, tris, idxs, grad_dists.contiguous(), ctx.min_triangle_area)
        return grad_points, None, grad_tris, None, None, None


class _PointEdgeDistance(Function):
    """dists[p] = squared distance of points[p] to the closest segment of its example (pytorch3d point_edge_dist_*)"""

    @staticmethod
    def forward(ctx, points, points_first_idx, segms, segms_first_idx, max_points):
        dists, idxs = _forward(_POINT_EDGE, points, points_first_idx, segms, segms_first_idx, max_points, 0.0)
        ctx.save_for_backward(points, segms, idxs)
        return dists

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_dists):
        points, segms, idxs = ctx.saved_tensors
        grad_points, grad_segms = _backward(_POINT_EDGE, points, segms, idxs, grad_dists.contiguous(), 0.0)
        return grad_points, None, grad_segms, None, None


class _EdgePointDistance(Function):
    """dists[s] = squared distance of segms[s] to the closest point of its example (pytorch3d edge_point_dist_*)"""

    @staticmethod
    def forward(ctx, points, points_first_idx, segms, segms_first_idx, max_segms):
        dists, idxs = _forward(_EDGE_POINT, points, points_first_idx, segms, segms_first_idx, max_segms, 0.0)
        ctx.save_for_backward(points, segms, idxs)
        return dists

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_dists):
        points, segms, idxs = ctx.saved_tensors
        grad_points, grad_segms = _backward(_EDGE_POINT, points, segms, idxs, grad_dists.contiguous(), 0.0)
        return grad_points, None, grad_segms, None, None


point_face_distance = _PointFaceDistance.apply
face_point_distance = _FacePointDistance.apply
point_edge_distance = _PointEdgeDistance.apply
edge_point_distance = _EdgePointDistance.apply


# ---- the two accessors' worth of pytorch3d.structures that the losses below call ---------------------------------------------
def _first_idx(counts):
    return torch.cumsum(counts, 0) - counts


class Pointclouds:
    """Pointclouds(points: list of f32[P_i, 3]) -- the packed accessors of pytorch3d.structures.Pointclouds that
    metrics/p2m.py calls. The packed tensor is a torch.cat of the list, so gradients reach the list's tensors."""

    def __init__(self, points):
        points = list(points)
        if not points:
            raise ValueError("Pointclouds needs at least one cloud")
        for i, p in enumerate(points):
            if p.dim() != 2 or p.shape[1] != 3:
                raise ValueError(f"cloud {i} must be [P, 3], got {tuple(p.shape)}")
            if p.shape[0] == 0:
                raise ValueError(f"cloud {i} has no points")
        self._points = points
        self._packed = torch.cat(points, 0)
        self._num = torch.tensor([p.shape[0] for p in points], dtype=torch.int64, device=self._packed.device)

    def __len__(self):
        return len(self._points)

    def points_packed(self):
        return self._packed

    def num_points_per_cloud(self):
        return self._num

    def cloud_to_packed_first_idx(self):
        return _first_idx(self._num)

    def packed_to_cloud_idx(self):
        return torch.repeat_interleave(torch.arange(len(self), device=self._num.device), self._num)


class Meshes:
    """Meshes(verts: list of f32[V_i, 3], faces: list of i64[F_i, 3]) -- the packed accessors of pytorch3d.structures.Meshes
    that metrics/p2m.py calls. edges_packed: the three sides of every face as (min, max) vertex pairs, unique per mesh, ascending
    by (v0, v1), offset by the mesh's first vertex."""

    def __init__(self, verts, faces):
        verts, faces = list(verts), list(faces)
        if not verts or len(verts) != len(faces):
            raise ValueError("Meshes needs as many vertex tensors as face tensors, at least one")
        edges = []
        for i, (v, f) in enumerate(zip(verts, faces)):
            if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
                raise ValueError(f"mesh {i}: verts must be [V, 3] and faces [F, 3], got {tuple(v.shape)} and {tuple(f.shape)}")
            if f.dtype not in (torch.int64, torch.int32):
                raise ValueError(f"mesh {i}: faces must be integers")
            if v.shape[0] == 0 or f.shape[0] == 0:
                raise ValueError(f"mesh {i} has no vertices or no faces")
            if int(f.min()) < 0 or int(f.max()) >= v.shape[0]:
                raise ValueError(f"mesh {i}: a face names a vertex outside [0, {v.shape[0]})")
            f = f.long()
            sides = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
            sides = torch.stack([sides.min(dim=1).values, sides.max(dim=1).values], 1)
            edges.append(torch.unique(sides, dim=0))  # sorted: ascending by (v0, v1)
        dev = verts[0].device
        nv = torch.tensor([v.shape[0] for v in verts], dtype=torch.int64)
        v_first = (torch.cumsum(nv, 0) - nv).tolist()
        self._verts = verts
        self._verts_packed = torch.cat(verts, 0)
        self._faces_packed = torch.cat([f.long() + o for f, o in zip(faces, v_first)], 0).to(dev)
        self._edges_packed = torch.cat([e + o for e, o in zip(edges, v_first)], 0).to(dev)
        self._num_faces = torch.tensor([f.shape[0] for f in faces], dtype=torch.int64, device=dev)
        self._num_edges = torch.tensor([e.shape[0] for e in edges], dtype=torch.int64, device=dev)

    def __len__(self):
        return len(self._verts)

    def verts_packed(self):
        return self._verts_packed

    def faces_packed(self):
        return self._faces_packed

    def edges_packed(self):
        return self._edges_packed

    def num_faces_per_mesh(self):
        return self._num_faces

    def num_edges_per_mesh(self):
        return self._num_edges

    def mesh_to_faces_packed_first_idx(self):
        return _first_idx(self._num_faces)

    def mesh_to_edges_packed_first_idx(self):
        return _first_idx(self._num_edges)

    def faces_packed_to_mesh_idx(self):
        return torch.repeat_interleave(torch.arange(len(self), device=self._num_faces.device), self._num_faces)

    def edges_packed_to_mesh_idx(self):
        return torch.repeat_interleave(torch.arange(len(self), device=self._num_edges.device), self._num_edges)


# ---- the batched losses (metrics/p2m.py:243-375) ----------------------------------------------------------------------------
def _weighted(dists, counts, to_example, n):
    """every example's mean, summed, over the batch size: the reference's 1 / count weights"""
    return (dists * (1.0 / counts.gather(0, to_example).float())).sum() / n


def point_mesh_edge_distance(meshes, pcls):
    """point_edge(mesh, pcl) + edge_point(mesh, pcl): per example the mean squared distance of the points to the nearest edge
    plus that of the edges to the nearest point, averaged over the batch"""
    if len(meshes) != len(pcls):
        raise ValueError("meshes and pointclouds must be equal sized batches")
    n = len(meshes)
    points = pcls.points_packed()
    points_first_idx = pcls.cloud_to_packed_first_idx()
    max_points = pcls.num_points_per_cloud().max().item()
    segms = meshes.verts_packed()[meshes.edges_packed()]  # (S, 2, 3)
    segms_first_idx = meshes.mesh_to_edges_packed_first_idx()
    max_segms = meshes.num_edges_per_mesh().max().item()

    point_to_edge = point_edge_distance(points, points_first_idx, segms, segms_first_idx, max_points)
    point_dist = _weighted(point_to_edge, pcls.num_points_per_cloud(), pcls.packed_to_cloud_idx(), n)
    edge_to_point = edge_point_distance(points, points_first_idx, segms, segms_first_idx, max_segms)
    edge_dist = _weighted(edge_to_point, meshes.num_edges_per_mesh(), meshes.edges_packed_to_mesh_idx(), n)
    return point_dist + edge_dist


def point_mesh_face_distance_custom(meshes, pcls, min_triangle_area: float = _DEFAULT_MIN_TRIANGLE_AREA):
    """-> (point_dist, face_dist): per example the mean squared distance of the points to the nearest face, and of the faces
    to the nearest point, each averaged over the batch"""
    if len(meshes) != len(pcls):
        raise ValueError("meshes and pointclouds must be equal sized batches")
    n = len(meshes)
    points = pcls.points_packed()
    points_first_idx = pcls.cloud_to_packed_first_idx()
    max_points = pcls.num_points_per_cloud().max().item()
    tris = meshes.verts_packed()[meshes.faces_packed()]  # (T, 3, 3)
    tris_first_idx = meshes.mesh_to_faces_packed_first_idx()
    max_tris = meshes.num_faces_per_mesh().max().item()

    point_to_face = point_face_distance(points, points_first_idx, tris, tris_first_idx, max_points, min_triangle_area)
    point_dist = _weighted(point_to_face, pcls.num_points_per_cloud(), pcls.packed_to_cloud_idx(), n)
    face_to_point = face_point_distance(points, points_first_idx, tris, tris_first_idx, max_tris, min_triangle_area)
    face_dist = _weighted(face_to_point, meshes.num_faces_per_mesh(), meshes.faces_packed_to_mesh_idx(), n)
    return point_dist, face_dist
