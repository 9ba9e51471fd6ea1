"""Drop-in for the reference's compiled extension module `pointnet2_batch_cuda`
(third_party/openpoints/cpp/pointnet2_batch/src/pointnet2_api.cpp:31-47; same function names, argument
order, return lists, zero-initialised fresh outputs and RuntimeError preconditions), implemented on
the gfx950 C-ABI library. `p2p_bridge_amd.install_dropin()` registers it under the reference's
module names so the reference's Python runs unmodified.
"""
import ctypes
import os

import torch

from . import _experiment

from ._lib import P2PBError, ask, call, check, lib, ptr, stream_ptr  # noqa: F401  (lib: tests reach the loaded library through this module)

F32, I32 = torch.float32, torch.int32


def _ws(nbytes, device):
    return torch.empty((nbytes + 3) // 4, dtype=I32, device=device)


def voxel_coords(coords, resolution, normalize=True, eps=0.0):
    """Build addition: Voxelization.forward's normalisation as one deterministic kernel
    (models/pvcnn.py:215-228). Returns (norm_coords f32[B,3,N], vox_coords i32[B,3,N])."""
    check(coords, F32, "coords")
    b, _, n = coords.shape
    norm = torch.empty_like(coords)
    vox = torch.empty(b, 3, n, dtype=I32, device=coords.device)
    call("p2pb_voxel_coords", b, n, int(resolution), int(normalize), eps, ptr(coords), ptr(norm), ptr(vox), stream_ptr())
    return norm, vox


def avg_voxelize_forward(features, coords, resolution):
    """PN2/vox.cpp:17-44 -> [out f32[B,C,r^3], ind i32[B,N], cnt i32[B,r^3]]"""
    check(features, F32, "features"), check(coords, I32, "coords")
    b, c, n = features.shape
    r = int(resolution)
    r3 = r * r * r
    dev = features.device
    out = torch.empty(b, c, r3, dtype=F32, device=dev)
    ind = torch.empty(b, n, dtype=I32, device=dev)
    cnt = torch.empty(b, r3, dtype=I32, device=dev)
    ws = _ws(ask("p2pb_avg_voxelize_ws_bytes", b, n, r), dev)
    call("p2pb_avg_voxelize_forward", b, c, n, r, ptr(coords), ptr(features), ptr(ind), ptr(cnt), ptr(out), ptr(ws), stream_ptr())
    return [out, ind, cnt]


def avg_voxelize_backward(grad_y, indices, cnt):
    """PN2/vox.cpp:55-79"""
    check(grad_y, F32, "grad_y"), check(indices, I32, "indices"), check(cnt, I32, "cnt")
    b, c, s = grad_y.shape
    n = indices.shape[1]
    gx = torch.empty(b, c, n, dtype=F32, device=grad_y.device)
    call("p2pb_avg_voxelize_backward", b, c, n, s, ptr(indices), ptr(cnt), ptr(grad_y), ptr(gx),
         stream_ptr())
    return gx


def trilinear_devoxelize_forward(r, is_training, coords, features):
    """PN2/trilinear_devox.cpp:18-60 -> [outs, inds, wgts] (inds/wgts are [1] placeholders in eval)"""
    check(features, F32, "features"), check(coords, F32, "coords")
    b, c = features.shape[:2]
    n = coords.shape[2]
    dev = features.device
    outs = torch.empty(b, c, n, dtype=F32, device=dev)
    if is_training:
        inds = torch.empty(b, 8, n, dtype=I32, device=dev)
        wgts = torch.empty(b, 8, n, dtype=F32, device=dev)
    else:
        inds = torch.zeros(1, dtype=I32, device=dev)
        wgts = torch.zeros(1, dtype=F32, device=dev)
    call("p2pb_trilinear_devoxelize_forward", b, c, n, int(r), int(bool(is_training)), ptr(coords),
         ptr(features), ptr(inds), ptr(wgts), ptr(outs), stream_ptr())
    return [outs, inds, wgts]


def trilinear_devoxelize_backward(grad_y, indices, weights, r):
    """PN2/trilinear_devox.cpp:73-100"""
    check(grad_y, F32, "grad_y"), check(weights, F32, "weights"), check(indices, I32, "indices")
    b, c, n = grad_y.shape
    r3 = int(r) ** 3
    gx = torch.empty(b, c, r3, dtype=F32, device=grad_y.device)
    try:
        call("p2pb_trilinear_devoxelize_backward", b, c, n, r3, ptr(indices), ptr(weights), ptr(grad_y),
             ptr(gx), stream_ptr())
    except P2PBError as e:
        if not ask("p2pb_get_deterministic"):
            raise
        # (the library refuses a grid row beyond the LDS -- csrc/scatter_grad.hip SCAT_LDS_MAX, scat_rows -- in deterministic mode: only
        #  the global-atomic kernel, whose order is not fixed, would be left)
        raise P2PBError(f"trilinear_devoxelize_backward: no deterministic kernel for r = {r} (r^3 = {r3} voxels per grid row, "
                           "beyond what the fixed-order kernel holds in LDS): train this resolution outside "
                           "p2p_bridge_amd.deterministic()") from e
    return gx


def ball_query(centers_coords, points_coords, radius, num_neighbors):
    """PN2/pvcnn_ball_query.cpp:6-31 -> i32[B,M,U]"""
    check(centers_coords, F32, "centers_coords"), check(points_coords, F32, "points_coords")
    b, _, m = centers_coords.shape
    n = points_coords.shape[2]
    rf = ctypes.c_float(radius).value
    r2 = ctypes.c_float(rf * rf).value  # float*float, pvcnn_ball_query.cpp:25
    idx = torch.empty(b, m, int(num_neighbors), dtype=I32, device=centers_coords.device)
    call("p2pb_ball_query", b, n, m, r2, int(num_neighbors), ptr(centers_coords),
         ptr(points_coords), ptr(idx), stream_ptr())
    return idx


def grouping_forward(features, indices):
    """PN2/pvcnn_grouping.cpp:6-25"""
    check(features, F32, "features"), check(indices, I32, "indices")
    b, c, n = features.shape
    _, m, u = indices.shape
    out = torch.empty(b, c, m, u, dtype=F32, device=features.device)
    call("p2pb_grouping_forward", b, c, n, m, u, ptr(features), ptr(indices), ptr(out),
         stream_ptr())
    return out


def grouping_backward(grad_y, indices, n):
    """PN2/pvcnn_grouping.cpp:27-46"""
    check(grad_y, F32, "grad_y"), check(indices, I32, "indices")
    b, c, m, u = grad_y.shape
    gx = torch.empty(b, c, int(n), dtype=F32, device=grad_y.device)
    call("p2pb_grouping_backward", b, c, int(n), m, u, ptr(grad_y), ptr(indices), ptr(gx),
         stream_ptr())
    return gx


def sample_pitch(t):
    """floats between two samples of t if t[b] is contiguous for every b and the samples do not overlap (a contiguous tensor, or a
    channel slice t = big[:, lo:hi] of one), else None"""
    inner = 1
    for size, stride in zip(reversed(t.shape[1:]), reversed(t.stride()[1:])):
        if size != 1 and stride != inner:
            return None
        inner *= size
    return t.stride(0) if (t.shape[0] == 1 or t.stride(0) >= inner) else None


def grouping_backward_pitched(grad_y, indices, n):
    """build addition (training): grouping_backward reading a sample-pitched grad_y (`sample_pitch`) in place"""
    check(indices, I32, "indices")
    pitch = sample_pitch(grad_y)
    if pitch is None or grad_y.dtype != F32 or not grad_y.is_cuda:
        return grouping_backward(grad_y.contiguous(), indices, n)
    b, c, m, u = grad_y.shape
    gx = torch.empty(b, c, int(n), dtype=F32, device=grad_y.device)
    call("p2pb_grouping_backward_pitched", b, c, int(n), m, u, ptr(grad_y), max(pitch, c * m * u),
         ptr(indices), ptr(gx), stream_ptr())
    return gx


def three_nearest_neighbors_interpolate_backward_pitched(grad_y, indices, weights, m):
    """build addition (training): the same for three_nearest_neighbors_interpolate_backward"""
    check(indices, I32, "indices"), check(weights, F32, "weights")
    pitch = sample_pitch(grad_y)
    if pitch is None or grad_y.dtype != F32 or not grad_y.is_cuda:
        return three_nearest_neighbors_interpolate_backward(grad_y.contiguous(), indices, weights, m)
    b, c, n = grad_y.shape
    gx = torch.empty(b, c, int(m), dtype=F32, device=grad_y.device)
    call("p2pb_three_nn_interpolate_backward_pitched", b, c, n, int(m), ptr(grad_y), max(pitch, c * n),
         ptr(indices), ptr(weights), ptr(gx), stream_ptr())
    return gx


def gather_features_forward(features, indices):
    """PN2/pvcnn_sampling.cpp:6-23"""
    check(features, F32, "features"), check(indices, I32, "indices")
    b, c, n = features.shape
    m = indices.shape[1]
    out = torch.empty(b, c, m, dtype=F32, device=features.device)
    call("p2pb_gather_features_forward", b, c, n, m, ptr(features), ptr(indices), ptr(out),
         stream_ptr())
    return out


def gather_features_backward(grad_y, indices, n):
    """PN2/pvcnn_sampling.cpp:25-43"""
    check(grad_y, F32, "grad_y"), check(indices, I32, "indices")
    b, c, m = grad_y.shape
    gx = torch.empty(b, c, int(n), dtype=F32, device=grad_y.device)
    call("p2pb_gather_features_backward", b, c, int(n), m, ptr(grad_y), ptr(indices), ptr(gx),
         stream_ptr())
    return gx


# n > 16384: "grid" (pruned, one workgroup per cloud: 1.9x faster than `coop` at 50000 points, and b CUs instead of
# 64 b workgroups), "coop" (64 workgroups per cloud sharing the rounds), "single" (one workgroup streaming the cloud)
FPS_BIG_DEFAULT = "grid"


def furthest_point_sampling_forward(coords, num_samples):
    """PN2/pvcnn_sampling.cpp:45-61 -> i32[B,M]"""
    check(coords, F32, "coords")
    b, _, n = coords.shape
    m = int(num_samples)
    idx = torch.empty(b, m, dtype=I32, device=coords.device)
    big = _experiment.get("fps_big", FPS_BIG_DEFAULT)  # grid | coop | single
    if n > 16384 and m > 1 and big == "grid":
        # large clouds, pruned: one workgroup per cloud, a round revisits only the grid cells near the new sample
        # (csrc/sampling.hip fps_grid_kernel); same indices as every other FPS kernel here
        ws = torch.empty(int(ask("p2pb_fps_grid_ws_bytes", b, n)), dtype=torch.uint8, device=coords.device)
        call("p2pb_furthest_point_sampling_grid", b, n, m, ptr(coords), ptr(ws), ptr(idx), stream_ptr())
        return idx
    if 16384 < n <= 524288 and m > 1 and big != "single":
        # large clouds (BASELINE configs 4-5: 50000 points): 64 workgroups per cloud, four clouds per launch; same
        # indices as the single-workgroup kernel, 2.2x faster. A cooperative launch that loses a peer (GPU shared
        # with other work for the whole bounded spin) raises a per-cloud flag and the single-workgroup kernel
        # recomputes that cloud on the device: idx is valid either way, no host synchronisation needed.
        ws = torch.empty(int(ask("p2pb_fps_coop_ws_bytes", b, n)), dtype=torch.uint8, device=coords.device)
        rc = ask("p2pb_furthest_point_sampling_coop", b, n, m, ptr(coords), ptr(ws), ptr(idx), stream_ptr())
        if rc == 0:
            global _last_coop_flags
            _last_coop_flags = ws[b * 1024: b * 1024 + 4 * b].view(I32)  # diagnostics: fps_coop_fallbacks()
            return idx
        # (EINVAL: the device cannot hold 64 such workgroups at once -> single-workgroup kernel below)
    dist = torch.empty(b, n, dtype=F32, device=coords.device) if n > 16384 else None
    call("p2pb_furthest_point_sampling", b, n, m, ptr(coords), ptr(dist), ptr(idx), stream_ptr())
    return idx


_last_coop_flags = None


def fps_coop_fallbacks() -> int:
    """how many clouds of the LAST cooperative FPS call were recomputed by the single-workgroup fallback (synchronises)"""
    return 0 if _last_coop_flags is None else int(_last_coop_flags.sum().item())


furthest_point_sampling = furthest_point_sampling_forward  # name used by `_pvcnn_backend` (third_party/pvcnn/functional/src/bindings.cpp:15)


def three_nearest_neighbors_interpolate_forward(points_coords, centers_coords, centers_features):
    """PN2/pvcnn_neighbor_interpolate.cpp:6-41 -> [out f32[B,C,N], idx i32[B,3,N], w f32[B,3,N]]"""
    check(points_coords, F32, "points_coords"), check(centers_coords, F32, "centers_coords")
    check(centers_features, F32, "centers_features")
    b, c, m = centers_features.shape
    n = points_coords.shape[2]
    dev = points_coords.device
    idx = torch.empty(b, 3, n, dtype=I32, device=dev)
    w = torch.empty(b, 3, n, dtype=F32, device=dev)
    out = torch.empty(b, c, n, dtype=F32, device=dev)
    call("p2pb_three_nn_interpolate_forward", b, c, m, n, ptr(points_coords), ptr(centers_coords),
         ptr(centers_features), ptr(idx), ptr(w), ptr(out), stream_ptr())
    return [out, idx, w]


def three_nearest_neighbors_interpolate_backward(grad_y, indices, weights, m):
    """PN2/pvcnn_neighbor_interpolate.cpp:43-70"""
    check(grad_y, F32, "grad_y"), check(indices, I32, "indices"), check(weights, F32, "weights")
    b, c, n = grad_y.shape
    gx = torch.empty(b, c, int(m), dtype=F32, device=grad_y.device)
    call("p2pb_three_nn_interpolate_backward", b, c, n, int(m), ptr(grad_y), ptr(indices),
         ptr(weights), ptr(gx), stream_ptr())
    return gx


def three_nn(points_coords, centers_coords):
    """build addition: the search half of the op -> (idx i32[B,3,N], w f32[B,3,N])"""
    check(points_coords, F32, "points_coords"), check(centers_coords, F32, "centers_coords")
    b, _, n = points_coords.shape
    m = centers_coords.shape[2]
    idx = torch.empty(b, 3, n, dtype=I32, device=points_coords.device)
    w = torch.empty(b, 3, n, dtype=F32, device=points_coords.device)
    if 256 <= m and _experiment.get("nn_cells", "1") != "0":  # grid search (exact) once brute force is the slower one
        # (records in LDS up to 8192 centres, L2-resident above: PVDL's 12500-centre level)
        ws = _ws(ask("p2pb_three_nn_cells_ws_bytes", b, m), points_coords.device)
        call("p2pb_three_nn_cells", b, m, n, ptr(points_coords), ptr(centers_coords), ptr(idx), ptr(w), ptr(ws), stream_ptr())
        return idx, w
    call("p2pb_three_nn", b, m, n, ptr(points_coords), ptr(centers_coords), ptr(idx), ptr(w), stream_ptr())
    return idx, w


def three_interpolate(centers_features, idx, w):
    """build addition: the interpolation half -> f32[B,C,N]"""
    check(centers_features, F32, "centers_features"), check(idx, I32, "idx"), check(w, F32, "w")
    b, c, m = centers_features.shape
    n = idx.shape[2]
    out = torch.empty(b, c, n, dtype=F32, device=centers_features.device)
    call("p2pb_three_interpolate", b, c, m, n, ptr(centers_features), ptr(idx), ptr(w), ptr(out),
         stream_ptr())
    return out


def group_concat(points_coords, centers_coords, points_features, indices):
    """build addition (inference): [coords[:, idx] - centers | features[:, idx]] -> f32[B, 3+C, M, U]"""
    check(points_coords, F32, "points_coords"), check(centers_coords, F32, "centers_coords")
    check(points_features, F32, "points_features"), check(indices, I32, "indices")
    b, c, n = points_features.shape
    _, m, u = indices.shape
    out = torch.empty(b, 3 + c, m, u, dtype=F32, device=points_features.device)
    call("p2pb_group_concat", b, c, n, m, u, ptr(points_coords), ptr(centers_coords),
         ptr(points_features), ptr(indices), ptr(out), stream_ptr())
    return out


# ---- the classic PointNet++ operators (PN2/pointnet2_api.cpp:17-29; csrc/ball_query.hip, three_nn.hip) --------------
# Clouds are POINT-major f32[B,N,3]. The caller allocates every output and passes the sizes as integers, exactly as the
# reference's layers do (third_party/openpoints/models/layers/{group,subsample,upsampling}.py); the kernels run on the
# current stream and write into the caller's tensors. The reference's `int` functions return 1, its `void` ones None.
# Where the reference exit(-1)s on a launch error or reads whatever memory a mismatched argument names, these raise
# RuntimeError: wrong device, dtype, contiguity, or a shape that disagrees with the integers.

def _pn2_check(*specs):
    """specs: (tensor, dtype, name, shape). `check` on each, one device for all, shapes equal to what the integers say."""
    dev = None
    for t, dtype, name, shape in specs:
        check(t, dtype, name)
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"{name} is on {t.device}, the other tensors on {dev}")
        if tuple(t.shape) != tuple(shape):
            raise RuntimeError(f"{name} must have shape {tuple(shape)} for the sizes passed, got {tuple(t.shape)}")


def ball_query_wrapper(b, n, m, radius, nsample, new_xyz, xyz, idx):
    """PN2/ball_query.cpp:29. new_xyz f32[B,M,3], xyz f32[B,N,3] -> idx i32[B,M,nsample] (rows without a neighbour are left
    as they are: the layer zero-fills idx first, group.py:198)"""
    b, n, m, nsample = int(b), int(n), int(m), int(nsample)
    _pn2_check((new_xyz, F32, "new_xyz", (b, m, 3)), (xyz, F32, "xyz", (b, n, 3)), (idx, I32, "idx", (b, m, nsample)))
    call("p2pb_pn2_ball_query", b, n, m, radius, nsample, ptr(new_xyz), ptr(xyz), ptr(idx), stream_ptr())
    return 1


def group_points_wrapper(b, c, n, npoints, nsample, points, idx, out):
    """PN2/group_points.cpp:25. points f32[B,C,N], idx i32[B,npoints,nsample] -> out f32[B,C,npoints,nsample]"""
    b, c, n, npoints, nsample = int(b), int(c), int(n), int(npoints), int(nsample)
    _pn2_check((points, F32, "points", (b, c, n)), (idx, I32, "idx", (b, npoints, nsample)),
               (out, F32, "out", (b, c, npoints, nsample)))
    call("p2pb_grouping_forward", b, c, n, npoints, nsample, ptr(points), ptr(idx), ptr(out), stream_ptr())
    return 1


def group_points_grad_wrapper(b, c, n, npoints, nsample, grad_out, idx, grad_points):
    """PN2/group_points.cpp:13. ADDS the scattered grad_out f32[B,C,npoints,nsample] into grad_points f32[B,C,N]: the
    library's scatter writes a fresh tensor, which is then added to the caller's."""
    b, c, n, npoints, nsample = int(b), int(c), int(n), int(npoints), int(nsample)
    _pn2_check((grad_out, F32, "grad_out", (b, c, npoints, nsample)), (idx, I32, "idx", (b, npoints, nsample)),
               (grad_points, F32, "grad_points", (b, c, n)))
    grad_points.add_(grouping_backward(grad_out, idx, n))
    return 1


def gather_points_wrapper(b, c, n, npoints, points, idx, out):
    """PN2/sampling.cpp:16. points f32[B,C,N], idx i32[B,npoints] -> out f32[B,C,npoints]"""
    b, c, n, npoints = int(b), int(c), int(n), int(npoints)
    _pn2_check((points, F32, "points", (b, c, n)), (idx, I32, "idx", (b, npoints)), (out, F32, "out", (b, c, npoints)))
    call("p2pb_gather_features_forward", b, c, n, npoints, ptr(points), ptr(idx), ptr(out), stream_ptr())
    return 1


def gather_points_grad_wrapper(b, c, n, npoints, grad_out, idx, grad_points):
    """PN2/sampling.cpp:27. ADDS the scattered grad_out f32[B,C,npoints] into grad_points f32[B,C,N] (as
    group_points_grad_wrapper)"""
    b, c, n, npoints = int(b), int(c), int(n), int(npoints)
    _pn2_check((grad_out, F32, "grad_out", (b, c, npoints)), (idx, I32, "idx", (b, npoints)),
               (grad_points, F32, "grad_points", (b, c, n)))
    grad_points.add_(gather_features_backward(grad_out, idx, n))
    return 1


def furthest_point_sampling_wrapper(b, n, m, points, temp, idx):
    """PN2/sampling.cpp:39. points f32[B,N,3], temp f32[B,N] in/out (the layer fills it with 1e10) -> idx i32[B,m];
    tie order of the reference's min(2^floor(log2 N), 1024)-thread block (include/p2pb_hip.h p2pb_pn2_fps)"""
    b, n, m = int(b), int(n), int(m)
    _pn2_check((points, F32, "points", (b, n, 3)), (temp, F32, "temp", (b, n)), (idx, I32, "idx", (b, max(m, 0))))
    call("p2pb_pn2_fps", b, n, m, ptr(points), ptr(temp), ptr(idx), stream_ptr())
    return 1


def three_nn_wrapper(b, n, m, unknown, known, dist2, idx):
    """PN2/interpolate.cpp:20. unknown f32[B,N,3], known f32[B,m,3] -> dist2 f32[B,N,3] (squared), idx i32[B,N,3]"""
    b, n, m = int(b), int(n), int(m)
    _pn2_check((unknown, F32, "unknown", (b, n, 3)), (known, F32, "known", (b, m, 3)), (dist2, F32, "dist2", (b, n, 3)),
               (idx, I32, "idx", (b, n, 3)))
    call("p2pb_pn2_three_nn", b, n, m, ptr(unknown), ptr(known), ptr(dist2), ptr(idx), stream_ptr())


def three_interpolate_wrapper(b, c, m, n, points, idx, weight, out):
    """PN2/interpolate.cpp:31. points f32[B,c,m], idx i32[B,n,3], weight f32[B,n,3] -> out f32[B,c,n]"""
    b, c, m, n = int(b), int(c), int(m), int(n)
    _pn2_check((points, F32, "points", (b, c, m)), (idx, I32, "idx", (b, n, 3)), (weight, F32, "weight", (b, n, 3)),
               (out, F32, "out", (b, c, n)))
    call("p2pb_pn2_three_interpolate", b, c, m, n, ptr(points), ptr(idx), ptr(weight), ptr(out), stream_ptr())


def three_interpolate_grad_wrapper(b, c, n, m, grad_out, idx, weight, grad_points):
    """PN2/interpolate.cpp:45. ADDS grad_out f32[B,c,n] * weight at idx into grad_points f32[B,c,m] (fp32 atomics in no
    fixed order: refused inside p2p_bridge_amd.deterministic())"""
    b, c, n, m = int(b), int(c), int(n), int(m)
    _pn2_check((grad_out, F32, "grad_out", (b, c, n)), (idx, I32, "idx", (b, n, 3)), (weight, F32, "weight", (b, n, 3)),
               (grad_points, F32, "grad_points", (b, c, m)))
    if ask("p2pb_get_deterministic"):
        raise P2PBError("three_interpolate_grad_wrapper: no deterministic kernel (it accumulates with fp32 atomics, whose order is "
                        "not fixed): run this backward pass outside p2p_bridge_amd.deterministic()")
    call("p2pb_pn2_three_interpolate_grad", b, c, n, m, ptr(grad_out), ptr(idx), ptr(weight), ptr(grad_points), stream_ptr())
