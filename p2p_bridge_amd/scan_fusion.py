"""iPhone scans from depth frames: the GPU stages of the reference's data/scannetpp/iphone/process_dataset.py:102-283 with
the helpers of data/scannetpp/iphone/arkit_pcl.py, which run there through Open3D's CUDA tensor geometry and cuML.

    backproject              arkit_pcl.py:235-255    valid pixels of a depth frame -> world points + colours
    voxel_down_sample        Open3D tensor PointCloud.voxel_down_sample / voxel_down_sample_with_features (:61-90)
    remove_radius_outliers   Open3D tensor PointCloud.remove_radius_outliers (:260)
    knn_kth_distance         cuML NearestNeighbors(k).fit(ref).kneighbors(query)[0][:, -1]
    outlier_removal          outlier_removal_cuml :117-154
    filter_iphone_scan       filter_iphone_scan_fast :36-58
    process_frame            process_dataset.py:102-134
    fuse_frames              process_dataset.py:233-273
    python -m p2p_bridge_amd.scan_fusion   process_dataset.py:137-283 (the video / depth-stream decoding stays out)

Every function takes and returns CUDA tensors and runs the kernels of csrc/scan.hip; a CPU tensor raises RuntimeError (there is
no fallback). Torch does the plumbing: sorting keys, prefix sums, boolean compaction, mean and standard deviation of a vector.
No float atomics: the same inputs give the same bits. Contract of the kernels: include/p2pb_hip.h, "scan fusion"; what is taken
from Open3D's and cuML's documentation and not from a run: INTEGRATION.md.

The neighbour search (radius counts, k-th distances) is a uniform grid held as SORTED CELL KEYS: the reference points sorted by
the packed key of their cell. Memory is O(n) whatever the bounding box, and one column of cells is one run of the sorted
points, found by two binary searches. DESIGN.md section 3.7.
"""
import argparse
import ctypes
import json
import math
import os

import numpy as np
import torch

from . import cell_grid
from ._lib import ask, call, ptr, stream_ptr

F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
SMALL_VOXEL = 64  # voxels of up to this many points: one thread per (voxel, channel); larger: chunks of a workgroup each
KNN_RINGS = 3  # rings of cells a k-NN query walks on one grid before it moves on
KNN_LEVELS = 3  # grids (cell, 4 cell, 16 cell) before the brute-force pass
KNN_BRUTE_PAIRS = 1 << 31  # unresolved queries x reference points below which the brute-force pass is taken at once
KNN_MAX_K = 64


def _cuda(t, dtype, shape, name):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{name} must be a CUDA tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must be {str(dtype).replace('torch.', '')}, got {str(t.dtype).replace('torch.', '')}")
    if t.dim() != len(shape) or any(s is not None and t.shape[i] != s for i, s in enumerate(shape)):
        raise ValueError(f"{name} must have shape {list('?' if s is None else s for s in shape)}, got {list(t.shape)}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous tensor")
    if t.numel() >= 2 ** 31:
        raise ValueError(f"{name} has {t.numel()} elements, 2^31 or more")


def _host64(m, shape, name):
    m = m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m)
    m = np.ascontiguousarray(m, dtype=np.float64)
    if m.shape != shape:
        raise ValueError(f"{name} must have shape {list(shape)}, got {list(m.shape)}")
    return m


# ---- back-projection -------------------------------------------------------------------------------------------------
def backproject(image, depth, camera_to_world, intrinsic, min_depth=0.1, max_depth=10.0, intrinsic_scale=256 / 1920):
    """arkit_pcl.py:235-255. image u8[H,W,3] at the depth map's resolution, depth f32[H,W] in metres (both CUDA);
    camera_to_world 4x4 and intrinsic 3x3 (numpy or tensor, read as fp64 on the host). The intrinsic's fx, fy, cx, cy are scaled
    by intrinsic_scale and the 3x3 inverse is taken on the host in fp64. A pixel is valid iff not (z < min or z > max or NaN or
    +-inf), the bounds compared as fp32 like the depth map (a depth equal to a bound is valid). fp64 throughout:
    world = c2w . (Kinv . (x, y, 1) . z, 1), rounded to fp32 once.
    -> xyz f32[n,3], rgb f32[n,3] (the bytes 0..255 as floats, unscaled), the valid pixels in row-major order; (0,3) and no
    point kernel when no pixel is valid."""
    _cuda(depth, F32, (None, None), "depth")
    h, w = depth.shape
    _cuda(image, U8, (h, w, 3), "image")
    if image.device != depth.device:
        raise RuntimeError("backproject: image and depth must be on one device")
    c2w = _host64(camera_to_world, (4, 4), "camera_to_world")
    k = _host64(intrinsic, (3, 3), "intrinsic").copy()
    for i, j in ((0, 0), (1, 1), (0, 2), (1, 2)):
        k[i, j] *= intrinsic_scale
    kinv = np.ascontiguousarray(np.linalg.inv(k))
    dev = depth.device
    if h * w == 0:
        return torch.empty(0, 3, dtype=F32, device=dev), torch.empty(0, 3, dtype=F32, device=dev)
    valid = torch.empty(h * w, dtype=U8, device=dev)
    call("p2pb_scan_depth_valid", h * w, ptr(depth), min_depth, max_depth, ptr(valid), stream_ptr())
    pix = torch.nonzero(valid).flatten()  # i64, ascending = row-major
    n = pix.numel()
    xyz, rgb = torch.empty(n, 3, dtype=F32, device=dev), torch.empty(n, 3, dtype=F32, device=dev)
    if n:
        call("p2pb_scan_backproject", n, w, h, ptr(pix), ptr(image), ptr(depth),
             kinv.ctypes.data_as(ctypes.c_void_p), c2w.ctypes.data_as(ctypes.c_void_p), ptr(xyz), ptr(rgb), stream_ptr())
    return xyz, rgb


# ---- cell keys and the sorted grid -----------------------------------------------------------------------------------
def _cell(cell, what):
    """-> (the cell edge as the kernels see it: fp32(cell), positive and finite; the ValueError for a cell index that leaves
    [-2^20, 2^20))"""
    cell = float(np.float32(cell))
    if not (cell > 0.0 and math.isfinite(cell)):
        raise ValueError(f"{what}: cell size {cell} must be positive and finite")
    return cell, ValueError(f"{what}: a coordinate is NaN or its cell index at size {cell} lies outside [-2^20, 2^20)")


def _grid(ref, cell, what):
    """-> (points sorted by cell key f32[n,3], sorted keys i64[n], the permutation i64[n], the cell edge as the kernels see it)"""
    cell, refuse = _cell(cell, what)
    return cell_grid.sorted_cells(ref, cell, refuse) + (cell,)


# ---- voxel down-sampling ---------------------------------------------------------------------------------------------
def voxel_down_sample(xyz, voxel_size, *attrs):
    """Open3D's tensor PointCloud.voxel_down_sample(voxel_size), with any number of attribute tensors f32[n,c] averaged along
    (voxel_down_sample_with_features, arkit_pcl.py:61-90). Key per axis: floor(fp32(p / fp32(voxel_size))), an IEEE fp32 divide,
    no bounding-box shift (-0.001 lies in voxel -1); keys outside [-2^20, 2^20): ValueError. One row per occupied voxel, sorted
    ascending by (kx, ky, kz) -- Open3D's order is its hash map's; a fixed one makes runs repeatable. Each row is the mean of
    the voxel's positions and attributes: fp64 sums in a fixed order, one rounding to fp32.
    -> (xyz f32[m,3], *attrs f32[m,c]) -- always a tuple."""
    _cuda(xyz, F32, (None, 3), "xyz")
    n = xyz.shape[0]
    for i, a in enumerate(attrs):
        _cuda(a, F32, (n, None), f"attrs[{i}]")
        if a.shape[1] < 1 or a.device != xyz.device:
            raise ValueError(f"attrs[{i}] must have at least one channel and live on the device of xyz")
    if n == 0:
        return (xyz.clone(),) + tuple(a.clone() for a in attrs)
    skeys, perm = torch.sort(cell_grid.cell_keys(xyz, *_cell(voxel_size, "voxel_down_sample")), stable=True)
    _, counts = torch.unique_consecutive(skeys, return_counts=True)
    m = counts.numel()
    starts = torch.zeros(m + 1, dtype=I64, device=xyz.device)
    torch.cumsum(counts, 0, out=starts[1:])
    big = torch.nonzero(counts > SMALL_VOXEL).flatten()
    nbig = big.numel()
    if nbig:
        rows = int(ask("p2pb_scan_big_chunk_rows"))
        per = (counts[big] + rows - 1) // rows  # chunks of each large voxel
        chunk_begin = torch.zeros(nbig + 1, dtype=I64, device=xyz.device)
        torch.cumsum(per, 0, out=chunk_begin[1:])
        nchunks = int(chunk_begin[-1].item())
        owner = torch.repeat_interleave(torch.arange(nbig, device=xyz.device), per)
        within = torch.arange(nchunks, device=xyz.device) - chunk_begin[owner]
        chunk_row0 = (starts[big[owner]] + within * rows).contiguous()
        chunk_rows = torch.minimum(starts[big[owner] + 1] - chunk_row0, torch.full_like(chunk_row0, rows)).contiguous()
    out = []
    for src in (xyz,) + tuple(attrs):
        c = src.shape[1]
        if m * c >= 2 ** 31:
            raise ValueError(f"voxel_down_sample: {m} voxels x {c} channels is 2^31 or more")
        dst = torch.empty(m, c, dtype=F32, device=xyz.device)
        call("p2pb_scan_segment_mean", m, c, SMALL_VOXEL, ptr(src), ptr(perm), ptr(starts), ptr(dst), stream_ptr())
        if nbig:
            partial = torch.empty(nchunks, c, dtype=F64, device=xyz.device)
            call("p2pb_scan_segment_mean_big", nbig, nchunks, c, ptr(src), ptr(perm),
                 ptr(starts), ptr(big), ptr(chunk_begin), ptr(chunk_row0), ptr(chunk_rows), ptr(partial), ptr(dst), stream_ptr())
        out.append(dst)
    return tuple(out)


# ---- radius outliers -------------------------------------------------------------------------------------------------
def remove_radius_outliers(xyz, nb_points, search_radius, include_self=True):
    """Open3D's remove_radius_outliers as a mask: point i is kept iff #{ j : sqdist3(p_i - p_j) <= fp32(r*r) } >= nb_points,
    the point itself counted unless include_self=False. Exact: a grid of cell edge r, the 27 cells around each point's.
    -> bool[n]"""
    _cuda(xyz, F32, (None, 3), "xyz")
    n, dev = xyz.shape[0], xyz.device
    need = int(nb_points) + (0 if include_self else 1)
    if n == 0 or need <= 0:
        return torch.ones(n, dtype=torch.bool, device=dev)
    r = float(search_radius)
    if not (r > 0.0 and math.isfinite(r)):
        raise ValueError(f"remove_radius_outliers: search_radius {search_radius} must be positive and finite")
    r2 = np.float32(r * r)
    # the largest per-axis |p - q| that can pass the fp32 test: sqrt(r2) with the roundings of sqdist3 and of the difference
    # (under 4 * 2^-24 together) added, rounded up
    reach = np.nextafter(np.float32(math.sqrt(float(r2)) * (1.0 + 1e-6)), np.float32(np.inf))
    pts, skeys, perm, cell = _grid(xyz, r, "remove_radius_outliers")
    counts = torch.empty(n, dtype=I32, device=dev)
    call("p2pb_scan_radius_count", n, n, ptr(pts), ptr(pts), ptr(skeys), cell,
         float(r2), float(reach), min(need, 2 ** 31 - 1), ptr(counts), stream_ptr())
    mask = torch.empty(n, dtype=torch.bool, device=dev)
    mask[perm] = counts >= need  # (the queries ran in sorted order: neighbouring threads read the same cells)
    return mask


# ---- k-th neighbour distance -----------------------------------------------------------------------------------------
def _knn_cell(ref, k, what="knn_kth_distance"):
    """a first cell edge from the bounding box (k points per cell if the cloud filled it), and the smallest edge that keeps
    every key in range"""
    lo, hi = ref.min(0).values.double().cpu().numpy(), ref.max(0).values.double().cpu().numpy()
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError(f"{what}: ref holds NaN or inf")
    amax = float(max(np.abs(lo).max(), np.abs(hi).max()))
    floor = max(amax * 2.0 ** -19, 1e-30)
    ext = (hi - lo)[(hi - lo) > 0]
    cell = float((k * np.prod(ext) / ref.shape[0]) ** (1.0 / len(ext))) if len(ext) else 1.0
    return max(cell, floor), floor


def _knn_fit(ref, k, what):
    """the grid of ref (as _grid returns it) at a cell edge fitted to the density: the edge is moved, at most three times, until
    the cell of the median point holds about k/2 points. Also knn_grid.PointGrid's."""
    n, dev = ref.shape[0], ref.device
    cell, floor = _knn_cell(ref, k, what)
    target = max(k / 2.0, 2.0)
    for it in range(4):
        pts, skeys, perm, cell = _grid(ref, cell, what)
        if it == 3:
            break
        counts = torch.unique_consecutive(skeys, return_counts=True)[1].sort().values
        half = torch.searchsorted(torch.cumsum(counts, 0), torch.tensor([(n + 1) // 2], device=dev))
        occ = float(counts[half.clamp(max=counts.numel() - 1)].item())  # points in the cell of the median point
        if target / 2.0 <= occ <= target * 2.0:
            break
        step = min(8.0, max(0.125, (target / occ) ** 0.4))  # occupancy grows like cell^2 (surfaces) to cell^3
        if cell * step < floor and cell <= floor * 1.0001:
            break
        cell = max(cell * step, floor)
    return pts, skeys, perm, cell


def knn_kth_distance(query, ref, k):
    """The Euclidean distance from each query point to its k-th nearest point of ref, 1 <= k <= 64: the fp32 square root of the
    k-th smallest fp32 sqdist3. Exact (the true order statistic). When query is ref the point itself is neighbour 1 at
    distance 0, as cuML's kneighbors on its own fit data returns it. k > n_ref: ValueError.
    query f32[nq,3], ref f32[n,3] -> f32[nq].
    The cell edge is fitted to the density: it is moved until the cell of the median point holds about k/2 points (on a
    surface the k-th neighbour then lies within one cell edge, and the 27 cells hold a few k candidates). Each query walks up to
    KNN_RINGS rings; what is left repeats on a grid four times coarser (isolated points), and at last in a brute-force pass."""
    _cuda(query, F32, (None, 3), "query")
    _cuda(ref, F32, (None, 3), "ref")
    if query.device != ref.device:
        raise RuntimeError("knn_kth_distance: query and ref must be on one device")
    k = int(k)
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"knn_kth_distance: k={k} must be in [1, {KNN_MAX_K}]")
    nq, n, dev = query.shape[0], ref.shape[0], ref.device
    if k > n:
        raise ValueError(f"knn_kth_distance: k={k} exceeds the {n} points of ref")
    out = torch.empty(nq, dtype=F32, device=dev)
    if nq == 0:
        return out
    pts, skeys, _, cell = _knn_fit(ref, k, "knn_kth_distance")
    unresolved = torch.empty(nq, dtype=U8, device=dev)
    call("p2pb_scan_knn_grid", nq, n, k, KNN_RINGS, None, ptr(query),
         ptr(pts), ptr(skeys), cell, ptr(out), ptr(unresolved), stream_ptr())
    left = torch.nonzero(unresolved).flatten().to(I32)
    level = 1
    while left.numel():
        if level >= KNN_LEVELS or left.numel() * n <= KNN_BRUTE_PAIRS:
            call("p2pb_scan_knn_brute", left.numel(), n, k, ptr(left), ptr(query),
                 ptr(ref), ptr(out), stream_ptr())
            break
        level += 1
        pts, skeys, _, cell = _grid(ref, cell * 4.0, "knn_kth_distance")
        call("p2pb_scan_knn_grid", left.numel(), n, k, KNN_RINGS,
             ptr(left), ptr(query), ptr(pts), ptr(skeys), cell, ptr(out), ptr(unresolved), stream_ptr())
        left = left[unresolved[left.long()] != 0].contiguous()
    return out


# ---- the two filters on top of it ------------------------------------------------------------------------------------
def _band(d, low, high):
    """mean and population standard deviation in fp64 of the fp32 distances -> (mean + high*std, mean - low*std)"""
    d64 = d.double()
    mean, std = d64.mean(), d64.std(unbiased=False)
    return d64, mean + high * std, mean - low * std


def outlier_removal(xyz, nb_points, radius, std_thresh=None):
    """outlier_removal_cuml (arkit_pcl.py:117-154) as a mask over xyz f32[n,3]. Without std_thresh: keep iff the distance to
    the nb_points-th neighbour (the point itself is the first) is < radius. With std_thresh: k is FORCED to 20 (the
    reference's quirk, :130-131; nb_points and radius are then unused) and a point is kept iff
    mean - t*std < kth < mean + t*std, mean and population std (ddof=0) in fp64 from the fp32 distances. -> bool[n]"""
    _cuda(xyz, F32, (None, 3), "xyz")
    if xyz.shape[0] == 0:
        return torch.ones(0, dtype=torch.bool, device=xyz.device)
    kth = knn_kth_distance(xyz, xyz, 20 if std_thresh is not None else int(nb_points))
    if std_thresh is None:
        return kth < float(np.float32(radius))  # (fp32 against the fp32 distances, as numpy compares them there)
    d64, upper, lower = _band(kth, float(std_thresh), float(std_thresh))
    return (d64 < upper) & (d64 > lower)


def filter_iphone_scan(iphone_xyz, faro_xyz, threshold=1.0):
    """filter_iphone_scan_fast (arkit_pcl.py:36-58) as a mask: keep the iPhone points whose distance to the nearest Faro point
    is < mean + threshold * std over all iPhone points (fp64 statistics of the fp32 distances). -> bool[n]"""
    _cuda(iphone_xyz, F32, (None, 3), "iphone_xyz")
    _cuda(faro_xyz, F32, (None, 3), "faro_xyz")
    if iphone_xyz.shape[0] == 0:
        return torch.ones(0, dtype=torch.bool, device=iphone_xyz.device)
    d64, upper, _ = _band(knn_kth_distance(iphone_xyz, faro_xyz, 1), 0.0, float(threshold))
    return d64 < upper


# ---- the composition -------------------------------------------------------------------------------------------------
def build_parser():
    """the options of process_dataset.py:138-181, names and defaults"""
    p = argparse.ArgumentParser(prog="python -m p2p_bridge_amd.scan_fusion", description=__doc__.split("\n")[0])
    p.add_argument("--data_root", type=str, required=True)
    p.add_argument("--filename", type=str, default="iphone", help="Name of the iphone scans.")
    p.add_argument("--split", type=int, default=None, help="Split id to process")
    p.add_argument("--sample_rate", type=int, default=30, help="Sample rate of the frames.")
    p.add_argument("--max_depth", type=float, default=10.0)
    p.add_argument("--min_depth", type=float, default=0.1)
    p.add_argument("--grid_size", type=float, default=0.01, help="Grid size for voxel downsampling.")
    p.add_argument("--n_outliers", type=int, default=10, help="Number of neighbors for outlier removal.")
    p.add_argument("--outlier_radius", type=float, default=0.05, help="Radius for outlier removal.")
    p.add_argument("--final_grid_size", type=float, default=0.01, help="Grid size for voxel downsampling.")
    p.add_argument("--final_n_outliers", type=int, default=10, help="Number of neighbors for outlier removal.")
    p.add_argument("--final_outlier_radius", type=float, default=0.05, help="Radius for outlier removal.")
    p.add_argument("--no_cleaning", action="store_true", help="Do not apply any outlier removal etc.")
    p.add_argument("--overwrite", action="store_true", help="Overwrite existing files.")
    return p


def default_args(**overrides):
    """the parser's defaults as a namespace (data_root: None), for callers that bring their own frames"""
    args = build_parser().parse_args(["--data_root", ""])
    args.data_root = None
    for key, value in overrides.items():
        if not hasattr(args, key):
            raise TypeError(f"default_args: no option {key!r}")
        setattr(args, key, value)
    return args


def process_frame(image, depth, camera_to_world, intrinsic, args):
    """process_dataset.py:102-134 for one decoded frame: backproject, remove_radius_outliers(n_outliers, outlier_radius) unless
    args.no_cleaning, voxel_down_sample(grid_size). -> xyz f32[m,3], rgb f32[m,3]"""
    xyz, rgb = backproject(image, depth, camera_to_world, intrinsic, min_depth=args.min_depth, max_depth=args.max_depth)
    if not args.no_cleaning and xyz.shape[0]:
        keep = remove_radius_outliers(xyz, args.n_outliers, args.outlier_radius)
        xyz, rgb = xyz[keep].contiguous(), rgb[keep].contiguous()
    return voxel_down_sample(xyz, args.grid_size, rgb)


def fuse_frames(frames, args, faro_xyz=None):
    """process_dataset.py:233-273. frames: an iterable of dicts {image u8[H,W,3], depth f32[H,W] (CUDA), camera_to_world 4x4,
    intrinsic 3x3}, already sampled. process_frame each, concatenate, voxel_down_sample(final_grid_size); unless
    args.no_cleaning: outlier_removal(final_n_outliers, final_outlier_radius, std_thresh=2.0), then filter_iphone_scan against
    faro_xyz f32[F,3] when one is given. -> xyz f32[m,3], rgb f32[m,3]"""
    parts = [process_frame(f["image"], f["depth"], f["camera_to_world"], f["intrinsic"], args) for f in frames]
    if not parts:
        raise ValueError("fuse_frames: no frames")
    xyz, rgb = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    xyz, rgb = voxel_down_sample(xyz, args.final_grid_size, rgb)
    if not args.no_cleaning:
        keep = outlier_removal(xyz, args.final_n_outliers, args.final_outlier_radius, std_thresh=2.0)
        xyz, rgb = xyz[keep].contiguous(), rgb[keep].contiguous()
        if faro_xyz is not None:
            keep = filter_iphone_scan(xyz, faro_xyz)
            xyz, rgb = xyz[keep].contiguous(), rgb[keep].contiguous()
    return xyz, rgb


# ---- files -----------------------------------------------------------------------------------------------------------
def write_ply(path, points, rgb=None):
    """binary little-endian PLY of float x y z + uchar red green blue, the layout of the reference's save_point_cloud
    (arkit_pcl.py:270-297; no colours: grey 128). evaluate_rooms.read_ply reads it back."""
    points = np.asarray(points.detach().cpu() if isinstance(points, torch.Tensor) else points, dtype=np.float32)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"write_ply: points must be [N,3], got {list(points.shape)}")
    if rgb is None:
        rgb = np.full((len(points), 3), 128, dtype=np.uint8)
    rgb = np.asarray(rgb.detach().cpu() if isinstance(rgb, torch.Tensor) else rgb)
    if rgb.shape != points.shape:
        raise ValueError(f"write_ply: rgb must be [N,3] like points, got {list(rgb.shape)}")
    if rgb.dtype != np.uint8:
        rgb = np.clip(rgb, 0, 255).astype(np.uint8)  # (truncated, as the reference's structured-array cast does)
    rec = np.empty(len(points), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    for i, a in enumerate("xyz"):
        rec[a] = points[:, i]
    for i, a in enumerate(("red", "green", "blue")):
        rec[a] = rgb[:, i]
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % len(points))
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())


def load_frames(scene_dir, sample_rate, device="cuda"):
    """the frames of <scene_dir>/iphone in the reference's layout: rgb/<frame_id>.png, depth/<frame_id>.png (uint16
    millimetres), pose_intrinsic_imu.json {frame_id: {aligned_pose, intrinsic}} with frame ids frame_%06d; every
    sample_rate-th of the sorted ids (process_dataset.py:226-231). The colour image is resized to the depth map (the
    reference's extract_rgb writes it at that size already). A generator: one frame on the device at a time."""
    from PIL import Image

    iphone = os.path.join(scene_dir, "iphone")
    with open(os.path.join(iphone, "pose_intrinsic_imu.json")) as f:
        meta = sorted(json.load(f).items())
    for frame_id, data in meta[::sample_rate]:
        depth = np.asarray(Image.open(os.path.join(iphone, "depth", frame_id + ".png")), dtype=np.float32) / 1000.0
        img = Image.open(os.path.join(iphone, "rgb", frame_id + ".png")).convert("RGB")
        if img.size != (depth.shape[1], depth.shape[0]):
            img = img.resize((depth.shape[1], depth.shape[0]))
        yield {"image": torch.from_numpy(np.ascontiguousarray(np.asarray(img, dtype=np.uint8))).to(device),
               "depth": torch.from_numpy(np.ascontiguousarray(depth)).to(device),
               "camera_to_world": np.array(data["aligned_pose"], dtype=np.float64).reshape(4, 4),
               "intrinsic": np.array(data["intrinsic"], dtype=np.float64).reshape(3, 3)}


def main(argv=None):
    from .evaluate_rooms import read_ply

    args = build_parser().parse_args(argv)
    scenes = sorted(s for s in os.listdir(args.data_root)
                    if os.path.exists(os.path.join(args.data_root, s, "scans", "mesh_aligned_0.05.ply")))
    per = int(math.ceil(len(scenes) / 10))  # (ten splits, process_dataset.py:198-201)
    if args.split is not None:
        scenes = scenes[args.split * per:(args.split + 1) * per]
    for scene in scenes:
        scene_dir = os.path.join(args.data_root, scene)
        target = os.path.join(scene_dir, "scans", f"{args.filename}.ply")
        if os.path.exists(target) and not args.overwrite:
            print("Skipping", scene)
            continue
        faro = None
        if not args.no_cleaning:
            faro = torch.from_numpy(read_ply(os.path.join(scene_dir, "scans", "mesh_aligned_0.05.ply"))["points"]).to("cuda", F32)
        xyz, rgb = fuse_frames(load_frames(scene_dir, args.sample_rate), args, faro_xyz=faro)
        write_ply(target, xyz, rgb)
        print("Saved point cloud with {} points to {}".format(xyz.shape[0], target))


if __name__ == "__main__":
    main()
