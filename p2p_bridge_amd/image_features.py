"""Image features onto a room scan: the per-point stages of the reference's data/processing/image_features.py
(`process_scene`, :329-514, driven by data/extract_image_features_snpp.py), which produce the `features` arrays that
denoise_room / room_data consume (`point_features="dino"`).

    project_point_cloud_batch   :114-143   fp64 projection of the scan into a batch of frames
    visible_points              :146-190   the occlusion test (with the projection in front of it)
    update_features             :223-279   sample the frames' feature maps, fp16 running mean per point
    sample_grid / update_features_from_grid  the same from the coarse DINO token grid, without the upsampled map (:110)
    interpolate_missing_features :282-326  unobserved points take the median of their filled / observed neighbours
    frame_stride                :411-427   every n-th frame
    fuse_scene                  :399-514   the driver (scene FILE reading stays with the caller), save_features :514

CUDA tensors run the HIP kernels of csrc/imgfeat.hip (and csrc/knn.hip for the neighbours); there is no fallback from them.
CPU tensors and numpy arrays take a torch / numpy path under the SAME arithmetic contract (include/p2pb_hip.h, "image
features"; the precedent is evaluation_metrics_fast.py) -- that path is what the CPU tests hold against the stored results of
the reference's own functions, and what `update_features_torch` offers as the operator-level yardstick on a GPU.

Deviations from the reference, all deliberate:
  * frame pairing: `update_features_batched_torch` zips the FLAT concatenation of the batch's sampled rows with the per-frame
    masks, so on its DINO path frame b receives row b of the concatenation, broadcast to all its points. Here frame b's rows go
    to frame b's points, as the function's docstring and the RGB path describe;
  * the reference's RGB branch calls a numpy function on CUDA tensors (:487-492) and cannot run; here "rgb" fuses the image
    itself as a 3-channel fp16 map;
  * the DINOv2 model is `dinov2.DinoV2` from a checkpoint file, or the caller's (`feature_fn`): torch.hub is a download;
  * COLMAP text, the pose JSON and the PNGs are read by the caller.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from ._lib import ask, call, ptr, stream_ptr
from .knn_grid import PointGrid

F16, F32, F64, I32, U8 = torch.float16, torch.float32, torch.float64, torch.int32, torch.uint8
KNN_WS_BYTES = 1 << 30  # scratch of one p2pb_knn_points launch: the missing points are taken in chunks of this size


def _tensor(x, name):
    if isinstance(x, np.ndarray):
        return torch.from_numpy(x)  # (shares memory: in-place updates reach the caller's array)
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor or a numpy array")
    return x


def _check(t, dtype, shape, name):
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must be {str(dtype).replace('torch.', '')}, got {str(t.dtype).replace('torch.', '')}")
    if t.dim() != len(shape) or any(s is not None and t.shape[i] != s for i, s in enumerate(shape)):
        raise ValueError(f"{name} must have shape {list('?' if s is None else s for s in shape)}, got {list(t.shape)}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous tensor")


def _one_device(name, *ts):
    devs = {t.device for t in ts}
    if len(devs) != 1:
        raise RuntimeError(f"{name}: all arguments must be on one device, got {sorted(str(d) for d in devs)}")
    return ts[0].device


def _back(t, like):
    return t.numpy() if isinstance(like, np.ndarray) else t


# ---- projection ------------------------------------------------------------------------------------------------------
def _rows3(m, x, y, z):
    """(m0*x + m1*y) + m2*z for the three rows of m [B,3,3]: the fixed order of the kernel, one rounding per operator"""
    return [(m[:, i, 0, None] * x + m[:, i, 1, None] * y) + m[:, i, 2, None] * z for i in range(3)]


def _project(points, rotation, translation, camera):
    p = points if points.dim() == 3 else points[None]
    cx, cy, cz = _rows3(rotation, p[..., 0], p[..., 1], p[..., 2])
    cx, cy, cz = cx + translation[:, 0, None], cy + translation[:, 1, None], cz + translation[:, 2, None]
    u, v, w = _rows3(camera, cx, cy, cz)
    return u / w, v / w, w


def project_point_cloud_batch(points, translation, rotation, camera_matrix):
    """points f64[N,3] or [B,N,3], translation f64[B,3] or [B,3,1], rotation f64[B,3,3], camera_matrix f64[B,3,3] ->
    f64[B,N,3] of (x, y, depth); argument order of the reference (:114-143). Arithmetic: fp64, `(r0*x + r1*y) + r2*z`, `+ t`,
    the same order for the camera matrix, IEEE divides -- the order `visible_points` uses inside its kernel (elementwise torch
    operators on whichever device holds the arguments; this helper is not on the hot path: the kernel projects itself)."""
    like = points
    points, translation = _tensor(points, "points"), _tensor(translation, "translation")
    rotation, camera_matrix = _tensor(rotation, "rotation"), _tensor(camera_matrix, "camera_matrix")
    _one_device("project_point_cloud_batch", points, translation, rotation, camera_matrix)
    if translation.dim() == 3:
        translation = translation[..., 0]
    b = rotation.shape[0] if rotation.dim() == 3 else None
    _check(rotation, F64, (None, 3, 3), "rotation"), _check(camera_matrix, F64, (b, 3, 3), "camera_matrix")
    _check(translation.contiguous(), F64, (b, 3), "translation")
    if points.dim() == 3:
        _check(points, F64, (b, None, 3), "points")
    else:
        _check(points, F64, (None, 3), "points")
    return _back(torch.stack(_project(points, rotation, translation, camera_matrix), -1), like)


# ---- visibility ------------------------------------------------------------------------------------------------------
def _visible_cpu(points, rotation, translation, camera, width, height, min_depth, max_depth):
    x, y, d = _project(points, rotation, translation, camera)
    # bounds in floating point before any conversion (the kernel's rule): trunc(x) in [0, W) <=> -1 < x < W
    inside = (x > -1.0) & (x < float(width)) & (y > -1.0) & (y < float(height)) & (d > min_depth) & (d < max_depth)
    minus = torch.full_like(x, -1.0)
    xy = torch.stack([torch.where(inside, x, minus), torch.where(inside, y, minus)], -1).to(I32)  # (.to: truncation)
    valid = torch.zeros_like(inside)
    for f in range(x.shape[0]):
        idx = torch.nonzero(inside[f]).flatten()  # ascending
        if idx.numel() == 0:
            continue
        pix = xy[f, idx, 1].long() * width + xy[f, idx, 0].long()
        ps, order = torch.sort(pix, stable=True)  # each pixel's points in ascending index
        ds = d[f, idx][order]
        run = ds.clone()  # -> inclusive running minimum inside each pixel's segment (log-step scan)
        longest = int(torch.unique_consecutive(ps, return_counts=True)[1].max())
        shift = 1
        while shift < longest:
            same = ps[shift:] == ps[:-shift]
            run = torch.cat([run[:shift], torch.where(same, torch.minimum(run[shift:], run[:-shift]), run[shift:])])
            shift *= 2
        before = torch.full_like(ds, math.inf)  # smallest depth of the EARLIER points of the pixel
        before[1:] = torch.where(ps[1:] == ps[:-1], run[:-1], before[1:])
        valid[f, idx[order]] = ds < before  # strict: an equal depth is rejected, the first point of a pixel is valid
    return valid, xy


def visible_points(points, rotation, translation, camera_matrix, width, height, min_depth=0.1, max_depth=1000.0):
    """Which points each frame sees: projection (:114-143) + occlusion filter (:146-190).
    points f64[N,3], rotation f64[B,3,3], translation f64[B,3], camera_matrix f64[B,3,3] -> (valid bool[B,N], xy i32[B,N,2]).
    A point is inside iff -1 < x < width, -1 < y < height and min_depth < depth < max_depth (all strict); its pixel is the
    coordinates truncated toward zero. valid = inside and depth strictly below the smallest depth of the earlier (lower-index)
    inside points of the same pixel: NOT a z-buffer, a later nearer point does not revoke an earlier farther one. xy holds the
    truncated pixel of every inside point and (-1, -1) elsewhere. Contract in full: include/p2pb_hip.h."""
    like = points
    points, rotation = _tensor(points, "points"), _tensor(rotation, "rotation")
    translation, camera_matrix = _tensor(translation, "translation"), _tensor(camera_matrix, "camera_matrix")
    dev = _one_device("visible_points", points, rotation, translation, camera_matrix)
    _check(points, F64, (None, 3), "points")
    _check(rotation, F64, (None, 3, 3), "rotation")
    b, n = rotation.shape[0], points.shape[0]
    _check(translation, F64, (b, 3), "translation"), _check(camera_matrix, F64, (b, 3, 3), "camera_matrix")
    width, height = int(width), int(height)
    if b < 1 or n < 1 or width < 1 or height < 1 or b > 65535 or b * n >= 2 ** 31 or width * height >= 2 ** 31:
        raise ValueError(f"visible_points: B={b}, N={n}, width={width}, height={height} out of range")
    if dev.type != "cuda":
        valid, xy = _visible_cpu(points, rotation, translation, camera_matrix, width, height, float(min_depth), float(max_depth))
        return _back(valid, like), _back(xy, like)
    valid = torch.empty(b, n, dtype=U8, device=dev)
    xy = torch.empty(b, n, 2, dtype=I32, device=dev)
    args = (b, n, width, height)
    ws = torch.empty(int(ask("p2pb_imgfeat_visibility_ws_bytes", *args)), dtype=U8, device=dev)
    call("p2pb_imgfeat_visibility", b, n, ptr(points), ptr(rotation), ptr(translation), ptr(camera_matrix), width, height,
         min_depth, max_depth, ptr(valid), ptr(xy), ptr(ws), stream_ptr())
    return valid.view(torch.bool), xy


# ---- fusion ----------------------------------------------------------------------------------------------------------
def update_features_torch(mean, count, maps, valid, xy):
    """`update_features` with torch operators on whichever device holds the tensors: one gather and three fp16 roundings per
    frame (d = f16(f32(new) - f32(mean)), q = f16(f32(d) / f32(count)), mean = f16(f32(mean) + f32(q))). The CPU path, and the
    operator-level yardstick of tools/bench_image_features.py."""
    hmap, wmap = maps.shape[1], maps.shape[2]
    for f in range(maps.shape[0]):
        idx = torch.nonzero(valid[f]).flatten()
        if idx.numel() == 0:
            continue
        x = xy[f, idx, 0].long().clamp(0, wmap - 1)
        y = xy[f, idx, 1].long().clamp(0, hmap - 1)
        new = maps[f, y, x].float()
        cnt = count[idx] + 1
        count[idx] = cnt
        m = mean[idx].float()
        d = (new - m).half()
        q = (d.float() / cnt.float()[:, None]).half()
        mean[idx] = (m + q.float()).half()
    return mean, count


def update_features(mean, count, maps, valid, xy):
    """Sample each frame's feature map at its valid points (:223-250) and fold the rows into the per-point running mean
    (:253-279), IN PLACE. mean f16[N,C], count i32[N], maps f16[B,Hmap,Wmap,C] channel-last, valid bool[B,N], xy i32[B,N,2]
    (from `visible_points`; the map may be larger or smaller than the mask: coordinates are clamped to it). Frames in order,
    frame b's rows to frame b's points; per valid point count += 1, mean += (new - mean) / count with every operator rounded to
    fp16 once from an fp32 evaluation. One launch for the whole batch on a GPU. -> (mean, count)"""
    out = (mean, count)
    mean, count, maps = _tensor(mean, "mean"), _tensor(count, "count"), _tensor(maps, "maps")
    valid, xy = _tensor(valid, "valid"), _tensor(xy, "xy")
    dev = _one_device("update_features", mean, count, maps, valid, xy)
    _check(mean, F16, (None, None), "mean")
    n, c = mean.shape
    _check(maps, F16, (None, None, None, c), "maps")
    b, hmap, wmap = maps.shape[:3]
    _check(count, I32, (n,), "count"), _check(valid, torch.bool, (b, n), "valid"), _check(xy, I32, (b, n, 2), "xy")
    if n < 1 or c < 1 or b < 1 or hmap < 1 or wmap < 1 or b * n >= 2 ** 31:
        raise ValueError(f"update_features: N={n}, C={c}, maps {list(maps.shape)} out of range")
    if dev.type != "cuda":
        update_features_torch(mean, count, maps, valid, xy)
        return out
    call("p2pb_imgfeat_fuse", b, n, c, hmap, wmap, ptr(maps), ptr(valid.view(U8)), ptr(xy), ptr(mean), ptr(count), stream_ptr())
    return out


# ---- fusion from the coarse grid -------------------------------------------------------------------------------------
def _lin_axis(dst, size_in, size_out):
    """the bilinear coordinates of one axis under the contract of include/p2pb_hip.h (p2pb_imgfeat_sample_grid): every
    operator one fp32 torch operation -> (i0, i1 int64, l0, l1 fp32)"""
    scale = torch.tensor(float(size_in), dtype=F32, device=dst.device) / torch.tensor(float(size_out), dtype=F32, device=dst.device)
    src = (((dst.to(F32) + 0.5) * scale) - 0.5).clamp_min(0.0)
    i0 = src.to(torch.int64).clamp_max(size_in - 1)  # (src >= 0: truncation is floor)
    i1 = (i0 + 1).clamp_max(size_in - 1)
    l1 = src - i0.to(F32)
    return i0, i1, 1.0 - l1, l1


def sample_grid_torch(grid, out_size, xy):
    """`sample_grid` with torch operators on whichever device holds the tensors (the CPU path and the operator-level yardstick)"""
    b, h, w, c = grid.shape
    out_h, out_w = int(out_size[0]), int(out_size[1])
    x = xy[..., 0].long().clamp(0, out_w - 1)
    y = xy[..., 1].long().clamp(0, out_h - 1)
    x0, x1, lx0, lx1 = _lin_axis(x, w, out_w)
    y0, y1, ly0, ly1 = _lin_axis(y, h, out_h)
    f = torch.arange(b, device=grid.device)[:, None]
    lx0, lx1, ly0, ly1 = lx0[..., None], lx1[..., None], ly0[..., None], ly1[..., None]
    top = lx0 * grid[f, y0, x0].float() + lx1 * grid[f, y0, x1].float()
    bot = lx0 * grid[f, y1, x0].float() + lx1 * grid[f, y1, x1].float()
    return (ly0 * top + ly1 * bot).half()


def _check_grid(name, grid, out_size, xy):
    _check(grid, F16, (None, None, None, None), "grid")
    b, h, w, c = grid.shape
    _check(xy, I32, (b, None, 2), "xy")
    n = xy.shape[1]
    out_h, out_w = int(out_size[0]), int(out_size[1])
    if min(b, h, w, c, n, out_h, out_w) < 1 or b * n >= 2 ** 31 or h * w >= 2 ** 30:
        raise ValueError(f"{name}: grid {list(grid.shape)}, out_size {(out_h, out_w)}, N={n} out of range")
    return b, h, w, c, n, out_h, out_w


def sample_grid(grid, out_size, xy):
    """The value that bilinear upsampling (align_corners=False) of the coarse grid f16[B,h,w,C] to out_size = (H, W) has at the
    pixels xy i32[B,N,2] (x, y; clamped to the map) -> f16[B,N,C], without building the map. Evaluated in fp32 from the fp16
    grid, rounded to fp16 once; per axis src = max((dst + 0.5) * (in / out) - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1, in - 1),
    l1 = src - i0, l0 = 1 - l1, value = ly0 * (lx0*a + lx1*b) + ly1 * (lx0*c + lx1*d) (contract: include/p2pb_hip.h). Within one
    fp16 ulp of F.interpolate(grid.float(), mode="bilinear").half() at those pixels."""
    like = grid
    grid, xy = _tensor(grid, "grid"), _tensor(xy, "xy")
    dev = _one_device("sample_grid", grid, xy)
    b, h, w, c, n, out_h, out_w = _check_grid("sample_grid", grid, out_size, xy)
    if dev.type != "cuda":
        return _back(sample_grid_torch(grid, (out_h, out_w), xy), like)
    out = torch.empty(b, n, c, dtype=F16, device=dev)
    call("p2pb_imgfeat_sample_grid", b, n, c, h, w, out_h, out_w, ptr(grid), ptr(xy), ptr(out),
         stream_ptr())
    return out


def update_features_from_grid_torch(mean, count, grid, out_size, valid, xy):
    """`update_features_from_grid` with torch operators: `sample_grid_torch` rows folded in like `update_features_torch`"""
    for f in range(grid.shape[0]):
        idx = torch.nonzero(valid[f]).flatten()
        if idx.numel() == 0:
            continue
        new = sample_grid_torch(grid[f:f + 1], out_size, xy[f:f + 1, idx])[0].float()
        cnt = count[idx] + 1
        count[idx] = cnt
        m = mean[idx].float()
        d = (new - m).half()
        q = (d.float() / cnt.float()[:, None]).half()
        mean[idx] = (m + q.float()).half()
    return mean, count


def update_features_from_grid(mean, count, grid, out_size, valid, xy):
    """`update_features` whose rows are `sample_grid(grid, out_size, xy)`: the running mean of the bilinearly upsampled map's
    pixels, IN PLACE, without the map. mean f16[N,C], count i32[N], grid f16[B,h,w,C] channel-last (the fp16 patch tokens),
    out_size = (H, W) of the map that is not built, valid bool[B,N], xy i32[B,N,2]. Frames in order; per valid point count += 1,
    mean += (new - mean) / count, every operator rounded to fp16 once from an fp32 evaluation. One launch for the whole batch on
    a GPU. -> (mean, count)"""
    out = (mean, count)
    mean, count, grid = _tensor(mean, "mean"), _tensor(count, "count"), _tensor(grid, "grid")
    valid, xy = _tensor(valid, "valid"), _tensor(xy, "xy")
    dev = _one_device("update_features_from_grid", mean, count, grid, valid, xy)
    b, h, w, c, n, out_h, out_w = _check_grid("update_features_from_grid", grid, out_size, xy)
    _check(mean, F16, (n, c), "mean"), _check(count, I32, (n,), "count"), _check(valid, torch.bool, (b, n), "valid")
    if dev.type != "cuda":
        update_features_from_grid_torch(mean, count, grid, (out_h, out_w), valid, xy)
        return out
    call("p2pb_imgfeat_fuse_grid", b, n, c, h, w, out_h, out_w, ptr(grid), ptr(valid.view(U8)),
         ptr(xy), ptr(mean), ptr(count), stream_ptr())
    return out


# ---- fill ------------------------------------------------------------------------------------------------------------
def _neighbours_cpu(points, missing, k):
    """the k nearest points of the cloud per missing point (fp64 distances of the fp32 coordinates, ties by ascending index)"""
    p = points.double().numpy()
    out = np.empty((len(missing), k), dtype=np.int64)
    step = max(1, (1 << 24) // len(p))
    for m0 in range(0, len(missing), step):
        q = p[missing[m0:m0 + step]]
        d2 = ((q[:, None, :] - p[None, :, :]) ** 2).sum(-1)
        part = np.argpartition(d2, k - 1, axis=1)[:, :k]
        kth = np.take_along_axis(d2, part, 1).max(1)
        for r in np.nonzero((d2 <= kth[:, None]).sum(1) > k)[0]:  # a tie across the k-th place: lowest indices first
            cand = np.nonzero(d2[r] <= kth[r])[0]
            part[r] = cand[np.lexsort((cand, d2[r, cand]))][:k]
        out[m0:m0 + step] = part
    return out


def _fill_cpu(feats, count, points, k):
    f, cnt = feats.numpy(), count.numpy()
    missing = np.nonzero(cnt == 0)[0]
    nbr = _neighbours_cpu(points, missing, k)
    for i, nb in zip(missing, nbr):  # ascending, in place: a filled point is seen by the later ones
        rows = f[nb[nb != i]].astype(np.float32)
        rows = rows[np.any(rows != 0, axis=1)]
        f[i] = np.median(rows, axis=0).astype(np.float16) if len(rows) else 0  # (two fp16 middles: their fp32 mean, one rounding)
    return 0


def _neighbours_hip(cloud, missing, k):
    """the exhaustive search of csrc/knn.hip, the missing points taken in chunks of KNN_WS_BYTES of scratch -> i32[m,k]"""
    n, m, dev = cloud.shape[1], missing.numel(), cloud.device
    nbr = torch.empty(m, k, dtype=I32, device=dev)
    step = max(1, min(m, KNN_WS_BYTES // (4 * n)))
    ws = torch.empty(int(ask("p2pb_knn_points_ws_bytes", 1, step, n)), dtype=U8, device=dev)
    for m0 in range(0, m, step):
        s = min(step, m - m0)
        query = cloud[0, missing[m0:m0 + s].long()].contiguous()
        call("p2pb_knn_points", 1, s, n, k, ptr(query), ptr(cloud),
             None, ptr(nbr[m0:m0 + s]), None, ptr(ws), stream_ptr())
    return nbr


def _fill_hip(feats, count, points, k, neighbours="brute"):
    n, c = feats.shape
    dev = feats.device
    missing = torch.nonzero(count == 0).flatten().to(I32)  # ascending
    m = missing.numel()
    if m == 0:
        return 0
    cloud = points.float().reshape(1, n, 3).contiguous()
    if neighbours == "grid":  # the same rows, bit for bit, from one ring search over the sorted cell-key grid
        nbr = PointGrid(cloud[0], k)._search(cloud[0, missing.long()].contiguous(), k)[1]
    else:
        nbr = _neighbours_hip(cloud, missing, k)
    done_round = torch.zeros(n, dtype=I32, device=dev)
    remaining = torch.zeros(1, dtype=I32, device=dev)
    remaining += m
    left, rounds = m, 0
    while left > 0:
        rounds += 1
        call("p2pb_imgfeat_fill_round", m, n, c, k, ptr(missing),
             ptr(nbr), ptr(count), ptr(feats), ptr(done_round), rounds, ptr(remaining), stream_ptr())
        now = int(remaining.item())
        if not 0 <= now < left:  # (the lowest unfinished point is always ready: every round finishes at least one)
            raise RuntimeError(f"interpolate_missing_features: round {rounds} left {now} of {left} points")
        left = now
    return rounds


def interpolate_missing_features(feats, count, points, k=10, return_rounds=False, neighbours="brute"):
    """Give every unobserved point (count == 0) the per-channel median of its neighbours (:282-326), IN PLACE.
    feats f16[N,C], count i32[N], points f32 or f64 [N,3] (neighbours are searched in fp32: csrc/knn.hip, ties by ascending
    index). The points are taken in ascending index; point i looks at its k nearest points of the whole cloud, keeps the rows
    that are not all-zero AT THAT MOMENT -- observed points, and unobserved points j < i with their filled rows -- and stores
    their median (mean of the two middle values for an even number, rounded to fp16 once), or zeros if none is left. On a GPU
    the in-place order runs as a wavefront of rounds (csrc/imgfeat.hip). Fewer than k points: ValueError.
    neighbours "grid" (opt-in, CUDA only): the same neighbour rows from knn_grid.PointGrid instead of the exhaustive search --
    the rounds are fed the same indices, so the result has the same bits. NaN or inf in points is then a ValueError.
    -> feats (with return_rounds: (feats, number of rounds; 0 on the CPU path))"""
    if neighbours not in ("brute", "grid"):
        raise ValueError(f"interpolate_missing_features: neighbours {neighbours!r} is neither 'brute' nor 'grid'")
    out = feats
    feats, count, points = _tensor(feats, "feats"), _tensor(count, "count"), _tensor(points, "points")
    dev = _one_device("interpolate_missing_features", feats, count, points)
    _check(feats, F16, (None, None), "feats")
    n, c = feats.shape
    _check(count, I32, (n,), "count")
    if points.dtype not in (F32, F64):
        raise RuntimeError("points must be float32 or float64")
    _check(points, points.dtype, (n, 3), "points")
    k = int(k)
    if not 1 <= k <= 32:
        raise ValueError(f"interpolate_missing_features: k={k} must be in [1, 32]")
    if n < k:
        raise ValueError(f"interpolate_missing_features: {n} points, fewer than k={k}")
    if c < 1:
        raise ValueError("interpolate_missing_features: feats has no channels")
    if dev.type == "cuda":
        rounds = _fill_hip(feats, count, points, k, neighbours)
    else:
        rounds = _fill_cpu(feats, count, points.float(), k)  # (its own exhaustive search: `neighbours` has nothing to choose)
    return (out, rounds) if return_rounds else out


# ---- driver ----------------------------------------------------------------------------------------------------------
def frame_stride(total, sampling_rate=5, autoskip=False):
    """every n-th frame of a scene with `total` frames (:411-427, including its final min(5, ...))"""
    if autoskip:
        skip = 1 if total < 25 else 5 if total < 50 else 10 if total < 100 else 20 if total < 500 else sampling_rate
    else:
        skip = sampling_rate
    return min(5, skip)


@torch.no_grad()
def fuse_scene(points, frames, feature_type="rgb", feature_fn=None, batch_size=2, mask_size=(192, 256),
               intrinsic_scale=256 / 1920, sampling_rate=5, autoskip=False, k=10, device=None, dino_from_grid=False,
               neighbours="brute"):
    """The per-scene loop of process_scene (:399-514) -> features f16[C,N'] (tensor on `device`), the transposed layout the
    data sets read; N' = the rows of `points` without NaN / inf (:403-405).
    points [N,3]; frames: a sequence of dicts {image f32[H,W,3] in [0,1], intrinsic 3x3 (full-resolution; rows 0-1 are scaled
    by intrinsic_scale, :466), world_to_camera 4x4}; every frame_stride(len(frames))-th is used, in batches of batch_size.
    mask_size = (height, width) of the occlusion mask. feature_type "rgb": the image itself as a 3-channel fp16 map;
    "dino": feature_fn(images f16[B,3,H,W]) -> f16[B,C,h,w] (DINOv2 patch tokens: `dinov2.feature_fn(model)`, or the caller's
    own model), upsampled to (H, W) with F.interpolate(mode="bilinear") as :110 does. dino_from_grid=True (opt-in) never builds
    that [B,H,W,C] map: the token grid is sampled at the points' pixels (`update_features_from_grid`; fp32 evaluation of the
    fp16 grid, within one fp16 ulp of the map's values, so the features differ from the default path's in the last place).
    device: default the device of `points` (cpu for numpy). neighbours: interpolate_missing_features' ("grid": opt-in)."""
    if neighbours not in ("brute", "grid"):
        raise ValueError(f"fuse_scene: neighbours {neighbours!r} is neither 'brute' nor 'grid'")
    if feature_type not in ("rgb", "dino"):
        raise ValueError(f"fuse_scene: feature_type {feature_type!r} is neither 'rgb' nor 'dino'")
    if feature_type == "dino" and feature_fn is None:
        raise ValueError("fuse_scene: feature_type 'dino' needs feature_fn (dinov2.feature_fn(model), or the caller's DINOv2 model)")
    points = torch.as_tensor(points)
    dev = torch.device(device) if device is not None else points.device
    points = points.to(dev, F64)
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"fuse_scene: points must be [N,3], got {list(points.shape)}")
    points = points[torch.isfinite(points).all(1)].contiguous()
    n = points.shape[0]
    frames = list(frames)
    frames = frames[::frame_stride(len(frames), sampling_rate, autoskip)]
    if not frames:
        raise ValueError("fuse_scene: no frames")
    height, width = int(mask_size[0]), int(mask_size[1])
    mean = count = None
    for batch in np.array_split(np.arange(len(frames)), int(math.ceil(len(frames) / batch_size))):
        fr = [frames[i] for i in batch]
        cam = np.stack([np.array(f["intrinsic"], dtype=np.float64) for f in fr])
        cam[:, :2, :] *= intrinsic_scale
        w2c = np.stack([np.asarray(f["world_to_camera"], dtype=np.float64) for f in fr])
        rot = torch.from_numpy(np.ascontiguousarray(w2c[:, :3, :3])).to(dev)
        trans = torch.from_numpy(np.ascontiguousarray(w2c[:, :3, 3])).to(dev)
        valid, xy = visible_points(points, rot, trans, torch.from_numpy(cam).to(dev), width, height)
        images = torch.stack([torch.as_tensor(f["image"], dtype=F32) for f in fr]).to(dev)  # [B,H,W,3]
        if feature_type == "dino" and dino_from_grid:
            grid = feature_fn(images.permute(0, 3, 1, 2).to(F16).contiguous()).permute(0, 2, 3, 1).to(F16).contiguous()
            if mean is None:
                mean = torch.zeros(n, grid.shape[-1], dtype=F16, device=dev)
                count = torch.zeros(n, dtype=I32, device=dev)
            update_features_from_grid(mean, count, grid, tuple(images.shape[1:3]), valid, xy)
            continue
        if feature_type == "rgb":
            maps = images.to(F16).contiguous()
        else:
            feat = feature_fn(images.permute(0, 3, 1, 2).to(F16).contiguous())
            feat = F.interpolate(feat, size=tuple(images.shape[1:3]), mode="bilinear", antialias=False)
            maps = feat.permute(0, 2, 3, 1).to(F16).contiguous()
        if mean is None:
            mean = torch.zeros(n, maps.shape[-1], dtype=F16, device=dev)
            count = torch.zeros(n, dtype=I32, device=dev)
        update_features(mean, count, maps, valid, xy)
    interpolate_missing_features(mean, count, points, k=k, neighbours=neighbours)
    return torch.nan_to_num(mean).t().contiguous()  # (:511-514)


def save_features(path, feats):
    """np.save of the transposed array f16[C,N] (:514; what room_data reads back)"""
    feats = feats.detach().cpu().numpy() if isinstance(feats, torch.Tensor) else np.asarray(feats)
    if feats.dtype != np.float16 or feats.ndim != 2:
        raise ValueError("save_features expects f16[C,N]")
    np.save(path, feats)
