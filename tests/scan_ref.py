"""An independent CPU restatement of p2p_bridge_amd.scan_fusion for the tests (a plain helper module, not a conftest):
numpy fp64 for back-projection and voxel means, scipy.spatial.cKDTree on the fp64 points for counts and k-th distances, and
the margin rules under which keep / drop decisions are compared (tests/test_scan_fusion_gpu.py)."""
import numpy as np
from scipy.spatial import cKDTree

REL = 1e-6  # relative margin of a decision: sqdist3 on fp32 inputs errs by ~4 * 2^-24 in d^2, ~2e-7 in d
MAX_LEFT_OUT = 1e-3  # at most this share of the points may fall inside a margin


def room(n, seed, ext=(1.0, 0.8, 0.6)):
    """a box room: points on the six faces with 4 mm noise, the first 5 % uniform clutter in the box scaled 1.5x; fp32"""
    rng = np.random.default_rng(seed)
    ext = np.asarray(ext, dtype=np.float64)
    p = rng.uniform(0.0, 1.0, (n, 3)) * ext
    axis, side = rng.integers(0, 3, n), rng.integers(0, 2, n)
    p[np.arange(n), axis] = side * ext[axis]
    p += rng.normal(0.0, 0.004, (n, 3))
    m = int(0.05 * n)
    p[:m] = ext / 2 + (rng.uniform(0.0, 1.0, (m, 3)) - 0.5) * 1.5 * ext
    return p.astype(np.float32)


def backproject(image, depth, camera_to_world, intrinsic, min_depth=0.1, max_depth=10.0, intrinsic_scale=256 / 1920):
    """-> xyz f64[n,3] (not rounded), rgb f64[n,3], the valid pixels in row-major order"""
    k = np.array(intrinsic, dtype=np.float64)
    k[0, 0] *= intrinsic_scale
    k[1, 1] *= intrinsic_scale
    k[0, 2] *= intrinsic_scale
    k[1, 2] *= intrinsic_scale
    yy, xx = np.meshgrid(np.arange(depth.shape[0]), np.arange(depth.shape[1]), indexing="ij")
    xx, yy = xx.reshape(-1), yy.reshape(-1)
    z = depth[yy, xx]
    with np.errstate(invalid="ignore"):
        valid = np.logical_not((z < np.float32(min_depth)) | (z > np.float32(max_depth)) | np.isnan(z) | np.isinf(z))
    x, y = xx[valid], yy[valid]
    uv1 = np.stack([x, y, np.ones_like(x)], 0).astype(np.float64)
    cam = (np.linalg.inv(k) @ uv1) * z[valid].astype(np.float64)
    world = np.asarray(camera_to_world, dtype=np.float64) @ np.concatenate([cam, np.ones_like(cam[:1])], 0)
    return world[:3].T, image[y, x].astype(np.float64)


def voxel_means(xyz, voxel_size, *attrs):
    """-> keys i64[m,3] ascending by (kx, ky, kz), [fp64 means of xyz and of every attribute]"""
    keys = np.floor(xyz.astype(np.float32) / np.float32(voxel_size)).astype(np.int64)  # the fp32 divide
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    sk = keys[order]
    first = np.concatenate([[True], np.any(sk[1:] != sk[:-1], axis=1)])
    seg = np.cumsum(first) - 1
    m = seg[-1] + 1
    cnt = np.bincount(seg, minlength=m).astype(np.float64)
    means = []
    for a in (xyz,) + attrs:
        a64 = a.astype(np.float64)[order]
        means.append(np.stack([np.bincount(seg, weights=a64[:, c], minlength=m) for c in range(a.shape[1])], 1) / cnt[:, None])
    return sk[first], means


def within_ulps(got32, want64, ulps=1):
    """|got - want| <= ulps * ulp(fp32(want)), elementwise"""
    got32 = np.asarray(got32)
    assert got32.dtype == np.float32
    w32 = np.asarray(want64, dtype=np.float64).astype(np.float32)
    return np.abs(got32.astype(np.float64) - want64) <= ulps * np.spacing(np.maximum(np.abs(w32), np.float32(1e-30))).astype(np.float64)


def radius_decisions(xyz, nb_points, r, include_self=True):
    """-> (keep bool[n], sure bool[n]): sure where the fp64 decision is the same at r (1 - REL) and r (1 + REL)"""
    p = xyz.astype(np.float64)
    tree = cKDTree(p)
    need = nb_points + (0 if include_self else 1)
    lo = tree.query_ball_point(p, r * (1 - REL), return_length=True) >= need
    hi = tree.query_ball_point(p, r * (1 + REL), return_length=True) >= need
    return lo, lo == hi


def kth_distance(query, ref, k, workers=1):
    """fp64 distance to the k-th nearest point of ref (the query itself included when it is among ref)"""
    d = cKDTree(ref.astype(np.float64)).query(query.astype(np.float64), k=[k], workers=workers)[0]
    return d[:, 0]


def threshold_decisions(kth, lower, upper):
    """-> (keep, sure) for lower < kth < upper (None: no bound); sure where kth is further than REL from either bound"""
    keep, sure = np.ones(len(kth), dtype=bool), np.ones(len(kth), dtype=bool)
    for bound, sign in ((lower, 1), (upper, -1)):
        if bound is not None:
            keep &= (kth - bound) * sign > 0
            sure &= np.abs(kth - bound) > REL * abs(bound)
    return keep, sure


def std_band(kth, t_low, t_high):
    mean, std = kth.mean(), kth.std()
    return (None if t_low is None else mean - t_low * std), mean + t_high * std


def compare_masks(got, keep, sure):
    """the decisions agree wherever the restatement is sure, and it is sure nearly everywhere"""
    left_out = int((~sure).sum())
    assert left_out <= MAX_LEFT_OUT * len(sure), f"{left_out} of {len(sure)} points lie in the margin"
    wrong = np.nonzero((got != keep) & sure)[0]
    assert wrong.size == 0, f"{wrong.size} decisions differ, first at {wrong[:5]}"
    return left_out
