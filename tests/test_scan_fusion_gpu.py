"""Scan fusion on the GPU against the CPU restatement of tests/scan_ref.py (numpy fp64, scipy cKDTree).
Tolerances: back-projection and voxel means 1 fp32 ulp against the fp64 result (double rounding); counts, keys, order exact;
k-th distances 1e-6 relative (sqdist3 errs by ~4 * 2^-24 in d^2); keep / drop decisions under the margin rule of scan_ref."""
import numpy as np
import pytest
import torch

import scan_ref
from oracle.poison_arena import PoisonArena
from p2p_bridge_amd import scan_fusion as SF

pytestmark = pytest.mark.gpu
KTH_REL = 1e-6


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared reference arrays are read-only)


def host(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def rooms():
    """the test clouds and their fp64 k-th distances, computed once and never written to"""
    out = {}
    for n, seed in ((20000, 0), (20000, 1), (3000, 2)):
        pts = scan_ref.room(n, seed)
        faro = scan_ref.room(n // 2, seed + 100)
        entry = {"pts": pts, "faro": faro, "kth": {k: scan_ref.kth_distance(pts, pts, k) for k in (10, 20, 64)},
                 "nn_faro": scan_ref.kth_distance(pts, faro, 1)}
        for a in [pts, faro, entry["nn_faro"]] + list(entry["kth"].values()):
            a.setflags(write=False)
        out[(n, seed)] = entry
    return out


# ---- back-projection -------------------------------------------------------------------------------------------------
def test_backproject_exact_case():
    k = np.array([[8.0, 0, 4], [0, 8, 4], [0, 0, 1]])
    depth = (2.0 ** np.random.default_rng(0).integers(-2, 3, (8, 8))).astype(np.float32)
    image = np.random.default_rng(1).integers(0, 256, (8, 8, 3)).astype(np.uint8)
    xyz, rgb = SF.backproject(dev(image), dev(depth), np.eye(4), k, intrinsic_scale=1)
    want, want_rgb = scan_ref.backproject(image, depth, np.eye(4), k, intrinsic_scale=1)
    assert xyz.dtype == torch.float32 and rgb.dtype == torch.float32 and xyz.shape == (64, 3)
    assert np.array_equal(host(xyz).astype(np.float64), want)  # powers of two: every operation is exact
    assert np.array_equal(host(rgb).astype(np.float64), want_rgb)
    yy, xx = np.divmod(np.arange(64), 8)
    assert np.array_equal(want[:, 0], (xx - 4) / 8 * depth.reshape(-1)) and np.array_equal(want[:, 2], depth.reshape(-1))


def _pose(seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    pose = np.eye(4)
    pose[:3, :3], pose[:3, 3] = q, rng.uniform(-3, 3, 3)
    return pose


def test_backproject_random_frame_against_fp64():
    rng = np.random.default_rng(2)
    depth = rng.uniform(0.05, 6.0, (192, 256)).astype(np.float32)
    image = rng.integers(0, 256, (192, 256, 3)).astype(np.uint8)
    k = np.array([[1450.0, 0, 958.3], [0, 1452.5, 721.9], [0, 0, 1]])
    pose = _pose(3)
    xyz, rgb = SF.backproject(dev(image), dev(depth), pose, k, min_depth=0.1, max_depth=5.0)
    want, want_rgb = scan_ref.backproject(image, depth, pose, k, min_depth=0.1, max_depth=5.0)
    assert 0 < len(want) < depth.size and tuple(xyz.shape) == want.shape  # count exact
    assert scan_ref.within_ulps(host(xyz), want, 1).all()
    assert np.array_equal(host(rgb).astype(np.float64), want_rgb)  # order exact
    again = SF.backproject(dev(image), dev(depth), torch.from_numpy(pose), torch.from_numpy(k), min_depth=0.1, max_depth=5.0)
    assert torch.equal(again[0], xyz) and torch.equal(again[1], rgb)


def test_backproject_validity_bounds():
    lo, hi = np.float32(0.1), np.float32(10.0)
    vals = np.array([lo, hi, np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(20)), 0.0, -1.0, np.nan, np.inf,
                     -np.inf, 1.0, 5.0, 0.5], dtype=np.float32)
    depth = vals.reshape(3, 4)
    image = np.arange(36, dtype=np.uint8).reshape(3, 4, 3)
    k = np.array([[30.0, 0, 15], [0, 30, 11], [0, 0, 1]])
    xyz, rgb = SF.backproject(dev(image), dev(depth), _pose(5), k)
    want, want_rgb = scan_ref.backproject(image, depth, _pose(5), k)
    kept = [0, 1, 9, 10, 11]  # the two bounds themselves and the ordinary depths
    assert np.array_equal(want_rgb, image.reshape(-1, 3)[kept].astype(np.float64))
    assert np.array_equal(host(rgb).astype(np.float64), want_rgb) and scan_ref.within_ulps(host(xyz), want, 1).all()


def test_backproject_all_invalid_frame():
    depth = np.full((5, 7), np.nan, dtype=np.float32)
    depth[0, :3] = [0.0, 50.0, -2.0]
    xyz, rgb = SF.backproject(dev(np.zeros((5, 7, 3), np.uint8)), dev(depth), np.eye(4), np.eye(3))
    assert tuple(xyz.shape) == (0, 3) and tuple(rgb.shape) == (0, 3) and xyz.is_cuda and xyz.dtype == torch.float32


# ---- voxels ----------------------------------------------------------------------------------------------------------
def _check_voxels(pts, size, *attrs):
    got = SF.voxel_down_sample(dev(pts), size, *[dev(a) for a in attrs])
    keys, means = scan_ref.voxel_means(pts, size, *attrs)
    assert isinstance(got, tuple) and len(got) == 1 + len(attrs)
    for g, w in zip(got, means):
        assert tuple(g.shape) == w.shape, (tuple(g.shape), w.shape)  # row count exact
        assert scan_ref.within_ulps(host(g), w, 1).all()
    # order exact: the key of each output row (its mean lies inside its voxel, or on its rounding edge) is ascending
    packed = (keys[:, 0] * (1 << 42)) + (keys[:, 1] * (1 << 21)) + keys[:, 2]
    assert np.all(np.diff(packed) > 0)
    return got, keys


def test_voxel_single_point_and_single_voxel():
    (xyz,), keys = _check_voxels(np.array([[0.3, -0.2, 0.9]], np.float32), 0.05)
    assert tuple(xyz.shape) == (1, 3)
    rng = np.random.default_rng(0)
    pts = (0.5 + rng.uniform(0, 0.01, (5000, 3)) * [1, 1, 1]).astype(np.float32)  # 5000 points in one voxel: two chunks
    feats = rng.normal(size=(5000, 35)).astype(np.float32)
    got, keys = _check_voxels(pts, 0.05, feats)
    assert len(keys) == 1 and tuple(got[1].shape) == (1, 35)


@pytest.mark.parametrize("size", [0.05, 0.01])
def test_voxel_room(rooms, size):
    pts = rooms[(20000, 0)]["pts"]
    rng = np.random.default_rng(7)
    rgb, feats = rng.uniform(0, 255, (20000, 3)).astype(np.float32), rng.normal(size=(20000, 35)).astype(np.float32)
    got, keys = _check_voxels(pts, size, rgb, feats)
    counts = np.unique(np.floor(pts / np.float32(size)).astype(np.int64), axis=0, return_counts=True)[1]
    assert len(keys) == len(counts) == {0.05: 3637, 0.01: 17706}[size]  # up to 25 points each; mostly single
    assert (counts.max() == 25 if size == 0.05 else np.median(counts) == 1)
    again = SF.voxel_down_sample(dev(pts), size, dev(rgb), dev(feats))
    assert all(torch.equal(a, b) for a, b in zip(got, again))  # identical bits


def test_voxel_mixed_occupancy_and_negative_coordinates():
    """one voxel above the small / large threshold next to thousands of single ones, on both sides of the origin"""
    rng = np.random.default_rng(1)
    pts = np.concatenate([rng.uniform(-1, 1, (3000, 3)), -0.52 + rng.uniform(0, 0.01, (9000, 3)),
                          0.31 + rng.uniform(0, 0.01, (65, 3)), 0.71 + rng.uniform(0, 0.01, (64, 3))]).astype(np.float32)
    pts = pts[rng.permutation(len(pts))]
    got, keys = _check_voxels(pts, 0.02, rng.normal(size=(len(pts), 3)).astype(np.float32))
    assert keys[:, 0].min() < 0 < keys[:, 0].max()


def test_voxel_faces_and_floor():
    g = np.arange(-8, 9, dtype=np.float32) / 16  # exactly on the faces of 2^-4 voxels
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    (xyz,), keys = _check_voxels(pts, 2.0 ** -4)
    assert len(keys) == 17 ** 3 and np.array_equal(host(xyz), pts)  # every point its own voxel, in key order = grid order
    (xyz,), keys = _check_voxels(np.array([[-0.001, 0.0, 0.05], [-0.002, 0.001, 0.051]], np.float32), 0.05)
    assert np.array_equal(keys, [[-1, 0, 1]])


def test_voxel_key_out_of_range_raises():
    pts = np.zeros((10, 3), np.float32)
    pts[3, 1] = 0.01 * (1 << 20) * 1.01
    with pytest.raises(ValueError):
        SF.voxel_down_sample(dev(pts), 0.01)
    pts[3, 1] = np.nan
    with pytest.raises(ValueError):
        SF.voxel_down_sample(dev(pts), 0.01)
    pts[3, 1] = -0.01 * (1 << 20) * 0.99  # inside
    assert SF.voxel_down_sample(dev(pts), 0.01)[0].shape[0] == 2


# ---- radius mask -----------------------------------------------------------------------------------------------------
def test_radius_lattice_ties_and_self_count():
    g = np.arange(6, dtype=np.float32) * 0.25
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    inner = np.all((pts > 0.1) & (pts < 1.2), axis=1)
    assert np.array_equal(host(SF.remove_radius_outliers(dev(pts), 7, 0.25)), inner)  # <= and the self count
    assert np.array_equal(host(SF.remove_radius_outliers(dev(pts), 6, 0.25, include_self=False)), inner)
    assert not host(SF.remove_radius_outliers(dev(pts), 7, 0.25, include_self=False)).any()
    assert host(SF.remove_radius_outliers(dev(pts), 4, 0.25)).all()  # a corner: itself and three


@pytest.mark.parametrize("r,nb", [(0.05, 30), (0.05, 10), (0.02, 5)])
@pytest.mark.parametrize("which", [(20000, 0), (20000, 1), (3000, 2)])
def test_radius_rooms(rooms, which, r, nb):
    pts = rooms[which]["pts"]
    got = host(SF.remove_radius_outliers(dev(pts), nb, r))
    keep, sure = scan_ref.radius_decisions(pts, nb, r)
    scan_ref.compare_masks(got, keep, sure)
    if which[0] == 20000:  # (the sparse small room keeps nothing at the tight settings: still compared)
        assert 0.5 * len(got) < got.sum() < len(got)


def test_radius_far_clusters_coincident_and_small_clouds():
    rng = np.random.default_rng(3)
    a = rng.normal(0, 0.02, (1000, 3))
    pts = np.concatenate([a, a[::-1] * 1.1 + [100.0, 0, 0]]).astype(np.float32)  # 10^11 cells of 0.02 m between them
    got = host(SF.remove_radius_outliers(dev(pts), 8, 0.02))
    scan_ref.compare_masks(got, *scan_ref.radius_decisions(pts, 8, 0.02))
    assert 0 < got.sum() < 2000
    same = np.tile(np.array([[0.3, -1.2, 2.5]], np.float32), (5000, 1))
    assert host(SF.remove_radius_outliers(dev(same), 10, 0.05)).all()
    few = rng.normal(0, 0.001, (5, 3)).astype(np.float32)
    assert not host(SF.remove_radius_outliers(dev(few), 6, 0.05)).any()  # n < nb
    assert host(SF.remove_radius_outliers(dev(few), 5, 0.05)).all()
    one = dev(np.array([[1.0, 2.0, 3.0]], np.float32))
    assert host(SF.remove_radius_outliers(one, 1, 0.05)).tolist() == [True]
    assert host(SF.remove_radius_outliers(one, 2, 0.05)).tolist() == [False]
    assert host(SF.remove_radius_outliers(one, 1, 0.05, include_self=False)).tolist() == [False]


# ---- k-th distance ---------------------------------------------------------------------------------------------------
def _check_kth(query, ref, k, want=None):
    q = dev(query)
    got = host(SF.knn_kth_distance(q, q if ref is query else dev(ref), k))
    want = scan_ref.kth_distance(query, ref, k) if want is None else want
    assert got.dtype == np.float32 and got.shape == want.shape
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err <= KTH_REL * want), (err.max(), np.argmax(err - KTH_REL * want))
    return got


@pytest.mark.parametrize("k", [10, 20, 64])
@pytest.mark.parametrize("which", [(20000, 0), (20000, 1), (3000, 2)])
def test_kth_rooms(rooms, which, k):
    r = rooms[which]
    _check_kth(r["pts"], r["pts"], k, want=r["kth"][k])


def test_kth_self_query_at_k1_is_zero(rooms):
    pts = dev(rooms[(3000, 2)]["pts"])
    assert not host(SF.knn_kth_distance(pts, pts, 1)).any()
    assert not host(SF.knn_kth_distance(pts, pts.clone(), 1)).any()


def test_kth_lone_point_and_outside_queries(rooms):
    rng = np.random.default_rng(4)
    cluster = rng.normal(0, 0.01, (30, 3))
    pts = np.concatenate([cluster, [[2.5, 0.0, 0.0]]]).astype(np.float32)  # the lone point: far more than 50 cell edges away
    got = _check_kth(pts, pts, 20)
    assert got[-1] > 2.4
    ref = rooms[(3000, 2)]["pts"]
    query = np.concatenate([ref[:500], ref[:300] + np.float32([40.0, -7.0, 3.0]), ref[:5] * np.float32(1e6)]).astype(np.float32)
    _check_kth(query, ref, 1)
    _check_kth(query, ref, 7)


def test_kth_coarser_grids_before_the_brute_force_pass(rooms, monkeypatch):
    """the queries the first grid leaves go to grids four times coarser when there are too many for the brute-force pass;
    forced here at a small size, the result must not change by a bit"""
    ref = rooms[(3000, 2)]["pts"]
    query = np.concatenate([ref, ref[:300] + np.float32([1.5, -0.7, 0.3]), ref[:5] * np.float32(1e6)]).astype(np.float32)
    q, r = dev(query), dev(ref)
    usual = SF.knn_kth_distance(q, r, 20)
    monkeypatch.setattr(SF, "KNN_BRUTE_PAIRS", 0)
    assert torch.equal(SF.knn_kth_distance(q, r, 20), usual)
    monkeypatch.setattr(SF, "KNN_LEVELS", 1)  # and with no grid but the first
    assert torch.equal(SF.knn_kth_distance(q, r, 20), usual)
    want = scan_ref.kth_distance(query, ref, 20)
    assert np.all(np.abs(host(usual).astype(np.float64) - want) <= KTH_REL * want)


def test_kth_nearest_of_another_cloud(rooms):
    r = rooms[(20000, 1)]
    _check_kth(r["pts"], r["faro"], 1, want=r["nn_faro"])


def test_kth_duplicates_and_limits():
    rng = np.random.default_rng(5)
    base = rng.uniform(0, 1, (400, 3)).astype(np.float32)
    pts = np.concatenate([base, base, base[:100], np.tile(base[:1], (3000, 1))])  # every point at least twice, one 3002 times
    got = _check_kth(pts, pts, 2)
    assert not got.any()
    _check_kth(pts, pts, 3)
    _check_kth(pts, pts, 64)
    few = dev(base[:19])
    with pytest.raises(ValueError):
        SF.knn_kth_distance(few, few, 20)
    with pytest.raises(ValueError):
        SF.knn_kth_distance(few, few, 65)
    _check_kth(base[:19], base[:19], 19)
    assert SF.knn_kth_distance(few[:0], few, 3).shape == (0,)


def test_far_from_the_origin(rooms):
    """half a kilometre out an fp32 quotient p / cell carries an error of a good fraction of a percent of a cell: the cells a
    query visits and the distance it may trust allow for that, the results stay exact"""
    pts = (rooms[(3000, 2)]["pts"] * np.float32(4.0) + np.float32([500.0, -300.0, 40.0])).astype(np.float32)
    _check_kth(pts, pts, 20)
    _check_kth(pts[:1000], pts[1000:], 1)
    for r, nb in ((0.2, 10), (0.08, 5)):
        got = host(SF.remove_radius_outliers(dev(pts), nb, r))
        scan_ref.compare_masks(got, *scan_ref.radius_decisions(pts, nb, r))
        assert 0 < got.sum() < len(got)
    _check_voxels(pts, 0.04, rooms[(3000, 2)]["pts"])


# ---- filters ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [(20000, 0), (20000, 1), (3000, 2)])
def test_outlier_removal_masks(rooms, which):
    r = rooms[which]
    pts = dev(r["pts"])
    kth20 = r["kth"][20]
    lower, upper = scan_ref.std_band(kth20, 2.0, 2.0)
    want = scan_ref.threshold_decisions(kth20, lower, upper)
    got = host(SF.outlier_removal(pts, 10, 0.05, std_thresh=2.0))
    scan_ref.compare_masks(got, *want)
    assert 0.9 < got.mean() < 1.0
    # the k = 20 override: nb_points and radius play no part once std_thresh is given
    assert np.array_equal(host(SF.outlier_removal(pts, 3, 123.0, std_thresh=2.0)), got)
    # without it: k = nb_points against the radius
    radius = float(np.median(r["kth"][10]))
    got10 = host(SF.outlier_removal(pts, 10, radius))
    scan_ref.compare_masks(got10, *scan_ref.threshold_decisions(r["kth"][10], None, float(np.float32(radius))))
    assert 0 < got10.sum() < len(got10) and not np.array_equal(got10, got)


@pytest.mark.parametrize("which", [(20000, 0), (20000, 1), (3000, 2)])
def test_filter_iphone_scan_mask(rooms, which):
    r = rooms[which]
    _, upper = scan_ref.std_band(r["nn_faro"], None, 1.0)
    got = host(SF.filter_iphone_scan(dev(r["pts"]), dev(r["faro"])))
    scan_ref.compare_masks(got, *scan_ref.threshold_decisions(r["nn_faro"], None, upper))
    assert 0.9 < got.mean() < 1.0


# ---- pipeline --------------------------------------------------------------------------------------------------------
BOX = np.array([4.0, 3.0, 2.5])


@pytest.fixture(scope="module")
def frames():
    """six 48 x 64 depth frames of an analytic box room: ray-plane intersection from known poses"""
    scale = 256 / 1920
    k_small = np.array([[40.0, 0, 31.5], [0, 40.0, 23.5], [0, 0, 1]])
    k_full = k_small.copy()
    k_full[:2] /= scale
    yy, xx = np.meshgrid(np.arange(48), np.arange(64), indexing="ij")
    rays = np.linalg.inv(k_small) @ np.stack([xx.ravel(), yy.ravel(), np.ones(48 * 64)]).astype(np.float64)  # z component 1
    rng = np.random.default_rng(11)
    out = []
    for f in range(6):
        a = f * np.pi / 3 + 0.2
        fwd, up = np.array([np.cos(a), np.sin(a), 0.1 * (f % 3 - 1)]), np.array([0.0, 0.0, 1.0])
        fwd /= np.linalg.norm(fwd)
        right = np.cross(fwd, up)
        right /= np.linalg.norm(right)
        pose = np.eye(4)
        pose[:3, :3] = np.stack([right, np.cross(fwd, right), fwd], 1)
        pose[:3, 3] = BOX / 2 + rng.uniform(-0.4, 0.4, 3)
        d = pose[:3, :3] @ rays
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.concatenate([(0.0 - pose[:3, 3, None]) / d, (BOX[:, None] - pose[:3, 3, None]) / d])
        t[~(t > 0)] = np.inf
        depth = t.min(0).reshape(48, 64).astype(np.float32)  # the ray parameter is the z depth: the rays have z = 1
        depth[rng.uniform(size=depth.shape) < 0.02] = 0.0  # holes
        spikes = rng.uniform(size=depth.shape) < 0.01
        depth[spikes] *= rng.uniform(0.3, 0.8, spikes.sum()).astype(np.float32)  # flying pixels
        image = rng.integers(0, 256, (48, 64, 3)).astype(np.uint8)
        out.append({"image": dev(image), "depth": dev(depth), "camera_to_world": pose, "intrinsic": k_full})
    faro = scan_ref.room(6000, 9, ext=tuple(BOX))[300:]  # the faces without the clutter
    return out, dev(faro)


def _args(**kw):
    base = dict(max_depth=8.0, grid_size=0.05, n_outliers=5, outlier_radius=0.3, final_grid_size=0.08)
    base.update(kw)
    return SF.default_args(**base)


def test_fuse_frames_is_the_composition_of_the_stages(frames):
    fr, faro = frames
    args = _args()
    xyz, rgb = SF.fuse_frames(fr, args, faro_xyz=faro)
    parts, dropped = [], 0
    for f in fr:
        p, c = SF.backproject(f["image"], f["depth"], f["camera_to_world"], f["intrinsic"], min_depth=0.1, max_depth=8.0)
        assert 0.9 * 48 * 64 < p.shape[0] < 48 * 64
        inside = ((p > -0.01) & (p < torch.tensor(BOX + 0.01, dtype=torch.float32, device="cuda"))).all(1)
        assert inside.all()  # the poses and the geometry are right: every point lies in the box
        keep = SF.remove_radius_outliers(p, 5, 0.3)
        dropped += int((~keep).sum())
        one = SF.process_frame(f["image"], f["depth"], f["camera_to_world"], f["intrinsic"], args)
        want = SF.voxel_down_sample(p[keep].contiguous(), 0.05, c[keep].contiguous())
        assert torch.equal(one[0], want[0]) and torch.equal(one[1], want[1])
        parts.append(want)
    assert dropped > 0
    p, c = SF.voxel_down_sample(torch.cat([q[0] for q in parts]), 0.08, torch.cat([q[1] for q in parts]))
    keep = SF.outlier_removal(p, args.final_n_outliers, args.final_outlier_radius, std_thresh=2.0)
    p, c = p[keep].contiguous(), c[keep].contiguous()
    keep2 = SF.filter_iphone_scan(p, faro)
    assert 0 < int((~keep).sum()) and 0 < int((~keep2).sum())
    assert torch.equal(xyz, p[keep2]) and torch.equal(rgb, c[keep2])  # bit for bit
    again = SF.fuse_frames(fr, args, faro_xyz=faro)
    assert torch.equal(again[0], xyz) and torch.equal(again[1], rgb)  # two runs are identical
    no_faro = SF.fuse_frames(fr, args)
    assert torch.equal(no_faro[0], p) and torch.equal(no_faro[1], c)


def test_no_cleaning_skips_exactly_the_three_filters(frames):
    fr, faro = frames
    xyz, rgb = SF.fuse_frames(fr, _args(no_cleaning=True), faro_xyz=faro)
    parts = []
    for f in fr:
        p, c = SF.backproject(f["image"], f["depth"], f["camera_to_world"], f["intrinsic"], min_depth=0.1, max_depth=8.0)
        parts.append(SF.voxel_down_sample(p, 0.05, c))
    p, c = SF.voxel_down_sample(torch.cat([q[0] for q in parts]), 0.08, torch.cat([q[1] for q in parts]))
    assert torch.equal(xyz, p) and torch.equal(rgb, c)
    assert xyz.shape[0] > SF.fuse_frames(fr, _args(), faro_xyz=faro)[0].shape[0]


# ---- memory and CPU tensors ------------------------------------------------------------------------------------------
def test_wrappers_hold_to_their_buffers(rooms, frames):
    pts = rooms[(3000, 2)]["pts"][:2999]
    faro = rooms[(3000, 2)]["faro"][:1499]
    heavy = np.concatenate([pts, np.tile(pts[:1], (4500, 1))])  # one voxel / cell of 4501 points: the chunked sums
    feats = np.random.default_rng(0).normal(size=(len(heavy), 35)).astype(np.float32)
    f = frames[0][0]
    image, depth = host(f["image"])[:47, :63].copy(), host(f["depth"])[:47, :63].copy()
    want = {
        "bp": SF.backproject(dev(image), dev(depth), f["camera_to_world"], f["intrinsic"]),
        "vox": SF.voxel_down_sample(dev(heavy), 0.03, dev(feats)),
        "rad": SF.remove_radius_outliers(dev(heavy), 10, 0.05),
        "kth": SF.knn_kth_distance(dev(heavy), dev(heavy), 20),
        "out": SF.outlier_removal(dev(pts), 10, 0.05, std_thresh=2.0),
        "far": SF.filter_iphone_scan(dev(pts), dev(faro)),
    }
    with PoisonArena("cuda", 96 << 20) as arena:
        put = lambda a: arena.put(torch.from_numpy(np.array(a)))  # noqa: E731  (a copy: the shared arrays are read-only)
        before = arena.n_allocations
        got = SF.backproject(put(image), put(depth), f["camera_to_world"], f["intrinsic"])
        arena.check_guards()
        assert arena.n_allocations >= before + 5  # the two inputs, the mask, xyz and rgb
        arena.assert_written(got[0], "xyz"), arena.assert_written(got[1], "rgb")
        assert torch.equal(got[0], want["bp"][0]) and torch.equal(got[1], want["bp"][1])
        before = arena.n_allocations
        got = SF.voxel_down_sample(put(heavy), 0.03, put(feats))
        arena.check_guards()
        assert arena.n_allocations >= before + 7  # inputs, keys, flag, starts, chunk table, outputs, partial sums
        arena.assert_written(got[0], "voxel xyz"), arena.assert_written(got[1], "voxel feats")
        assert torch.equal(got[0], want["vox"][0]) and torch.equal(got[1], want["vox"][1])
        h = put(heavy)
        got = SF.remove_radius_outliers(h, 10, 0.05)
        arena.check_guards()
        assert torch.equal(got, want["rad"])
        got = SF.knn_kth_distance(h, h, 20)
        arena.check_guards()
        arena.assert_written(got, "kth")
        assert torch.equal(got, want["kth"])
        p = put(pts)
        got = SF.outlier_removal(p, 10, 0.05, std_thresh=2.0)
        arena.check_guards()
        assert torch.equal(got, want["out"])
        got = SF.filter_iphone_scan(p, put(faro))
        arena.check_guards()
        assert torch.equal(got, want["far"])


def test_cpu_tensors_raise_and_devices_do_not_mix():
    x = torch.zeros(30, 3)
    for fn in (lambda: SF.voxel_down_sample(x, 0.1), lambda: SF.voxel_down_sample(x.cuda(), 0.1, torch.zeros(30, 2)),
               lambda: SF.remove_radius_outliers(x, 3, 0.1), lambda: SF.knn_kth_distance(x.cuda(), x, 2),
               lambda: SF.knn_kth_distance(x, x.cuda(), 2), lambda: SF.filter_iphone_scan(x.cuda(), x),
               lambda: SF.backproject(torch.zeros(4, 4, 3, dtype=torch.uint8).cuda(), torch.ones(4, 4), np.eye(4), np.eye(3))):
        with pytest.raises(RuntimeError):
            fn()
