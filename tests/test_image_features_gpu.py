"""csrc/imgfeat.hip through p2p_bridge_amd.image_features on the GPU: against the stored results of the reference's own functions
(tests/golden/image_features.npz, exact), against the package's CPU path on inputs whose arithmetic is exactly representable
(identity rotation, zero translation, K = [[8,0,4],[0,8,4],[0,0,1]], power-of-two depths: every projected coordinate is exact,
so equality is the only acceptable outcome), twice for bitwise repeatability, and inside a poisoned arena."""
import os

import numpy as np
import pytest
import torch

from oracle.poison_arena import PoisonArena

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "image_features.npz")
F16, F64, I32 = torch.float16, torch.float64, torch.int32
K8 = np.array([[8.0, 0.0, 4.0], [0.0, 8.0, 4.0], [0.0, 0.0, 1.0]])
W8 = H8 = 8


@pytest.fixture(scope="module")
def IF():
    from p2p_bridge_amd import image_features

    return image_features


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(GOLD))
    g["n"] = g["points"].shape[0]
    g["valid"] = np.unpackbits(g["valid"], axis=1)[:, :g["n"]].astype(bool)
    return g


def cuda(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy()


def run_gold(IF, gold):
    w, h = (int(v) for v in gold["size"])
    n, c, bs = gold["n"], gold["maps"].shape[-1], int(gold["batch"])
    pts = cuda(gold["points"], F64)
    mean, count = torch.zeros(n, c, dtype=F16, device="cuda"), torch.zeros(n, dtype=I32, device="cuda")
    valids = []
    for b0 in range(0, gold["maps"].shape[0], bs):
        sl = slice(b0, b0 + bs)
        valid, xy = IF.visible_points(pts, cuda(gold["rotation"][sl]), cuda(gold["translation"][sl]), cuda(gold["camera"][sl]), w, h)
        IF.update_features(mean, count, cuda(gold["maps"][sl]), valid, xy)
        valids.append(valid)
    filled = mean.clone()
    _, rounds = IF.interpolate_missing_features(filled, count, cuda(gold["points"]), return_rounds=True)
    return {"valid": torch.cat(valids).cpu().numpy(), "mean": mean.cpu().numpy(), "count": count.cpu().numpy(),
            "filled": filled.cpu().numpy(), "rounds": rounds}


@pytest.fixture(scope="module")
def hip_gold(IF, gold):
    return run_gold(IF, gold)


def test_golden_valid_mean_count_fill_exact(gold, hip_gold):
    assert np.array_equal(hip_gold["valid"], gold["valid"])
    assert np.array_equal(hip_gold["count"], gold["count"])
    assert np.array_equal(hip_gold["mean"].view(np.uint16), gold["mean"].view(np.uint16))
    assert np.array_equal(hip_gold["filled"].view(np.uint16), gold["filled"].view(np.uint16))
    assert hip_gold["rounds"] > 1
    assert np.array_equal(np.nan_to_num(hip_gold["filled"]).T.view(np.uint16), gold["final"].view(np.uint16))


def test_golden_run_twice_bitwise_identical(IF, gold, hip_gold):
    again = run_gold(IF, gold)
    for k in ("valid", "mean", "count", "filled"):
        assert np.array_equal(again[k].view(np.uint8), hip_gold[k].view(np.uint8)), k
    assert again["rounds"] == hip_gold["rounds"]


def test_driver_on_the_gpu(IF, gold):
    w, h = (int(v) for v in gold["size"])
    frames = []
    for f in range(gold["maps"].shape[0]):
        w2c = np.eye(4)
        w2c[:3, :3], w2c[:3, 3] = gold["rotation"][f], gold["translation"][f]
        frames.append({"image": np.full((h, w, 3), f / 8.0, dtype=np.float32), "intrinsic": gold["camera"][f], "world_to_camera": w2c})
    maps = cuda(gold["maps"])

    def feature_fn(images):
        first = int(round(float(images[0, 0, 0, 0]) * 8))
        return maps[first:first + images.shape[0]].permute(0, 3, 1, 2).contiguous()

    out = IF.fuse_scene(cuda(gold["points"]), frames, feature_type="dino", feature_fn=feature_fn, batch_size=2, mask_size=(h, w),
                        intrinsic_scale=1.0, sampling_rate=1)
    assert out.is_cuda and out.shape == gold["final"].shape
    assert np.array_equal(out.cpu().numpy().view(np.uint16), gold["final"].view(np.uint16))


# ---- visibility: exactly representable cases, HIP == CPU path == the stated expectation -------------------------------
def both(IF, points, b=1, width=W8, height=H8, trans=None, **kw):
    points = np.ascontiguousarray(points, dtype=np.float64)
    rot = np.repeat(np.eye(3)[None], b, 0)
    trans = np.zeros((b, 3)) if trans is None else np.asarray(trans, dtype=np.float64)
    cam = np.repeat(K8[None], b, 0)
    v0, xy0 = IF.visible_points(points, rot, trans, cam, width, height, **kw)
    v1, xy1 = IF.visible_points(cuda(points), cuda(rot), cuda(trans), cuda(cam), width, height, **kw)
    assert v1.dtype == torch.bool and xy1.dtype == I32 and v1.shape == v0.shape and xy1.shape == xy0.shape
    assert np.array_equal(v1.cpu().numpy(), v0)
    assert np.array_equal(xy1.cpu().numpy(), xy0)
    return v0, xy0


def test_equal_depth_is_rejected_and_a_later_nearer_point_revokes_nothing(IF):
    # x = 8 X / Z + 4: pixel (4, 4) for the first six points
    pts = [[0, 0, 2], [0.125, 0, 2], [0, 0, 4], [0, 0, 1], [0.0625, 0.0625, 1], [0, 0, 0.5], [-0.25, 0, 1]]
    v, xy = both(IF, pts)
    assert v[0].tolist() == [True, False, False, True, False, True, True]
    assert xy[0, :6].tolist() == [[4, 4]] * 6 and xy[0, 6].tolist() == [2, 4]
    v, _ = both(IF, [[0, 0, 4], [0, 0, 2]])  # farther first, nearer later: both records
    assert v[0].tolist() == [True, True]


def test_truncation_toward_zero_and_the_image_border(IF):
    # x = -0.5 (column 0), x = -1 (out), x = 8 = W (out), x = 7.5 (column 7); then the same four for y
    xs = [-1.125, -1.25, 1.0, 0.875]
    pts = [[x, 0, 2] for x in xs] + [[0, x, 2] for x in xs]
    v, xy = both(IF, pts)
    assert v[0].tolist() == [True, False, False, True] * 2
    assert xy[0].tolist() == [[0, 4], [-1, -1], [-1, -1], [7, 4], [4, 0], [-1, -1], [-1, -1], [4, 7]]


def test_depth_window_is_strict(IF):
    v, _ = both(IF, [[0, 0, 0.125], [0, 0, 0.25], [0, 0, 1024], [0, 0, 512]], min_depth=0.125, max_depth=1024.0)
    assert v[0].tolist() == [False, True, False, False]  # (512 lies behind 0.25 in the same pixel)
    v, _ = both(IF, [[0, 0, 1024], [0, 0, 512], [0, 0, 0.125]], min_depth=0.125, max_depth=1024.0)
    assert v[0].tolist() == [False, True, False]


def test_degenerate_coordinates_are_rejected_without_a_fault(IF):
    nan, inf = float("nan"), float("inf")
    pts = [[0, 0, 0], [1, 1, 0], [0, 0, -2], [1, 0, -2], [nan, 0, 2], [0, nan, 2], [0, 0, nan], [inf, 0, 2], [0, 0, inf],
           [-inf, -inf, 2], [1e300, 0, 2], [0, -1e300, 1e-300], [0, 0, 2]]
    v, xy = both(IF, pts)
    assert v[0].tolist() == [False] * 12 + [True]
    assert (xy[0, :12] == -1).all() and xy[0, 12].tolist() == [4, 4]


def test_one_pixel_holding_5000_points(IF):
    n = 5000
    z = 1.0 + np.arange(n) * 1e-3  # X = Y = 0: x = 4 Z / Z = 4 exactly, whatever the depth
    pts = np.zeros((n, 3))
    pts[:, 2] = z[::-1]
    v, xy = both(IF, pts)  # descending depths: every point is a record
    assert v.all() and (xy == 4).all()
    pts[:, 2] = z
    v, _ = both(IF, pts)  # ascending: only the first
    assert v[0, 0] and not v[0, 1:].any()
    rng = np.random.default_rng(5)
    pts[:, 2] = rng.uniform(1, 2, n)
    pts[::7, 2] = pts[3, 2]  # equal depths too
    v, _ = both(IF, pts)
    before = np.minimum.accumulate(np.concatenate([[np.inf], pts[:-1, 2]]))
    assert np.array_equal(v[0], pts[:, 2] < before) and 5 < v.sum() < 50


@pytest.mark.parametrize("n, b", [(1, 1), (65, 1), (65, 3), (6000, 2)])
def test_lattice_clouds_sizes_and_a_frame_that_sees_nothing(IF, n, b):
    """coordinates in eighths, depths 1 / 2 / 4: exact pixels, many equal depths, lists below and above one wave (6000 points on
    64 pixels); the last frame of a batch looks away (everything behind the camera)"""
    rng = np.random.default_rng(n + b)
    pts = np.stack([rng.integers(-16, 17, n) / 8.0, rng.integers(-16, 17, n) / 8.0, 2.0 ** rng.integers(0, 3, n)], 1)
    trans = np.zeros((b, 3))
    if b > 1:
        trans[-1, 2] = -64.0
        trans[0, 0] = 0.25
    v, xy = both(IF, pts, b=b, trans=trans)
    if b > 1:
        assert not v[-1].any() and (xy[-1] == -1).all()
    if n >= 65:
        assert v[0].any() and not v[0].all()
    v2, xy2 = both(IF, pts, b=b, trans=trans)
    assert np.array_equal(v, v2) and np.array_equal(xy, xy2)


# ---- fusion ----------------------------------------------------------------------------------------------------------
def fusion_case(seed, n, c, b, hmap, wmap):
    rng = np.random.default_rng(seed)
    valid = rng.random((b, n)) < 0.6
    xy = np.stack([rng.integers(0, 8, (b, n)), rng.integers(0, 8, (b, n))], -1).astype(np.int32)
    xy[~valid] = -1
    maps = rng.standard_normal((b, hmap, wmap, c)).astype(np.float16)
    mean = rng.standard_normal((n, c)).astype(np.float16)
    count = rng.integers(0, 4, n).astype(np.int32)
    mean[count == 0] = 0
    return mean, count, maps, valid, xy


@pytest.mark.parametrize("c", [3, 8, 384])
@pytest.mark.parametrize("hmap, wmap", [(8, 8), (5, 6)])
def test_fusion_matches_the_cpu_path_bit_for_bit(IF, c, hmap, wmap):
    """8 x 8 mask coordinates into an 8 x 8 map and into a smaller 5 x 6 one (clamping); n = 1001: no multiple of the points
    per workgroup for any c"""
    mean, count, maps, valid, xy = fusion_case(c, 1001, c, 5, hmap, wmap)
    m0, c0 = mean.copy(), count.copy()
    IF.update_features(m0, c0, maps, valid, xy)
    m1, c1 = cuda(mean), cuda(count)
    out = IF.update_features(m1, c1, cuda(maps), cuda(valid), cuda(xy))
    assert out[0] is m1 and out[1] is c1
    assert np.array_equal(c1.cpu().numpy(), c0) and np.array_equal(c0, count + valid.sum(0))
    assert np.array_equal(bits(m1), m0.view(np.int16))
    # five frames in one launch == five launches of one frame
    m2, c2 = cuda(mean), cuda(count)
    for f in range(5):
        IF.update_features(m2, c2, cuda(maps[f:f + 1]), cuda(valid[f:f + 1]), cuda(xy[f:f + 1]))
    assert np.array_equal(bits(m2), bits(m1)) and torch.equal(c2, c1)
    m3, c3 = cuda(mean), cuda(count)
    IF.update_features(m3, c3, cuda(maps), cuda(valid), cuda(xy))
    assert np.array_equal(bits(m3), bits(m1))  # run twice: the same bits


def test_fusion_wide_rows_and_unaligned_rows(IF):
    """c = 2056 (257 vectors: more than one step per thread) and c = 300 (scalar path, more channels than threads)"""
    for c in (2056, 300):
        mean, count, maps, valid, xy = fusion_case(c, 37, c, 3, 4, 4)
        m0, c0 = mean.copy(), count.copy()
        IF.update_features(m0, c0, maps, valid, xy)
        m1, c1 = cuda(mean), cuda(count)
        IF.update_features(m1, c1, cuda(maps), cuda(valid), cuda(xy))
        assert np.array_equal(bits(m1), m0.view(np.int16)) and np.array_equal(c1.cpu().numpy(), c0)


def test_fusion_divides_by_the_count_in_fp32(IF):
    m0 = np.array([[1.0, -3.0, 0.5, 7.0, 0.0, 2.0, -1.0, 9.0]], dtype=np.float16)
    new = np.array([2049.0, 1000.0, -2047.0, 3.0, 5.0, -4096.0, 33.0, 0.25], dtype=np.float16)
    mean, count = cuda(m0), cuda(np.array([2048], dtype=np.int32))
    IF.update_features(mean, count, cuda(new.reshape(1, 1, 1, 8)), torch.ones(1, 1, dtype=torch.bool, device="cuda"),
                       torch.zeros(1, 1, 2, dtype=I32, device="cuda"))
    d = (new.astype(np.float32) - m0[0].astype(np.float32)).astype(np.float16)
    q = (d.astype(np.float32) / np.float32(2049)).astype(np.float16)
    want = (m0[0].astype(np.float32) + q.astype(np.float32)).astype(np.float16)
    assert not np.array_equal(q, (d.astype(np.float32) / np.float32(2048)).astype(np.float16))
    assert count.item() == 2049 and np.array_equal(bits(mean)[0], want.view(np.int16))


# ---- fill ------------------------------------------------------------------------------------------------------------
def fill_both(IF, feats, count, points, k):
    f0 = feats.copy()
    IF.interpolate_missing_features(f0, count, points, k=k)
    f1 = cuda(feats)
    out, rounds = IF.interpolate_missing_features(f1, cuda(count), cuda(points), k=k, return_rounds=True)
    assert out is f1 and np.array_equal(bits(f1), f0.view(np.int16))
    f2 = cuda(feats)
    IF.interpolate_missing_features(f2, cuda(count), cuda(points), k=k)
    assert np.array_equal(bits(f2), bits(f1))
    return f0, rounds


def test_fill_cluster_without_observed_neighbours_stays_zero(IF):
    rng = np.random.default_rng(1)
    near = rng.uniform(0, 1, (200, 3)).astype(np.float32)
    far = (rng.uniform(0, 0.1, (12, 3)) + 50.0).astype(np.float32)  # 12 unobserved points, 10 neighbours: all inside the cluster
    points = np.concatenate([near[:100], far, near[100:]])
    count = np.ones(212, dtype=np.int32)
    count[100:112] = 0
    count[::9] = 0
    count[100:112] = 0
    feats = rng.standard_normal((212, 5)).astype(np.float16)
    feats[count == 0] = 0
    out, rounds = fill_both(IF, feats, count, points, 10)
    assert not out[100:112].any() and out[count == 0].any() and rounds >= 1
    assert np.array_equal(out[count > 0], feats[count > 0])  # observed rows are never written


def test_fill_chain_of_dependent_points_takes_many_rounds(IF):
    """points on a line with growing gaps, k = 4 (itself, both sides and the second to the left), only the first two observed:
    point i waits for point i - 1"""
    n = 40
    points = np.zeros((n, 3), dtype=np.float32)
    points[:, 0] = np.arange(n) * 1.0 + np.arange(n) ** 2 * 1e-3  # (growing gaps: no equal distances)
    count = np.zeros(n, dtype=np.int32)
    count[:2] = 1
    feats = np.zeros((n, 70), dtype=np.float16)
    feats[:2] = np.random.default_rng(2).standard_normal((2, 70)).astype(np.float16)
    out, rounds = fill_both(IF, feats, count, points, 4)
    assert rounds == n - 2
    assert np.array_equal(out[2], ((feats[0].astype(np.float32) + feats[1].astype(np.float32)) / 2).astype(np.float16))
    mid = ((feats[1].astype(np.float32) + out[2].astype(np.float32)) / 2).astype(np.float16)
    assert np.array_equal(out[3], mid) and out[-1].any()


@pytest.mark.parametrize("c, k", [(384, 10), (3, 20), (65, 1)])
def test_fill_random_cloud_against_the_cpu_path(IF, c, k):
    """even and odd numbers of contributing rows, observed rows that are all-zero (dropped), -0.0 rows, k above 16"""
    rng = np.random.default_rng(c)
    n = 700
    points = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    count = (rng.random(n) < 0.4).astype(np.int32) * rng.integers(1, 5, n).astype(np.int32)
    feats = rng.standard_normal((n, c)).astype(np.float16)
    feats[count == 0] = 0
    seen = np.nonzero(count)[0]
    feats[seen[::5]] = 0
    feats[seen[1::10]] = np.float16(-0.0)
    _, rounds = fill_both(IF, feats, count, points, k)
    assert rounds > 1 or k == 1


# ---- memory discipline -----------------------------------------------------------------------------------------------
def test_wrappers_hold_to_their_buffers(IF, gold):
    w, h = (int(v) for v in gold["size"])
    n = 999
    pts64 = gold["points"][:n].astype(np.float64)
    v0, xy0 = IF.visible_points(pts64, gold["rotation"][:2].copy(), gold["translation"][:2].copy(), gold["camera"][:2].copy(), w, h)
    m0, c0 = np.zeros((n, 8), dtype=np.float16), np.zeros(n, dtype=np.int32)
    IF.update_features(m0, c0, gold["maps"][:2].copy(), v0, xy0)
    f0 = m0.copy()
    IF.interpolate_missing_features(f0, c0, gold["points"][:n].copy())
    with PoisonArena("cuda", 64 << 20) as arena:
        put = lambda a: arena.put(torch.from_numpy(np.ascontiguousarray(a)))  # noqa: E731
        before = arena.n_allocations
        valid, xy = IF.visible_points(put(pts64), put(gold["rotation"][:2]), put(gold["translation"][:2]), put(gold["camera"][:2]), w, h)
        arena.check_guards()
        assert arena.n_allocations >= before + 3  # valid, xy and the workspace came out of the arena
        assert np.array_equal(valid.cpu().numpy(), v0) and np.array_equal(xy.cpu().numpy(), xy0)  # (unwritten: 0xFF / -1)
        mean, count = put(np.zeros((n, 8), dtype=np.float16)), put(np.zeros(n, dtype=np.int32))
        IF.update_features(mean, count, put(gold["maps"][:2]), valid, xy)
        arena.check_guards()
        arena.assert_written(mean, "mean")
        assert np.array_equal(bits(mean), m0.view(np.int16)) and np.array_equal(count.cpu().numpy(), c0)
        before = arena.n_allocations
        IF.interpolate_missing_features(mean, count, put(gold["points"][:n]))
        arena.check_guards()
        arena.assert_written(mean, "filled")
        assert arena.n_allocations >= before + 4  # neighbours, knn scratch, done_round, remaining
        assert np.array_equal(bits(mean), f0.view(np.int16))


def test_cuda_and_cpu_tensors_do_not_mix(IF):
    pts, eye = torch.zeros(20, 3, dtype=F64, device="cuda"), torch.eye(3, dtype=F64)[None].contiguous()
    with pytest.raises(RuntimeError):
        IF.visible_points(pts, eye, torch.zeros(1, 3, dtype=F64), eye, 8, 8)
    with pytest.raises(RuntimeError):
        IF.update_features(torch.zeros(20, 4, dtype=F16, device="cuda"), torch.zeros(20, dtype=I32), torch.zeros(1, 8, 8, 4, dtype=F16),
                           torch.zeros(1, 20, dtype=torch.bool), torch.zeros(1, 20, 2, dtype=I32))
