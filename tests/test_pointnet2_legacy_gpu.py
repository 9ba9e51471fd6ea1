"""The nine classic PointNet++ operators of `pointnet2_batch_cuda` (csrc/ball_query.hip, csrc/three_nn.hip, csrc/fps_ref.hip and the grouping / gather
entry points they share with the PVCNN operators) against brute-force references written here in numpy.

EXACT family: coordinates k/8 with integer k in [-8, 8], so every difference, square and three-term sum is exact in fp32 and
a squared distance is (sum of integer squares) / 64. The references work on the integers and apply the tie rules of
include/p2pb_hip.h; results must be bit-identical, nothing is excluded. 1000 points on 17^3 lattice sites: duplicates, equal
distances and pairs exactly on the radius (at radius 0.5: integer differences with sum of squares 16) are common.
Features, gradients and gradient targets are integers in [-8, 8], weights j/16: every sum is exact in any order.

FLOAT family: uniform fp32 clouds in [-1, 1]^3 (rng.uniform(-1, 1, (1000, 3)) then (257, 3), cast to fp32) against float64.
MARGIN = 4e-6 absolute on squared distances: the fp32 rounding of fma(dz,dz, fma(dy,dy, dx*dx)) at this extent is below
3e-6 (three differences of magnitude <= 2 rounded to 2^-24 relative, squares <= 4, sum <= 12: < 3 * 2 * 2 * 2^-23 +
3 * 12 * 2^-24). Each test first asserts that ITS float64 reference is decided by more than the margin (or counts what is
not), then requires exact indices.
"""
import functools
import sys

import numpy as np
import pytest
import torch

from oracle.poison_arena import PoisonArena

pytestmark = pytest.mark.gpu

B, N, M = 2, 1000, 257
MARGIN = 4e-6
F32, I32 = torch.float32, torch.int32

# the 21 names third_party/openpoints/cpp/pointnet2_batch/src/pointnet2_api.cpp exports
REFERENCE_NAMES = [
    "ball_query_wrapper", "group_points_wrapper", "group_points_grad_wrapper", "gather_points_wrapper",
    "gather_points_grad_wrapper", "furthest_point_sampling_wrapper", "three_nn_wrapper", "three_interpolate_wrapper",
    "three_interpolate_grad_wrapper", "avg_voxelize_backward", "avg_voxelize_forward", "trilinear_devoxelize_forward",
    "trilinear_devoxelize_backward", "ball_query", "three_nearest_neighbors_interpolate_forward",
    "three_nearest_neighbors_interpolate_backward", "grouping_forward", "grouping_backward", "gather_features_forward",
    "gather_features_backward", "furthest_point_sampling_forward",
]


@pytest.fixture(scope="module")
def ext():
    from p2p_bridge_amd import pointnet2_batch_cuda

    return pointnet2_batch_cuda


@pytest.fixture(scope="module")
def ops():
    from p2p_bridge_amd import pointnet2_ops

    return pointnet2_ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = got.view(np.int32) != want.view(np.int32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {tuple(np.argwhere(bad)[0])}"


def cm(t):
    """[B, N, K] -> channel-major [B, K, N], contiguous: the layout of the PVCNN operators"""
    return t.transpose(1, 2).contiguous()


# ---- the exact family ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lattice(n, seed=0, b=B):
    """integer coordinates i64[b, n, 3] in [-8, 8]; the cloud is lattice / 8"""
    return np.random.default_rng(1000 + seed).integers(-8, 9, (b, n, 3))


@functools.lru_cache(maxsize=None)
def main_case():
    """(points i64[B,N,3], centres i64[B,M,3]) of the main case, from one generator"""
    rng = np.random.default_rng(7)
    return rng.integers(-8, 9, (B, N, 3)), rng.integers(-8, 9, (B, M, 3))


def cloud(k):
    return (k / 8.0).astype(np.float32)


def d2_int(a, b):
    """sum of squared integer differences i64[len(a), len(b)] = 64 * the squared distance"""
    d = a[:, None, :] - b[None, :, :]
    return (d * d).sum(-1)


def ball_query_ref(d2, thr, nsample, fill):
    """d2[m, n] (any exact dtype), strict d2 < thr: first nsample hits in ascending k, padded with the first hit; a row
    without a hit keeps `fill`"""
    out = np.full((d2.shape[0], nsample), fill, np.int32)
    for j in range(d2.shape[0]):
        hits = np.flatnonzero(d2[j] < thr)
        if hits.size:
            out[j] = hits[0]
            out[j, :min(hits.size, nsample)] = hits[:nsample]
    return out


def three_nn_ref(d2):
    """d2[n, m] -> (three smallest values, their indices): ascending distance, lower index first among equals; unfilled
    slots (m < 3) are (+inf, 0)"""
    n, m = d2.shape
    order = np.argsort(d2, axis=1, kind="stable")[:, :3]
    idx = np.zeros((n, 3), np.int32)
    val = np.full((n, 3), np.inf)
    idx[:, :min(m, 3)] = order
    val[:, :min(m, 3)] = np.take_along_axis(d2, order, 1)
    return val, idx


def fps_ref(xyz, m, temp0=1e10):
    """xyz f64[n,3] -> (idx i32[m], temp f64[n], smallest gap between the two largest running minima over the rounds).
    Maximum in the order (temp desc, k mod T asc, k asc), T = min(2^floor(log2 n), 1024)."""
    n = xyz.shape[0]
    T = min(1 << (n.bit_length() - 1), 1024)
    k = np.arange(n)
    temp = np.full(n, float(np.float32(temp0)))
    idx = np.zeros(m, np.int32)
    gap = np.inf
    for j in range(1, m):
        d = xyz - xyz[idx[j - 1]]
        temp = np.minimum(temp, (d * d).sum(1))
        top = np.flatnonzero(temp == temp.max())
        idx[j] = top[np.lexsort((top, top % T))[0]]
        if n > 1:
            two = np.partition(temp, n - 2)[n - 2:]
            gap = min(gap, two[1] - two[0])
    return idx, temp, gap


def run_fps(ext, xyz32, m, temp_fill=1e10):
    b, n, _ = xyz32.shape
    temp = torch.full((b, n), temp_fill, dtype=F32, device="cuda")
    idx = torch.full((b, max(m, 0)), -7, dtype=I32, device="cuda")
    assert ext.furthest_point_sampling_wrapper(b, n, m, dev(xyz32), temp, idx) == 1
    return idx, temp


# T = 512 at 1000 (the main case), 1024 at 1024, the modulus wraps at 2500, 20000 takes the large-cloud path; 1, 2, 3, 37, 100:
# T below the wave / workgroup sizes; 1500, 5000, 16000: the other points-per-thread forms, 16000 without the LDS copy
@pytest.mark.parametrize("n", [1, 2, 3, 37, 100, 1000, 1024, 1500, 2500, 5000, 16000, 20000])
def test_fps_exact(ext, n):
    k = main_case()[0] if n == N else lattice(n)
    m = min(n, 128)
    idx, temp = run_fps(ext, cloud(k), m)
    for b in range(B):
        ridx, rtemp, _ = fps_ref(k[b] / 8.0, m)
        same_bits(idx[b], ridx, f"fps idx, n = {n}, cloud {b}")
        same_bits(temp[b], rtemp.astype(np.float32), f"fps temp, n = {n}, cloud {b}")


def test_fps_ties_are_common_in_the_exact_fixture():
    """the exact clouds must exercise the tie order: in some round several points share the maximum"""
    k = main_case()[0][0] / 8.0
    temp = np.full(N, 1e10)
    tied, last = 0, 0
    for _ in range(1, 128):
        temp = np.minimum(temp, ((k - k[last]) ** 2).sum(1))
        top = np.flatnonzero(temp == temp.max())
        tied += top.size > 1
        last = top[np.lexsort((top, top % 512))[0]]
    assert tied >= 10, tied


@pytest.mark.parametrize("n", [37, 1000, 20000])
def test_fps_m_zero_and_one(ext, n):
    """m = 0 writes nothing; m = 1 writes idx 0 and leaves temp as it was (no round ran)"""
    k = lattice(n)
    idx, temp = run_fps(ext, cloud(k), 0, temp_fill=3.5)
    assert idx.numel() == 0 and bool((temp == 3.5).all())
    idx, temp = run_fps(ext, cloud(k), 1, temp_fill=3.5)
    assert bool((idx == 0).all()) and bool((temp == 3.5).all())


@pytest.mark.parametrize("radius", [0.25, 0.5])
@pytest.mark.parametrize("nsample", [1, 16, 64])
def test_ball_query_exact(ext, nsample, radius):
    pts, ctr = main_case()
    thr = int(round(64 * radius * radius))  # 4 or 16: d2 < r^2 on the integers
    idx = torch.full((B, M, nsample), -7, dtype=I32, device="cuda")
    assert ext.ball_query_wrapper(B, N, M, radius, nsample, dev(cloud(ctr)), dev(cloud(pts)), idx) == 1
    on_radius = untouched = padded = truncated = 0
    for b in range(B):
        d2 = d2_int(ctr[b], pts[b])
        ref = ball_query_ref(d2, thr, nsample, -7)
        same_bits(idx[b], ref, f"ball query idx, cloud {b}")
        cnt = (d2 < thr).sum(1)
        on_radius += int((d2 == thr).sum())
        untouched += int((cnt == 0).sum())
        padded += int(((cnt > 0) & (cnt < nsample)).sum())
        truncated += int((cnt > nsample).sum())
    # the fixture must not pass vacuously
    assert on_radius > 0
    if radius == 0.25:
        assert untouched > 0
    if nsample == 64 or (nsample == 16 and radius == 0.25):
        assert padded > 0
    if nsample < 64 and radius == 0.5:
        assert truncated > 0


def test_ball_query_exact_many_centres(ext):
    """B * M >= 2048 centres: the cloud is staged in LDS and shared by the workgroup's waves (below: scanned from global memory)"""
    m, nsample = 1100, 16
    pts, ctr = main_case()[0], lattice(m, seed=3)
    for radius, thr in ((0.25, 4), (0.5, 16)):
        idx = torch.full((B, m, nsample), -7, dtype=I32, device="cuda")
        ext.ball_query_wrapper(B, N, m, radius, nsample, dev(cloud(ctr)), dev(cloud(pts)), idx)
        for b in range(B):
            same_bits(idx[b], ball_query_ref(d2_int(ctr[b], pts[b]), thr, nsample, -7), f"ball query idx, r = {radius}, cloud {b}")


def test_ball_query_exact_cloud_beyond_lds(ext):
    """13000 points: the cloud does not fit the LDS planes"""
    n, m, nsample = 13000, 64, 64
    pts, ctr = lattice(n, seed=1), lattice(m, seed=3)
    idx = torch.full((B, m, nsample), -7, dtype=I32, device="cuda")
    ext.ball_query_wrapper(B, n, m, 0.25, nsample, dev(cloud(ctr)), dev(cloud(pts)), idx)
    for b in range(B):
        same_bits(idx[b], ball_query_ref(d2_int(ctr[b], pts[b]), 4, nsample, -7), f"ball query idx, cloud {b}")


# One scan serves both layouts (csrc/ball_query.hip): global memory (B * m < 2048), the cloud in LDS, a cloud beyond the LDS bound
BALL_QUERY_ARMS = {
    "global": lambda: main_case(),
    "lds": lambda: (main_case()[0], lattice(1100, seed=3)),
    "beyond_lds": lambda: (lattice(13000, seed=1), lattice(64, seed=3)),  # 3 * 13000 * 4 B = 156 000 > 147 456
}


@pytest.mark.parametrize("radius", [0.25, 0.5])
@pytest.mark.parametrize("arm", list(BALL_QUERY_ARMS))
def test_ball_query_layouts_agree(ext, arm, radius):
    """the channel-major operator on the transposed clouds and the point-major one give the same bits on every row with a
    hit; without one the first writes zeros and the second leaves the caller's row (-7 here)"""
    pts, ctr = BALL_QUERY_ARMS[arm]()
    n, m, nsample = pts.shape[1], ctr.shape[1], 16
    xyz, new_xyz = dev(cloud(pts)), dev(cloud(ctr))
    pv = ext.ball_query(cm(new_xyz), cm(xyz), radius, nsample).cpu().numpy()
    idx = torch.full((B, m, nsample), -7, dtype=I32, device="cuda")
    assert ext.ball_query_wrapper(B, n, m, radius, nsample, new_xyz, xyz, idx) == 1
    pn = idx.cpu().numpy()
    thr = int(round(64 * radius * radius))
    hit = np.stack([(d2_int(ctr[b], pts[b]) < thr).any(1) for b in range(B)])
    same_bits(torch.from_numpy(pv[hit]), pn[hit], f"ball query, {arm}, r = {radius}: rows with a hit")
    assert (pv[~hit] == 0).all() and (pn[~hit] == -7).all()
    # the small clouds leave centres alone at the small radius (13000 points cover the neighbourhood of every lattice site)
    if radius == 0.25 and arm != "beyond_lds":
        assert (~hit).sum() > 0


# m = 1, 2: unfilled slots; 257: the main case; 2500: more than one LDS tile of known points
@pytest.mark.parametrize("m", [1, 2, 3, 257, 2500])
def test_three_nn_exact(ext, m):
    unknown = main_case()[0]
    known = lattice(m, seed=2) if m > M else main_case()[1][:, :m]
    dist2 = torch.empty(B, N, 3, dtype=F32, device="cuda")
    idx = torch.empty(B, N, 3, dtype=I32, device="cuda")
    assert ext.three_nn_wrapper(B, N, m, dev(cloud(unknown)), dev(cloud(known)), dist2, idx) is None
    ties = 0
    for b in range(B):
        d2 = d2_int(unknown[b], known[b])
        val, ref = three_nn_ref(d2)
        same_bits(idx[b], ref, f"three_nn idx, m = {m}, cloud {b}")
        same_bits(dist2[b], (val / 64.0).astype(np.float32), f"three_nn dist2, m = {m}, cloud {b}")
        if m >= 4:
            s = np.sort(d2, axis=1)[:, :4]
            ties += int((np.diff(s, axis=1) == 0).any(1).sum())
    if m < 3:
        assert bool(torch.isinf(dist2[:, :, m:]).all()) and bool((idx[:, :, m:] == 0).all())
    if m >= 4:
        assert ties > 0  # equal distances among the nearest four: the tie rule decides


def nn3_weights_ref(dist2):
    """nn3_store_weights (csrc/three_nn.hip) in numpy float32, one IEEE operation each: dist2 f32[B,N,3] -> w f32[B,3,N]"""
    d = np.maximum(np.minimum(np.float32(1e10), dist2), np.float32(1e-10))
    assert d.dtype == np.float32
    d0, d1, d2 = d[..., 0], d[..., 1], d[..., 2]
    d0d1, d0d2, d1d2 = d0 * d1, d0 * d2, d1 * d2
    inv = np.float32(1.0) / (d0d1 + d0d2 + d1d2)
    return np.stack([d1d2 * inv, d0d2 * inv, d0d1 * inv], axis=1)


@pytest.mark.parametrize("m", [1, 2, 3, 257, 2500])
def test_three_nn_layouts_agree(ext, m, monkeypatch):
    """the channel-major search (brute force, and the grid search where it is the default) finds the indices of the
    point-major one, and its weights are the weight arithmetic applied to the point-major squared distances, to the bit:
    duplicates (d = 0 -> 1e-10, products 1e-20) and unfilled slots (+inf -> 1e10, products 1e20) stay in the normal range"""
    unknown = main_case()[0]
    known = lattice(m, seed=2) if m > M else main_case()[1][:, :m]
    xyz, kn = dev(cloud(unknown)), dev(cloud(known))
    dist2 = torch.empty(B, N, 3, dtype=F32, device="cuda")
    idx = torch.empty(B, N, 3, dtype=I32, device="cuda")
    assert ext.three_nn_wrapper(B, N, m, xyz, kn, dist2, idx) is None
    want_idx, want_w = cm(idx).cpu().numpy(), nn3_weights_ref(dist2.cpu().numpy())
    for cells in ("0", "1") if m >= 256 else ("0",):  # "0": brute force for every m; "1" (the default): the grid from 256 on
        monkeypatch.setenv("P2PB_EXPERIMENT", f"nn_cells={cells}")
        got_idx, got_w = ext.three_nn(cm(xyz), cm(kn))
        same_bits(got_idx, want_idx, f"three_nn idx, m = {m}, nn_cells = {cells}")
        same_bits(got_w, want_w, f"three_nn weights, m = {m}, nn_cells = {cells}")


def int_features(rng, *shape):
    return rng.integers(-8, 9, shape).astype(np.float32)


@pytest.mark.parametrize("c", [1, 5, 64])
def test_gather_points_exact(ext, c):
    rng = np.random.default_rng(c)
    feat, idx = int_features(rng, B, c, N), rng.integers(0, N, (B, M)).astype(np.int32)
    gout, pre = int_features(rng, B, c, M), int_features(rng, B, c, N)
    out = torch.empty(B, c, M, dtype=F32, device="cuda")
    assert ext.gather_points_wrapper(B, c, N, M, dev(feat), dev(idx), out) == 1
    same_bits(out, np.take_along_axis(feat, np.broadcast_to(idx[:, None, :], (B, c, M)), 2), "gather_points")
    grad = dev(pre)
    assert ext.gather_points_grad_wrapper(B, c, N, M, dev(gout), dev(idx), grad) == 1
    want = pre.astype(np.float64)
    for b in range(B):
        for l in range(c):
            np.add.at(want[b, l], idx[b], gout[b, l])
    same_bits(grad, want.astype(np.float32), "gather_points_grad (adds into its target)")


@pytest.mark.parametrize("c", [1, 5, 64])
def test_group_points_exact(ext, c):
    rng = np.random.default_rng(10 + c)
    u = 16
    feat, idx = int_features(rng, B, c, N), rng.integers(0, N, (B, M, u)).astype(np.int32)
    gout, pre = int_features(rng, B, c, M, u), int_features(rng, B, c, N)
    out = torch.empty(B, c, M, u, dtype=F32, device="cuda")
    assert ext.group_points_wrapper(B, c, N, M, u, dev(feat), dev(idx), out) == 1
    flat = np.broadcast_to(idx.reshape(B, 1, M * u), (B, c, M * u))
    same_bits(out, np.take_along_axis(feat, flat, 2).reshape(B, c, M, u), "group_points")
    grad = dev(pre)
    assert ext.group_points_grad_wrapper(B, c, N, M, u, dev(gout), dev(idx), grad) == 1
    want = pre.astype(np.float64)
    for b in range(B):
        for l in range(c):
            np.add.at(want[b, l], idx[b].ravel(), gout[b, l].ravel())
    same_bits(grad, want.astype(np.float32), "group_points_grad (adds into its target)")


def interp_case(c):
    """features f32[B,c,M] on the coarse cloud, (idx, weight)[B,N,3] of the fine one, grad_out f32[B,c,N], target prefill"""
    rng = np.random.default_rng(20 + c)
    feat, idx = int_features(rng, B, c, M), rng.integers(0, M, (B, N, 3)).astype(np.int32)
    w = (rng.integers(0, 17, (B, N, 3)) / 16.0).astype(np.float32)
    return feat, idx, w, int_features(rng, B, c, N), int_features(rng, B, c, M)


def interp_ref(feat, idx, w):
    c = feat.shape[1]
    out = np.zeros((B, c, N))
    for j in range(3):
        ij = np.broadcast_to(idx[:, None, :, j], (B, c, N))
        out += w[:, None, :, j].astype(np.float64) * np.take_along_axis(feat.astype(np.float64), ij, 2)
    return out


def interp_grad_ref(gout, idx, w, pre):
    want = pre.astype(np.float64)
    for b in range(B):
        for l in range(gout.shape[1]):
            for j in range(3):
                np.add.at(want[b, l], idx[b, :, j], gout[b, l].astype(np.float64) * w[b, :, j])
    return want


@pytest.mark.parametrize("c", [1, 5, 64])
def test_three_interpolate_exact(ext, c):
    feat, idx, w, gout, pre = interp_case(c)
    out = torch.empty(B, c, N, dtype=F32, device="cuda")
    assert ext.three_interpolate_wrapper(B, c, M, N, dev(feat), dev(idx), dev(w), out) is None
    same_bits(out, interp_ref(feat, idx, w).astype(np.float32), "three_interpolate")
    grad = dev(pre)
    assert ext.three_interpolate_grad_wrapper(B, c, N, M, dev(gout), dev(idx), dev(w), grad) is None
    same_bits(grad, interp_grad_ref(gout, idx, w, pre).astype(np.float32), "three_interpolate_grad (adds into its target)")


@pytest.mark.parametrize("c", [1, 17])  # 17 crosses the 16-channel chunk of a thread
def test_three_interpolate_layouts_agree(ext, c):
    feat, idx, w, _, _ = interp_case(c)
    out = torch.empty(B, c, N, dtype=F32, device="cuda")
    assert ext.three_interpolate_wrapper(B, c, M, N, dev(feat), dev(idx), dev(w), out) is None
    same_bits(ext.three_interpolate(dev(feat), cm(dev(idx)), cm(dev(w))), out.cpu().numpy(), "three_interpolate, both layouts")


# ---- the float family ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def float_clouds(seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (1000, 3)).astype(np.float32), rng.uniform(-1, 1, (257, 3)).astype(np.float32)


def d2_f64(a, b):
    d = a.astype(np.float64)[:, None, :] - b.astype(np.float64)[None, :, :]
    return (d * d).sum(-1)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_three_nn_float(ext, seed):
    unknown, known = float_clouds(seed)
    d2 = d2_f64(unknown, known)
    gap = np.diff(np.sort(d2, axis=1)[:, :4], axis=1).min()
    print(f"three_nn float seed {seed}: smallest gap among the four nearest = {gap:.3g}")
    assert gap > MARGIN  # no query's three nearest are decided by less than the margin
    val, ref = three_nn_ref(d2)
    dist2 = torch.empty(1, 1000, 3, dtype=F32, device="cuda")
    idx = torch.empty(1, 1000, 3, dtype=I32, device="cuda")
    ext.three_nn_wrapper(1, 1000, 257, dev(unknown[None]), dev(known[None]), dist2, idx)
    same_bits(idx[0], ref, "three_nn idx")
    err = np.abs(dist2[0].cpu().numpy().astype(np.float64) - val).max()
    print(f"three_nn float seed {seed}: max |dist2 - float64| = {err:.3g}")
    assert err <= MARGIN


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_ball_query_float(ext, seed):
    pts, ctr = float_clouds(seed)
    radius, nsample = 0.3, 16
    r2 = float(np.float32(radius)) ** 2
    d2 = d2_f64(ctr, pts)
    excluded = (np.abs(d2 - r2) < MARGIN).any(1)
    share = excluded.mean()
    print(f"ball query float seed {seed}: {int(excluded.sum())} of {excluded.size} centres have a point within the margin of r^2")
    assert share <= 0.01, share
    idx = torch.full((1, 257, nsample), -7, dtype=I32, device="cuda")
    ext.ball_query_wrapper(1, 1000, 257, radius, nsample, dev(ctr[None]), dev(pts[None]), idx)
    ref = ball_query_ref(d2, r2, nsample, -7)
    same_bits(idx[0][torch.from_numpy(~excluded).cuda()], ref[~excluded], "ball query idx")


def test_fps_float(ext):
    pts, _ = float_clouds(0)
    ridx, rtemp, gap = fps_ref(pts.astype(np.float64), 128)
    print(f"fps float: smallest gap between the two largest running minima = {gap:.3g}")
    assert gap > MARGIN
    idx, temp = run_fps(ext, pts[None], 128)
    same_bits(idx[0], ridx, "fps idx")
    err = np.abs(temp[0].cpu().numpy().astype(np.float64) - rtemp).max()
    print(f"fps float: max |temp - float64| = {err:.3g}")
    assert err <= MARGIN


# ---- memory discipline --------------------------------------------------------------------------------------------------
def test_wrappers_hold_to_their_buffers(ext):
    """each of the nine wrappers once inside a poisoned arena at the main case's shapes: inputs `put` between guards, outputs
    allocated inside it; the guards stay intact and no float output holds a NaN (an unwritten element or an over-read)"""
    pts, ctr = main_case()
    c, u = 5, 16
    rng = np.random.default_rng(3)
    feat_n, feat_m = int_features(rng, B, c, N), int_features(rng, B, c, M)
    idx_g, idx_u = rng.integers(0, N, (B, M)).astype(np.int32), rng.integers(0, N, (B, M, u)).astype(np.int32)
    idx_3 = rng.integers(0, M, (B, N, 3)).astype(np.int32)
    w_3 = (rng.integers(0, 17, (B, N, 3)) / 16.0).astype(np.float32)
    with PoisonArena("cuda", 64 << 20) as arena:
        put = lambda a: arena.put(torch.from_numpy(np.ascontiguousarray(a)))  # noqa: E731
        xyz, new_xyz = put(cloud(pts)), put(cloud(ctr))

        def done(*outs):
            arena.check_guards()
            for k, t in enumerate(outs):
                arena.assert_written(t, f"output {k}")

        idx = torch.zeros(B, M, u, dtype=I32, device="cuda")
        ext.ball_query_wrapper(B, N, M, 0.5, u, new_xyz, xyz, idx)
        done(idx)
        assert int(idx.min()) >= 0 and int(idx.max()) < N

        out = torch.empty(B, c, M, u, dtype=F32, device="cuda")
        ext.group_points_wrapper(B, c, N, M, u, put(feat_n), put(idx_u), out)
        done(out)
        grad = torch.zeros(B, c, N, dtype=F32, device="cuda")
        gout, gidx = put(int_features(rng, B, c, M, u)), put(idx_u)
        n0 = arena.n_allocations
        ext.group_points_grad_wrapper(B, c, N, M, u, gout, gidx, grad)
        done(grad)
        assert arena.n_allocations == n0 + 1  # (the scatter's fresh tensor, added to the target, came from the arena too)

        out = torch.empty(B, c, M, dtype=F32, device="cuda")
        ext.gather_points_wrapper(B, c, N, M, put(feat_n), put(idx_g), out)
        done(out)
        grad = torch.zeros(B, c, N, dtype=F32, device="cuda")
        ext.gather_points_grad_wrapper(B, c, N, M, put(int_features(rng, B, c, M)), put(idx_g), grad)
        done(grad)

        temp = torch.empty(B, N, dtype=F32, device="cuda").fill_(1e10)
        fidx = torch.empty(B, 128, dtype=I32, device="cuda")
        ext.furthest_point_sampling_wrapper(B, N, 128, xyz, temp, fidx)
        done(temp)
        assert int(fidx.min()) >= 0 and int(fidx.max()) < N

        dist2 = torch.empty(B, N, 3, dtype=F32, device="cuda")
        nidx = torch.empty(B, N, 3, dtype=I32, device="cuda")
        ext.three_nn_wrapper(B, N, M, xyz, new_xyz, dist2, nidx)
        done(dist2)
        assert bool(torch.isfinite(dist2).all()) and int(nidx.min()) >= 0 and int(nidx.max()) < M

        out = torch.empty(B, c, N, dtype=F32, device="cuda")
        ext.three_interpolate_wrapper(B, c, M, N, put(feat_m), put(idx_3), put(w_3), out)
        done(out)
        grad = torch.zeros(B, c, M, dtype=F32, device="cuda")
        ext.three_interpolate_grad_wrapper(B, c, N, M, put(int_features(rng, B, c, N)), put(idx_3), put(w_3), grad)
        done(grad)


# ---- preconditions ------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_mismatched_arguments(ext):
    """where the reference would read or write whatever memory the integers name, the wrappers raise"""
    xyz = torch.zeros(1, 64, 3, device="cuda")
    idx = torch.zeros(1, 64, 3, dtype=I32, device="cuda")
    d2 = torch.zeros(1, 64, 3, device="cuda")
    with pytest.raises(RuntimeError, match="shape"):
        ext.three_nn_wrapper(1, 65, 64, xyz, xyz, d2, idx)  # n disagrees with unknown
    with pytest.raises(RuntimeError, match="int tensor"):
        ext.three_nn_wrapper(1, 64, 64, xyz, xyz, d2, idx.long())
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.three_nn_wrapper(1, 64, 64, torch.zeros(1, 3, 64, device="cuda").transpose(1, 2), xyz, d2, idx)
    with pytest.raises(RuntimeError, match="CUDA"):
        ext.three_nn_wrapper(1, 64, 64, xyz, xyz.cpu(), d2, idx)
    with pytest.raises(RuntimeError):
        ext.ball_query_wrapper(1, 64, 64, 0.5, 0, xyz, xyz, torch.zeros(1, 64, 0, dtype=I32, device="cuda"))  # nsample = 0


def test_three_interpolate_grad_is_refused_in_deterministic_mode(ext):
    """its atomics run in no fixed order: refused like every scatter the library cannot order (include/p2pb_hip.h)"""
    import p2p_bridge_amd

    feat, idx, w, gout, pre = interp_case(1)
    grad = dev(pre)
    with p2p_bridge_amd.deterministic():
        with pytest.raises(RuntimeError, match="deterministic"):
            ext.three_interpolate_grad_wrapper(B, 1, N, M, dev(gout), dev(idx), dev(w), grad)
    same_bits(grad, pre, "a refused call writes nothing")


# ---- the operator API ---------------------------------------------------------------------------------------------------
def test_autograd_through_the_feature_operators(ops):
    c, u = 5, 16
    rng = np.random.default_rng(40)
    feat = int_features(rng, B, c, N)
    idx_g, idx_u = rng.integers(0, N, (B, M)).astype(np.int32), rng.integers(0, N, (B, M, u)).astype(np.int32)
    zero = np.zeros((B, c, N), np.float32)

    x = dev(feat).requires_grad_()
    g = int_features(rng, B, c, M)
    y = ops.gather_operation(x, dev(idx_g))
    same_bits(y.detach(), np.take_along_axis(feat, np.broadcast_to(idx_g[:, None, :], (B, c, M)), 2), "gather_operation")
    y.backward(dev(g))
    want = zero.astype(np.float64)
    for b in range(B):
        for l in range(c):
            np.add.at(want[b, l], idx_g[b], g[b, l])
    same_bits(x.grad, want.astype(np.float32), "GatherOperation.backward")

    x = dev(feat).requires_grad_()
    g = int_features(rng, B, c, M, u)
    y = ops.grouping_operation(x, dev(idx_u))
    assert y.shape == (B, c, M, u)
    y.backward(dev(g))
    want = zero.astype(np.float64)
    for b in range(B):
        for l in range(c):
            np.add.at(want[b, l], idx_u[b].ravel(), g[b, l].ravel())
    same_bits(x.grad, want.astype(np.float32), "GroupingOperation.backward")

    feat_m, idx_3, w_3, gout, _ = interp_case(c)
    x = dev(feat_m).requires_grad_()
    y = ops.three_interpolate(x, dev(idx_3), dev(w_3))
    same_bits(y.detach(), interp_ref(feat_m, idx_3, w_3).astype(np.float32), "three_interpolate")
    y.backward(dev(gout))
    same_bits(x.grad, interp_grad_ref(gout, idx_3, w_3, np.zeros((B, c, M), np.float32)).astype(np.float32),
              "ThreeInterpolate.backward")


def test_search_operators_of_the_api(ops):
    """furthest_point_sample fills temp itself, ball_query zero-fills idx first, three_nn returns distances, not squares"""
    pts, ctr = main_case()
    xyz, new_xyz = dev(cloud(pts)), dev(cloud(ctr))
    fidx = ops.furthest_point_sample(xyz, 128)
    assert fidx.dtype == I32 and not fidx.requires_grad
    for b in range(B):
        same_bits(fidx[b], fps_ref(pts[b] / 8.0, 128)[0], "furthest_point_sample")
    idx = ops.ball_query(0.25, 16, xyz, new_xyz)
    dist, nidx = ops.three_nn(xyz, new_xyz)
    for b in range(B):
        same_bits(idx[b], ball_query_ref(d2_int(ctr[b], pts[b]), 4, 16, 0), "ball_query")
        val, ref = three_nn_ref(d2_int(pts[b], ctr[b]))
        same_bits(nidx[b], ref, "three_nn idx")
        # (the square root is torch's: within an ulp or two of the correctly rounded one)
        np.testing.assert_allclose(dist[b].cpu().numpy(), np.sqrt(val / 64.0), rtol=2.4e-7, atol=0)


def test_dropin_module_exposes_the_reference_surface():
    import p2p_bridge_amd

    p2p_bridge_amd.install_dropin()
    import pointnet2_batch_cuda

    assert len(REFERENCE_NAMES) == 21 == len(set(REFERENCE_NAMES))
    missing = [name for name in REFERENCE_NAMES if not callable(getattr(pointnet2_batch_cuda, name, None))]
    assert not missing, missing
    assert sys.modules["_pvcnn_backend"] is pointnet2_batch_cuda
