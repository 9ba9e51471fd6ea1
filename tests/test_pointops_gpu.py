"""The packed-batch ("offset") operators of `pointops_cuda` (csrc/pointops.hip), their layer API (`pointops`) and the
`chamfer` module against brute-force references written here in numpy / float64 torch.

Two shapes. A: segments of 300, 1 and 699 points (n = 1000, b = 3) with 100, 7 and 150 queries (m = 257): a one-point
segment, boundaries that align to no wave or block. B: segments of 4100 and 37 points with 130 and 5 queries: the long one
is longer than any 64-point step, than 1024 threads and than one point per thread, the short one has fewer points than
k = 100.

EXACT family: coordinates k/8 with integer k in [-8, 8], so every difference, square and three-term sum is exact in fp32 and
a squared distance is (sum of integer squares) / 64. The references work on the integers and apply the tie rules of
include/p2pb_hip.h; results must be bit-identical, nothing is excluded. On 17^3 lattice sites duplicates, equal distances
and pairs exactly on the radius (at radius 0.5: integer differences with sum of squares 16) are common, so this family is
the test of the tie rules and of the padding. Features, gradients and gradient targets are integers in [-8, 8], weights
j/16: every sum is exact in any order, so the atomics' order does not show.

FLOAT family: uniform fp32 clouds in [-1, 1]^3 (default_rng(7), points drawn before queries) against float64.
MARGIN = 4e-6 absolute on squared distances: the fp32 rounding of fma(dz,dz, fma(dy,dy, dx*dx)) at this extent is below
3e-6 (three differences of magnitude <= 2 rounded to 2^-24 relative, squares <= 4, sum <= 12: < 3 * 2 * 2 * 2^-23 +
3 * 12 * 2^-24). Each test first asserts that ITS float64 reference is decided by more than the margin (or counts what is
not and bounds the share), then requires exact indices where it is.

The arithmetic operators' float cases: a result is a sum of T terms of magnitude <= A, each term carrying at most two
roundings (an operand sum and a product) and the T - 1 additions one each, all relative u = 2^-24 on values <= T A:
|error| <= ((T - 1) T + 2 T) A u <= sum_tol(T, A) = (T + 2) T A u. T and A come from the case (for a scatter: the largest
number of contributions to one target, plus its initial value), not from what the kernels return.
"""
import functools
import sys

import numpy as np
import pytest
import torch

from oracle.poison_arena import PoisonArena

pytestmark = pytest.mark.gpu

MARGIN = 4e-6
U = 2.0 ** -24
F32, I32 = torch.float32, torch.int32
PAD = float(np.float32(1e10))

# third_party/openpoints/cpp/pointops/src/pointops_api.cpp:15-27 and chamfer_dist/chamfer_cuda.cpp:37-38
POINTOPS_NAMES = ["knnquery_cuda", "ballquery_cuda", "furthestsampling_cuda", "grouping_forward_cuda", "grouping_backward_cuda",
                  "interpolation_forward_cuda", "interpolation_backward_cuda", "subtraction_forward_cuda",
                  "subtraction_backward_cuda", "aggregation_forward_cuda", "aggregation_backward_cuda", "avg_voxelize_forward",
                  "avg_voxelize_backward"]
CHAMFER_NAMES = ["forward", "backward"]


class Shape:
    def __init__(self, lens, queries):
        self.lens, self.queries = list(lens), list(queries)
        self.b, self.n, self.m = len(lens), sum(lens), sum(queries)
        self.offset = np.cumsum(lens).astype(np.int32)
        self.new_offset = np.cumsum(queries).astype(np.int32)

    def segments(self):
        """(point start, point end, query start, query end) per segment"""
        p = np.concatenate([[0], self.offset])
        q = np.concatenate([[0], self.new_offset])
        return [(int(p[s]), int(p[s + 1]), int(q[s]), int(q[s + 1])) for s in range(self.b)]


SHAPES = {"A": Shape([300, 1, 699], [100, 7, 150]), "B": Shape([4100, 37], [130, 5])}


@pytest.fixture(scope="module")
def ext():
    from p2p_bridge_amd import pointops_cuda

    return pointops_cuda


@pytest.fixture(scope="module")
def ops():
    from p2p_bridge_amd import pointops

    return pointops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = got.view(np.int32) != want.view(np.int32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {tuple(np.argwhere(bad)[0])}"


def sum_tol(terms, magnitude):
    return (terms + 2) * terms * magnitude * U


# ---- clouds -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lattice_case(name):
    """(points i64[n,3], queries i64[m,3]) in [-8, 8]; the clouds are these / 8"""
    sh = SHAPES[name]
    rng = np.random.default_rng(7)
    return rng.integers(-8, 9, (sh.n, 3)), rng.integers(-8, 9, (sh.m, 3))


@functools.lru_cache(maxsize=None)
def float_case(name):
    sh = SHAPES[name]
    rng = np.random.default_rng(7)
    return rng.uniform(-1, 1, (sh.n, 3)).astype(np.float32), rng.uniform(-1, 1, (sh.m, 3)).astype(np.float32)


def cloud(k):
    return (k / 8.0).astype(np.float32)


def d2_int(a, b):
    d = a[:, None, :] - b[None, :, :]
    return (d * d).sum(-1)


def d2_f64(a, b):
    d = a.astype(np.float64)[:, None, :] - b.astype(np.float64)[None, :, :]
    return (d * d).sum(-1)


# ---- references (shared by the tests of a case, never modified) -----------------------------------------------------------
def knn_ref(sh, d2_of, nsample):
    """d2_of(query rows, point rows) -> exact or float64 matrix. -> (idx i32[m,ns], dist f64[m,ns], sorted rows per segment):
    ascending distance, lower index first among equals, unfilled slots (1e10, segment start)"""
    idx = np.zeros((sh.m, nsample), np.int32)
    val = np.full((sh.m, nsample), PAD)
    rows = []
    for ps, pe, qs, qe in sh.segments():
        d2 = d2_of(slice(qs, qe), slice(ps, pe))
        order = np.argsort(d2, axis=1, kind="stable")
        kk = min(nsample, pe - ps)
        idx[qs:qe] = ps
        idx[qs:qe, :kk] = ps + order[:, :kk]
        val[qs:qe, :kk] = np.take_along_axis(d2, order[:, :kk], 1)
        rows.append(np.take_along_axis(d2, order, 1))
    return idx, val, rows


def ball_ref(sh, d2_of, thr, nsample, fill):
    out = np.full((sh.m, nsample), fill, np.int32)
    for ps, pe, qs, qe in sh.segments():
        d2 = d2_of(slice(qs, qe), slice(ps, pe))
        for j in range(qe - qs):
            hits = np.flatnonzero(d2[j] < thr)
            if hits.size:
                out[qs + j] = ps + hits[0]
                out[qs + j, :min(hits.size, nsample)] = ps + hits[:nsample]
    return out


def fps_segment_ref(xyz, ms, T):
    """xyz f64[len,3] -> (local idx i32[ms], tmp f64[len], smallest gap between the two largest running minima over the rounds).
    Maximum in the order (tmp desc, k mod T asc, k asc)."""
    n = xyz.shape[0]
    tmp = np.full(n, PAD)
    idx = np.zeros(ms, np.int32)
    gap = np.inf
    for j in range(1, ms):
        d = xyz - xyz[idx[j - 1]]
        tmp = np.minimum(tmp, (d * d).sum(1))
        top = np.flatnonzero(tmp == tmp.max())
        idx[j] = top[np.lexsort((top, top % T))[0]]
        if n > 1:
            two = np.partition(tmp, n - 2)[n - 2:]
            gap = min(gap, two[1] - two[0])
    return idx, tmp, gap


def fps_ref(sh, xyz, n_max):
    """sh.queries = samples per segment -> (idx i32[m] global, tmp f64[n], gap)"""
    T = min(1 << (int(n_max).bit_length() - 1), 1024)
    idx, tmp, gap = np.zeros(sh.m, np.int32), np.full(sh.n, PAD), np.inf
    for ps, pe, qs, qe in sh.segments():
        if qe > qs and pe > ps:
            i, t, g = fps_segment_ref(xyz[ps:pe], qe - qs, T)
            idx[qs:qe], tmp[ps:pe], gap = ps + i, t, min(gap, g)
    return idx, tmp, gap


def run_knn(ext, sh, pts32, qry32, nsample, offset=None, new_offset=None):
    idx = torch.full((sh.m, nsample), -7, dtype=I32, device="cuda")
    dist2 = torch.full((sh.m, nsample), -7.0, dtype=F32, device="cuda")
    assert ext.knnquery_cuda(sh.m, nsample, dev(pts32), dev(qry32), dev(sh.offset if offset is None else offset),
                             dev(sh.new_offset if new_offset is None else new_offset), idx, dist2) is None
    return idx, dist2


def run_ball(ext, sh, pts32, qry32, radius, nsample, fill=-7):
    idx = torch.full((sh.m, nsample), fill, dtype=I32, device="cuda")
    assert ext.ballquery_cuda(sh.m, radius, nsample, dev(pts32), dev(qry32), dev(sh.offset), dev(sh.new_offset), idx) == 1
    return idx


def run_fps(ext, sh, pts32, n_max):
    tmp = torch.full((sh.n,), 1e10, dtype=F32, device="cuda")
    idx = torch.full((sh.m,), -7, dtype=I32, device="cuda")
    assert ext.furthestsampling_cuda(sh.b, n_max, dev(pts32), dev(sh.offset), dev(sh.new_offset), tmp, idx) is None
    return idx, tmp


# ---- the exact family: searches -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsample", [1, 3, 16, 100])
@pytest.mark.parametrize("name", ["A", "B"])
def test_knnquery_exact(ext, name, nsample):
    sh = SHAPES[name]
    pts, qry = lattice_case(name)
    ridx, rval, rows = knn_ref(sh, lambda q, p: d2_int(qry[q], pts[p]), nsample)
    idx, dist2 = run_knn(ext, sh, cloud(pts), cloud(qry), nsample)
    same_bits(idx, ridx, "knnquery idx")
    same_bits(dist2, np.where(rval == PAD, PAD, rval / 64.0).astype(np.float32), "knnquery dist2")
    # the fixture must not pass vacuously: equal distances inside the lists and across their last slot, unfilled slots
    ties = sum(int((np.diff(r[:, :nsample + 1], axis=1) == 0).any(1).sum()) for r in rows if r.shape[1] > 1)
    assert ties > 0
    assert (rval == PAD).any() == (nsample > min(sh.lens))


@pytest.mark.parametrize("radius", [0.0, 0.5, 4.0])
@pytest.mark.parametrize("nsample", [1, 16, 64])
@pytest.mark.parametrize("name", ["A", "B"])
def test_ballquery_exact(ext, name, nsample, radius):
    sh = SHAPES[name]
    pts, qry = lattice_case(name)
    thr = int(round(64 * radius * radius))  # 0, 16 or 1024: d2 < r^2 on the integers
    ref = ball_ref(sh, lambda q, p: d2_int(qry[q], pts[p]), thr, nsample, -7)
    same_bits(run_ball(ext, sh, cloud(pts), cloud(qry), radius, nsample), ref, "ballquery idx")
    untouched = int((ref == -7).all(1).sum())
    if radius == 0.0:
        assert untouched == sh.m  # d2 < 0 never holds: every row keeps the sentinel
    elif radius == 0.5:
        on_radius = sum(int((d2_int(qry[qs:qe], pts[ps:pe]) == thr).sum()) for ps, pe, qs, qe in sh.segments())
        assert on_radius > 0 and (untouched > 0 or name == "B")  # (A's one-point segment leaves queries without a hit)
    else:
        assert untouched == 0  # the whole cube is inside: the first nsample points of the segment


def test_ballquery_layer_zero_fills(ops):
    sh = SHAPES["A"]
    pts, qry = lattice_case("A")
    idx = ops.ballquery(0.5, 16, dev(cloud(pts)), dev(cloud(qry)), dev(sh.offset), dev(sh.new_offset))
    same_bits(idx, ball_ref(sh, lambda q, p: d2_int(qry[q], pts[p]), 16, 16, 0), "ballquery")


# samples per segment. A: the one-point segment is asked for 7 samples (repeats), then for none; B; a 17000-point segment
# (n_max > 16384: the streaming form) next to a 50-point one asked for 60. n_max: the longest segment, or what sets another
# form / tie modulus -- 40, 200 (and 2500, 37 for B) announce less than the segments hold (T = 32, 128: streaming inside
# the register forms), 1500, 3000, 5000 are the other points-per-thread forms, 16000 the one without the LDS copy
FPS_CASES = {
    "A": ([300, 1, 699], [100, 7, 150], [699, 40, 200, 1000, 1500, 3000, 5000, 16000, 20000]),
    "A-none": ([300, 1, 699], [100, 0, 150], [699]),
    "A-first-none": ([300, 1, 699], [0, 3, 150], [699]),
    "B": ([4100, 37], [130, 5], [4100, 2500, 37]),
    "big": ([17000, 50], [12, 60], [17000]),
    # segments longer than n_max announces that still fit the points-per-thread form n_max chooses (1500: two per thread, up
    # to 2048; 9000: sixteen, up to 16384), where the LDS copy of the winner's coordinates is sized by n_max; each next to the
    # n_max that tells the truth, and 16384: the sixteen-per-thread form without the copy
    "C": ([2000, 50], [64, 20], [1500, 2000]),
    "D": ([12000, 300], [64, 32], [9000, 12000, 16384]),
}


@pytest.mark.parametrize("case", sorted(FPS_CASES))
def test_furthestsampling_exact(ext, case):
    lens, samples, n_maxes = FPS_CASES[case]
    sh = Shape(lens, samples)
    pts = np.random.default_rng(11).integers(-8, 9, (sh.n, 3))
    for n_max in n_maxes:
        ridx, rtmp, _ = fps_ref(sh, pts / 8.0, n_max)
        idx, tmp = run_fps(ext, sh, cloud(pts), n_max)
        same_bits(idx, ridx, f"furthestsampling idx, n_max = {n_max}")
        same_bits(tmp, rtmp.astype(np.float32), f"furthestsampling tmp, n_max = {n_max}")
    for (ps, pe, qs, qe) in sh.segments():
        if qe - qs > pe - ps:
            assert len(set(ridx[qs:qe].tolist())) < qe - qs  # more samples than points: indices repeat


def test_furthestsampling_ties_are_common_in_the_exact_fixture():
    """the exact clouds must exercise the tie order: in some round several points share the maximum"""
    k = np.random.default_rng(11).integers(-8, 9, (1000, 3))[301:] / 8.0
    tmp, tied, last = np.full(699, 1e10), 0, 0
    for _ in range(1, 150):
        tmp = np.minimum(tmp, ((k - k[last]) ** 2).sum(1))
        top = np.flatnonzero(tmp == tmp.max())
        tied += top.size > 1
        last = top[np.lexsort((top, top % 512))[0]]
    assert tied >= 10, tied


@pytest.mark.parametrize("n", [37, 1000, 2500, 9000, 16000, 20000])
def test_furthestsampling_is_the_batched_sampler_on_equal_segments(ext, n):
    """`pointnet2_batch_cuda.furthest_point_sampling_wrapper` on [b, n, 3] and `furthestsampling_cuda` on the same clouds
    packed with n_max = n run one kernel family: equal indices once a segment's start is taken off, equal running minima.
    n: 64 threads; 1024 with one and four points each; sixteen with and without the LDS copy; the streaming form."""
    from p2p_bridge_amd import pointnet2_batch_cuda

    b, m = 2, min(n, 64)
    xyz = dev(cloud(np.random.default_rng(11).integers(-8, 9, (b, n, 3))))
    temp = torch.full((b, n), 1e10, dtype=F32, device="cuda")
    bidx = torch.full((b, m), -7, dtype=I32, device="cuda")
    assert pointnet2_batch_cuda.furthest_point_sampling_wrapper(b, n, m, xyz, temp, bidx) == 1
    sh = Shape([n] * b, [m] * b)
    pidx, tmp = run_fps(ext, sh, xyz.reshape(b * n, 3).cpu().numpy(), n)
    starts = torch.arange(b, dtype=I32, device="cuda")[:, None] * n
    same_bits(pidx.reshape(b, m) - starts, bidx.cpu().numpy(), f"packed against batched idx, n = {n}")
    same_bits(tmp.reshape(b, n), temp.cpu().numpy(), f"packed against batched tmp, n = {n}")


# ---- the exact family: arithmetic -----------------------------------------------------------------------------------------
N, M, NS = 1000, 257, 16


def ints(rng, *shape):
    return rng.integers(-8, 9, shape).astype(np.float32)


def sixteenths(rng, *shape):
    return (rng.integers(0, 17, shape) / 16.0).astype(np.float32)


def scatter_add(target, idx, src):
    """target f64[n,c] += src f64[..., c] at idx[...]"""
    out = target.copy()
    np.add.at(out, idx.ravel(), src.reshape(-1, src.shape[-1]))
    return out


@pytest.mark.parametrize("c", [1, 5, 32])
def test_grouping_exact(ext, c):
    rng = np.random.default_rng(c)
    feat, idx = ints(rng, N, c), rng.integers(0, 100, (M, NS)).astype(np.int32)  # (100 targets for 4112 rows: the atomics collide)
    gout, pre = ints(rng, M, NS, c), ints(rng, N, c)
    out = torch.full((M, NS, c), 77.0, dtype=F32, device="cuda")
    assert ext.grouping_forward_cuda(M, NS, c, dev(feat), dev(idx), out) is None
    same_bits(out, feat[idx], "grouping_forward (writes)")
    grad = dev(pre)
    ext.grouping_backward_cuda(M, NS, c, dev(gout), dev(idx), grad)
    same_bits(grad, scatter_add(pre.astype(np.float64), idx, gout.astype(np.float64)).astype(np.float32),
              "grouping_backward (adds into its target)")


def interpolation_refs(feat, idx, w, gout, pre_out, pre_grad):
    f, w64 = feat.astype(np.float64), w.astype(np.float64)
    out = pre_out.astype(np.float64) + (f[idx] * w64[:, :, None]).sum(1)
    grad = scatter_add(pre_grad.astype(np.float64), idx, gout.astype(np.float64)[:, None, :] * w64[:, :, None])
    return out, grad


@pytest.mark.parametrize("c", [1, 5, 32])
def test_interpolation_exact(ext, c):
    rng = np.random.default_rng(20 + c)
    k = 3
    feat, idx, w = ints(rng, M, c), rng.integers(0, M, (N, k)).astype(np.int32), sixteenths(rng, N, k)
    gout, pre_out, pre_grad = ints(rng, N, c), ints(rng, N, c), ints(rng, M, c)
    rout, rgrad = interpolation_refs(feat, idx, w, gout, pre_out, pre_grad)
    out = dev(pre_out)
    assert ext.interpolation_forward_cuda(N, c, k, dev(feat), dev(idx), dev(w), out) is None
    same_bits(out, rout.astype(np.float32), "interpolation_forward (adds to its output)")
    grad = dev(pre_grad)
    ext.interpolation_backward_cuda(N, c, k, dev(gout), dev(idx), dev(w), grad)
    same_bits(grad, rgrad.astype(np.float32), "interpolation_backward (adds into its target)")


def subtraction_refs(in1, in2, idx, gout, pre1, pre2):
    out = in1.astype(np.float64)[:, None, :] - in2.astype(np.float64)[idx]
    g = gout.astype(np.float64)
    return out, pre1.astype(np.float64) + g.sum(1), scatter_add(pre2.astype(np.float64), idx, -g)


@pytest.mark.parametrize("c", [1, 5, 32])
def test_subtraction_exact(ext, c):
    rng = np.random.default_rng(30 + c)
    in1, in2, idx = ints(rng, N, c), ints(rng, N, c), rng.integers(0, 60, (N, NS)).astype(np.int32)
    gout, pre1, pre2 = ints(rng, N, NS, c), ints(rng, N, c), ints(rng, N, c)
    rout, r1, r2 = subtraction_refs(in1, in2, idx, gout, pre1, pre2)
    out = torch.full((N, NS, c), 77.0, dtype=F32, device="cuda")
    assert ext.subtraction_forward_cuda(N, NS, c, dev(in1), dev(in2), dev(idx), out) is None
    same_bits(out, rout.astype(np.float32), "subtraction_forward (writes)")
    g1, g2 = dev(pre1), dev(pre2)
    ext.subtraction_backward_cuda(N, NS, c, dev(idx), dev(gout), g1, g2)
    same_bits(g1, r1.astype(np.float32), "subtraction_backward grad_input1 (adds)")
    same_bits(g2, r2.astype(np.float32), "subtraction_backward grad_input2 (adds)")


def aggregation_refs(inp, pos, w, idx, gout, pre_out, pre_gi, pre_gw):
    n, ns, c = pos.shape
    w_c = w.shape[-1]
    wfull = np.tile(w.astype(np.float64), (1, 1, c // w_c))  # [n, ns, c]: channel ch uses weight ch mod w_c
    s = inp.astype(np.float64)[idx] + pos.astype(np.float64)
    out = pre_out.astype(np.float64) + (s * wfull).sum(1)
    gw = gout.astype(np.float64)[:, None, :] * wfull
    gi = scatter_add(pre_gi.astype(np.float64), idx, gw)
    gweight = pre_gw.astype(np.float64) + (gout.astype(np.float64)[:, None, :] * s).reshape(n, ns, c // w_c, w_c).sum(2)
    return out, gi, gw, gweight


@pytest.mark.parametrize("c,w_c", [(1, 1), (5, 1), (5, 5), (32, 1), (32, 8), (32, 32)])
def test_aggregation_exact(ext, c, w_c):
    rng = np.random.default_rng(40 + 100 * c + w_c)
    inp, pos, w = ints(rng, N, c), ints(rng, N, NS, c), sixteenths(rng, N, NS, w_c)
    idx, gout = rng.integers(0, 60, (N, NS)).astype(np.int32), ints(rng, N, c)
    pre_out, pre_gi, pre_gw = ints(rng, N, c), ints(rng, N, c), ints(rng, N, NS, w_c)
    rout, rgi, rgp, rgw = aggregation_refs(inp, pos, w, idx, gout, pre_out, pre_gi, pre_gw)
    out = dev(pre_out)
    assert ext.aggregation_forward_cuda(N, NS, c, w_c, dev(inp), dev(pos), dev(w), dev(idx), out) is None
    same_bits(out, rout.astype(np.float32), "aggregation_forward (adds to its output)")
    gi, gw = dev(pre_gi), dev(pre_gw)
    gp = torch.full((N, NS, c), 77.0, dtype=F32, device="cuda")
    ext.aggregation_backward_cuda(N, NS, c, w_c, dev(inp), dev(pos), dev(w), dev(idx), dev(gout), gi, gp, gw)
    same_bits(gi, rgi.astype(np.float32), "aggregation_backward grad_input (adds)")
    same_bits(gp, rgp.astype(np.float32), "aggregation_backward grad_position (writes)")
    same_bits(gw, rgw.astype(np.float32), "aggregation_backward grad_weight (adds)")


# ---- the float family -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsample", [3, 16, 100])
@pytest.mark.parametrize("name", ["A", "B"])
def test_knnquery_float(ext, name, nsample):
    sh = SHAPES[name]
    pts, qry = float_case(name)
    ridx, rval, rows = knn_ref(sh, lambda q, p: d2_f64(qry[q], pts[p]), nsample)
    decided = np.zeros((sh.m, nsample), bool)
    real = np.zeros((sh.m, nsample), bool)
    for (ps, pe, qs, qe), r in zip(sh.segments(), rows):
        kk = min(nsample, pe - ps)
        gaps = np.diff(r[:, :kk + 1], axis=1) > 2 * MARGIN  # [mq, kk - 1 or kk]: slot j against slot j + 1 (the kk + 1-th counts)
        left = np.concatenate([np.ones((qe - qs, 1), bool), gaps[:, :kk - 1]], axis=1)
        right = np.concatenate([gaps, np.ones((qe - qs, kk - gaps.shape[1]), bool)], axis=1)
        decided[qs:qe, :kk] = left & right
        real[qs:qe, :kk] = True
    left_out = int((real & ~decided).sum())
    print(f"knnquery float {name}, nsample {nsample}: {left_out} of {int(real.sum())} slots left out")
    assert left_out <= 0.02 * real.sum()
    if nsample <= 3:
        assert left_out == 0
    idx, dist2 = run_knn(ext, sh, pts, qry, nsample)
    got = dist2.cpu().numpy().astype(np.float64)
    assert (got[~real] == PAD).all()
    err = np.abs(got[real] - rval[real]).max()
    print(f"knnquery float {name}, nsample {nsample}: max |dist2 - float64| = {err:.3g}")
    assert err <= MARGIN
    gi = idx.cpu().numpy()
    assert (gi[~real] == ridx[~real]).all()
    bad = decided & (gi != ridx)
    assert not bad.any(), f"{int(bad.sum())} decided slots differ, first at {tuple(np.argwhere(bad)[0])}"


@pytest.mark.parametrize("radius", [0.05, 0.3, 0.6])
@pytest.mark.parametrize("name", ["A", "B"])
def test_ballquery_float(ext, name, radius):
    sh = SHAPES[name]
    pts, qry = float_case(name)
    nsample = 16
    r2 = float(np.float32(radius) * np.float32(radius))
    excluded = np.zeros(sh.m, bool)
    for ps, pe, qs, qe in sh.segments():
        excluded[qs:qe] = (np.abs(d2_f64(qry[qs:qe], pts[ps:pe]) - r2) < MARGIN).any(1)
    print(f"ballquery float {name}, radius {radius}: {int(excluded.sum())} of {sh.m} rows have a point within the margin of r^2")
    assert excluded.mean() <= 0.01
    ref = ball_ref(sh, lambda q, p: d2_f64(qry[q], pts[p]), r2, nsample, -7)
    idx = run_ball(ext, sh, pts, qry, radius, nsample)
    same_bits(idx[torch.from_numpy(~excluded).cuda()], ref[~excluded], "ballquery idx")


@pytest.mark.parametrize("name", ["A", "B"])
def test_furthestsampling_float(ext, name):
    src = SHAPES[name]
    sh = Shape(src.lens, [100, 1, 150] if name == "A" else [130, 5])
    pts, _ = float_case(name)
    ridx, rtmp, gap = fps_ref(sh, pts.astype(np.float64), max(sh.lens))
    print(f"furthestsampling float {name}: smallest gap between the two largest running minima = {gap:.3g}")
    assert gap > MARGIN
    idx, tmp = run_fps(ext, sh, pts, max(sh.lens))
    same_bits(idx, ridx, "furthestsampling idx")
    err = np.abs(tmp.cpu().numpy().astype(np.float64) - rtmp).max()
    print(f"furthestsampling float {name}: max |tmp - float64| = {err:.3g}")
    assert err <= MARGIN


def uniform(rng, *shape):
    return rng.uniform(-1, 1, shape).astype(np.float32)


def most_hits(idx):
    """the largest number of contributions one scatter target receives"""
    return int(np.bincount(idx.ravel()).max())


def close(got, want, tol, what):
    err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
    print(f"{what}: max |error| = {err:.3g}, bound {tol:.3g}")
    assert err <= tol, (what, err, tol)


def test_arithmetic_float(ext):
    """one case per arithmetic kernel: uniform [-1, 1] operands against float64, bounds by sum_tol (module docstring)"""
    rng = np.random.default_rng(5)
    c, w_c, k = 12, 4, 3
    # grouping: the forward pass copies; the gradient sums most_hits + 1 values of magnitude <= 1
    feat, idx = uniform(rng, N, c), rng.integers(0, 100, (M, NS)).astype(np.int32)
    gout, pre = uniform(rng, M, NS, c), uniform(rng, N, c)
    out = torch.empty(M, NS, c, dtype=F32, device="cuda")
    ext.grouping_forward_cuda(M, NS, c, dev(feat), dev(idx), out)
    same_bits(out, feat[idx], "grouping_forward")
    grad = dev(pre)
    ext.grouping_backward_cuda(M, NS, c, dev(gout), dev(idx), grad)
    close(grad, scatter_add(pre.astype(np.float64), idx, gout.astype(np.float64)), sum_tol(most_hits(idx) + 1, 1.0),
          "grouping_backward")
    # interpolation: k products |input w| <= 1 and the initial value
    feat, idx, w = uniform(rng, M, c), rng.integers(0, M, (N, k)).astype(np.int32), uniform(rng, N, k)
    gout, pre_out, pre_grad = uniform(rng, N, c), uniform(rng, N, c), uniform(rng, M, c)
    rout, rgrad = interpolation_refs(feat, idx, w, gout, pre_out, pre_grad)
    out, grad = dev(pre_out), dev(pre_grad)
    ext.interpolation_forward_cuda(N, c, k, dev(feat), dev(idx), dev(w), out)
    close(out, rout, sum_tol(k + 1, 1.0), "interpolation_forward")
    ext.interpolation_backward_cuda(N, c, k, dev(gout), dev(idx), dev(w), grad)
    close(grad, rgrad, sum_tol(most_hits(idx) + 1, 1.0), "interpolation_backward")
    # subtraction: one difference of magnitude <= 2; row sums of nsample + 1 values; the scatter
    in1, in2, idx = uniform(rng, N, c), uniform(rng, N, c), rng.integers(0, 60, (N, NS)).astype(np.int32)
    gout, pre1, pre2 = uniform(rng, N, NS, c), uniform(rng, N, c), uniform(rng, N, c)
    rout, r1, r2 = subtraction_refs(in1, in2, idx, gout, pre1, pre2)
    out, g1, g2 = torch.empty(N, NS, c, dtype=F32, device="cuda"), dev(pre1), dev(pre2)
    ext.subtraction_forward_cuda(N, NS, c, dev(in1), dev(in2), dev(idx), out)
    close(out, rout, 2.0 * U, "subtraction_forward")
    ext.subtraction_backward_cuda(N, NS, c, dev(idx), dev(gout), g1, g2)
    close(g1, r1, sum_tol(NS + 1, 1.0), "subtraction_backward grad_input1")
    close(g2, r2, sum_tol(most_hits(idx) + 1, 1.0), "subtraction_backward grad_input2")
    # aggregation: terms (input + position) weight of magnitude <= 2
    inp, pos, w = uniform(rng, N, c), uniform(rng, N, NS, c), uniform(rng, N, NS, w_c)
    idx, gout = rng.integers(0, 60, (N, NS)).astype(np.int32), uniform(rng, N, c)
    pre_out, pre_gi, pre_gw = uniform(rng, N, c), uniform(rng, N, c), uniform(rng, N, NS, w_c)
    rout, rgi, rgp, rgw = aggregation_refs(inp, pos, w, idx, gout, pre_out, pre_gi, pre_gw)
    out, gi, gw = dev(pre_out), dev(pre_gi), dev(pre_gw)
    gp = torch.empty(N, NS, c, dtype=F32, device="cuda")
    ext.aggregation_forward_cuda(N, NS, c, w_c, dev(inp), dev(pos), dev(w), dev(idx), out)
    close(out, rout, sum_tol(NS + 1, 2.0), "aggregation_forward")
    ext.aggregation_backward_cuda(N, NS, c, w_c, dev(inp), dev(pos), dev(w), dev(idx), dev(gout), gi, gp, gw)
    close(gi, rgi, sum_tol(most_hits(idx) + 1, 1.0), "aggregation_backward grad_input")
    close(gp, rgp, U, "aggregation_backward grad_position")  # (one product of magnitude <= 1)
    close(gw, rgw, sum_tol(c // w_c + 1, 2.0), "aggregation_backward grad_weight")


# ---- the layer API --------------------------------------------------------------------------------------------------------
def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().double()


def test_autograd_functions_against_float64_indexing(ops):
    """exact-family operands: the float64 expressions in torch indexing ops and their autograd gradients must be met exactly"""
    rng = np.random.default_rng(50)
    c, w_c = 8, 4
    idx_g, idx_n = rng.integers(0, 100, (M, NS)).astype(np.int32), rng.integers(0, 60, (N, NS)).astype(np.int32)
    lg, ln = dev(idx_g).long(), dev(idx_n).long()

    feat, g = ints(rng, N, c), ints(rng, M, NS, c)
    x, x64 = dev(feat).requires_grad_(), t64(feat).requires_grad_()
    y, y64 = ops.grouping(x, dev(idx_g)), x64[lg]
    y.backward(dev(g)), y64.backward(t64(g))
    assert torch.equal(y.double(), y64) and torch.equal(x.grad.double(), x64.grad)

    in1, in2, g = ints(rng, N, c), ints(rng, N, c), ints(rng, N, NS, c)
    a, b_ = dev(in1).requires_grad_(), dev(in2).requires_grad_()
    a64, b64 = t64(in1).requires_grad_(), t64(in2).requires_grad_()
    y, y64 = ops.subtraction(a, b_, dev(idx_n)), a64[:, None, :] - b64[ln]
    y.backward(dev(g)), y64.backward(t64(g))
    assert torch.equal(y.double(), y64)
    assert torch.equal(a.grad.double(), a64.grad) and torch.equal(b_.grad.double(), b64.grad)

    inp, pos, w, g = ints(rng, N, c), ints(rng, N, NS, c), sixteenths(rng, N, NS, w_c), ints(rng, N, c)
    ts = [dev(v).requires_grad_() for v in (inp, pos, w)]
    ts64 = [t64(v).requires_grad_() for v in (inp, pos, w)]
    y = ops.aggregation(*ts, dev(idx_n))
    y64 = ((ts64[0][ln] + ts64[1]) * ts64[2].repeat(1, 1, c // w_c)).sum(1)
    y.backward(dev(g)), y64.backward(t64(g))
    assert torch.equal(y.double(), y64)
    for t, r, what in zip(ts, ts64, ("input", "position", "weight")):
        assert torch.equal(t.grad.double(), r.grad), what


def test_interpolation_layers(ops):
    """interpolation2 (kernels) against interpolation (torch indexing) and against float64 with the same (idx, weight); the
    gradient against float64 autograd. Weights are positive and sum to 1, features of magnitude <= 1: sum_tol(k + 1, 1)."""
    sh = SHAPES["A"]
    pts, qry = float_case("A")
    c, k = 6, 3
    rng = np.random.default_rng(60)
    feat, g = uniform(rng, sh.n, c), uniform(rng, sh.m, c)
    xyz, new_xyz, off, noff = dev(pts), dev(qry), dev(sh.offset), dev(sh.new_offset)
    x = dev(feat).requires_grad_()
    y2 = ops.interpolation2(xyz, new_xyz, x, off, noff, k)
    y1 = ops.interpolation(xyz, new_xyz, dev(feat), off, noff, k)
    idx, weight = ops._inverse_distance_weights(xyz, new_xyz, off, noff, k)
    x64 = t64(feat).requires_grad_()
    y64 = (x64[idx.long()] * weight.double()[:, :, None]).sum(1)
    close(y2.detach(), y64.detach().cpu().numpy(), sum_tol(k + 1, 1.0), "interpolation2")
    close(y1, y64.detach().cpu().numpy(), sum_tol(k + 1, 1.0), "interpolation")
    # interpolation(...) equals interpolation2(...): same (idx, weight), each within the bound of the exact sum
    close(y1, y2.detach().cpu().numpy().astype(np.float64), 2 * sum_tol(k + 1, 1.0), "interpolation against interpolation2")
    y2.backward(dev(g)), y64.backward(t64(g))
    close(x.grad, x64.grad.cpu().numpy(), sum_tol(most_hits(idx.cpu().numpy()) + 1, 1.0), "Interpolation.backward")


def test_query_layers(ops):
    """KNNQuery returns distances, not squares; new_xyz = None means xyz; queryandgroup / querygroup against torch indexing"""
    sh = SHAPES["A"]
    pts, qry = lattice_case("A")
    xyz, new_xyz, off, noff = dev(cloud(pts)), dev(cloud(qry)), dev(sh.offset), dev(sh.new_offset)
    ridx, rval, _ = knn_ref(sh, lambda q, p: d2_int(qry[q], pts[p]), 16)
    idx, dist = ops.knnquery(16, xyz, new_xyz, off, noff)
    same_bits(idx, ridx, "knnquery idx")
    want = np.sqrt(np.where(rval == PAD, PAD, rval / 64.0))
    # (the square root is torch's: within an ulp or two of the correctly rounded one)
    np.testing.assert_allclose(dist.cpu().numpy(), want, rtol=2.4e-7, atol=0)
    self_sh = Shape(sh.lens, sh.lens)
    sidx, _, _ = knn_ref(self_sh, lambda q, p: d2_int(pts[q], pts[p]), 3)
    same_bits(ops.knnquery(3, xyz, None, off, off)[0], sidx, "knnquery, new_xyz = None")

    c = 5
    feat = dev(ints(np.random.default_rng(70), sh.n, c))
    flat = dev(ridx).long().flatten()
    gxyz = xyz[flat].view(sh.m, 16, 3) - new_xyz[:, None, :]
    gfeat = feat[flat].view(sh.m, 16, c)
    assert torch.equal(ops.queryandgroup(16, xyz, new_xyz, feat, None, off, noff), torch.cat((gxyz, gfeat), -1))
    assert torch.equal(ops.queryandgroup(16, xyz, new_xyz, feat, dev(ridx), off, noff, use_xyz=False), gfeat)
    a, b_ = ops.querygroup(16, xyz, new_xyz, feat, off, noff)
    assert torch.equal(a, gxyz) and torch.equal(b_, gfeat)
    given = dev(np.random.default_rng(71).integers(0, sh.n, (sh.m, 4)).astype(np.int32))  # (the reference returns None here)
    a, b_ = ops.querygroup(None, xyz, new_xyz, feat, off, noff, idx=given)
    assert torch.equal(a, xyz[given.long().flatten()].view(sh.m, 4, 3) - new_xyz[:, None, :])
    assert torch.equal(b_, feat[given.long().flatten()].view(sh.m, 4, c))
    bidx = ball_ref(sh, lambda q, p: d2_int(qry[q], pts[p]), 16, 8, 0)
    a, _ = ops.querygroup(8, xyz, new_xyz, feat, off, noff, radius=0.5, query_method="ball")
    assert torch.equal(a, xyz[dev(bidx).long().flatten()].view(sh.m, 8, 3) - new_xyz[:, None, :])
    rel = xyz[dev(bidx).long().flatten()].view(sh.m, 8, 3) - new_xyz[:, None, :]
    a, _ = ops.querygroup(8, xyz, new_xyz, feat, off, noff, radius=0.5, query_method="ball", normalize_dp=True)
    assert torch.equal(a, rel / 0.5)  # a ball query's relative coordinates are divided by the radius
    a, _ = ops.querygroup(16, xyz, new_xyz, feat, off, noff, normalize_dp=True)  # "knn": by each neighbour's own distance + 1e-8
    torch.testing.assert_close(a, gxyz / (gxyz.square().sum(-1, keepdim=True).sqrt() + 1.0e-8), rtol=4 * 2.0 ** -23, atol=0)
    with pytest.raises(ValueError):
        ops.querygroup(None, xyz, new_xyz, feat, off, noff)
    self_grouped, _ = ops.querygroup(3, xyz, None, feat, off, off)  # (the reference asserts on None first)
    assert torch.equal(self_grouped, xyz[dev(sidx).long().flatten()].view(sh.n, 3, 3) - xyz[:, None, :])
    fidx = ops.furthestsampling(xyz, off, noff)
    same_bits(fidx, fps_ref(sh, pts / 8.0, 699)[0], "furthestsampling")


# ---- memory discipline ----------------------------------------------------------------------------------------------------
def test_entry_points_hold_to_their_buffers(ext):
    """each of the 11 entry points once inside a poisoned arena at shape A with c = 5: inputs `put` between guards, outputs
    allocated inside it; the guards stay intact and no float output that the contract says is written holds a NaN"""
    sh = SHAPES["A"]
    pts, qry = lattice_case("A")
    c, w_c, k = 5, 5, 3
    rng = np.random.default_rng(3)
    with PoisonArena("cuda", 64 << 20) as arena:
        put = lambda a: arena.put(torch.from_numpy(np.ascontiguousarray(a)))  # noqa: E731
        xyz, new_xyz, off, noff = put(cloud(pts)), put(cloud(qry)), put(sh.offset), put(sh.new_offset)

        def done(*outs):
            arena.check_guards()
            for j, t in enumerate(outs):
                arena.assert_written(t, f"output {j}")

        idx = torch.empty(sh.m, NS, dtype=I32, device="cuda")
        dist2 = torch.empty(sh.m, NS, dtype=F32, device="cuda")
        ext.knnquery_cuda(sh.m, NS, xyz, new_xyz, off, noff, idx, dist2)
        done(dist2)
        assert int(idx.min()) >= 0 and int(idx.max()) < sh.n

        idx = torch.zeros(sh.m, NS, dtype=I32, device="cuda")
        ext.ballquery_cuda(sh.m, 0.5, NS, xyz, new_xyz, off, noff, idx)
        done()
        assert int(idx.min()) >= 0 and int(idx.max()) < sh.n

        tmp = torch.empty(sh.n, dtype=F32, device="cuda").fill_(1e10)
        fidx = torch.empty(sh.m, dtype=I32, device="cuda")
        ext.furthestsampling_cuda(sh.b, 699, xyz, off, noff, tmp, fidx)
        done(tmp)
        assert int(fidx.min()) >= 0 and int(fidx.max()) < sh.n

        gidx, nidx = put(rng.integers(0, sh.n, (sh.m, NS)).astype(np.int32)), put(rng.integers(0, sh.n, (sh.n, NS)).astype(np.int32))
        kidx, kw = put(rng.integers(0, sh.m, (sh.n, k)).astype(np.int32)), put(sixteenths(rng, sh.n, k))
        out = torch.empty(sh.m, NS, c, dtype=F32, device="cuda")
        ext.grouping_forward_cuda(sh.m, NS, c, put(ints(rng, sh.n, c)), gidx, out)
        done(out)
        grad = torch.zeros(sh.n, c, dtype=F32, device="cuda")
        ext.grouping_backward_cuda(sh.m, NS, c, put(ints(rng, sh.m, NS, c)), gidx, grad)
        done(grad)

        out = torch.zeros(sh.n, c, dtype=F32, device="cuda")
        ext.interpolation_forward_cuda(sh.n, c, k, put(ints(rng, sh.m, c)), kidx, kw, out)
        done(out)
        grad = torch.zeros(sh.m, c, dtype=F32, device="cuda")
        ext.interpolation_backward_cuda(sh.n, c, k, put(ints(rng, sh.n, c)), kidx, kw, grad)
        done(grad)

        out = torch.empty(sh.n, NS, c, dtype=F32, device="cuda")
        ext.subtraction_forward_cuda(sh.n, NS, c, put(ints(rng, sh.n, c)), put(ints(rng, sh.n, c)), nidx, out)
        done(out)
        g1, g2 = torch.zeros(sh.n, c, dtype=F32, device="cuda"), torch.zeros(sh.n, c, dtype=F32, device="cuda")
        ext.subtraction_backward_cuda(sh.n, NS, c, nidx, put(ints(rng, sh.n, NS, c)), g1, g2)
        done(g1, g2)

        inp, pos, w = put(ints(rng, sh.n, c)), put(ints(rng, sh.n, NS, c)), put(sixteenths(rng, sh.n, NS, w_c))
        out = torch.zeros(sh.n, c, dtype=F32, device="cuda")
        ext.aggregation_forward_cuda(sh.n, NS, c, w_c, inp, pos, w, nidx, out)
        done(out)
        gi, gw = torch.zeros(sh.n, c, dtype=F32, device="cuda"), torch.zeros(sh.n, NS, w_c, dtype=F32, device="cuda")
        gp = torch.empty(sh.n, NS, c, dtype=F32, device="cuda")
        ext.aggregation_backward_cuda(sh.n, NS, c, w_c, inp, pos, w, nidx, put(ints(rng, sh.n, c)), gi, gp, gw)
        done(gi, gp, gw)


# offsets that claim more than the tensors hold, and offsets in no order: the lookups are bounded by b and the ends clamped
@pytest.mark.parametrize("offset,new_offset", [([300, 301, 1500], [100, 107, 400]), ([700, -5, 2000], [300, 2, -1])])
def test_searches_survive_offsets_that_lie(ext, offset, new_offset):
    """inside the arena, so that a stray write would show as a broken guard: the calls return and every index is in [0, n)"""
    sh = SHAPES["A"]
    pts, qry = lattice_case("A")
    with PoisonArena("cuda", 16 << 20) as arena:
        put = lambda a: arena.put(torch.from_numpy(np.ascontiguousarray(a)))  # noqa: E731
        xyz, new_xyz = put(cloud(pts)), put(cloud(qry))
        off, noff = put(np.array(offset, np.int32)), put(np.array(new_offset, np.int32))
        idx = torch.zeros(sh.m, NS, dtype=I32, device="cuda")
        dist2 = torch.zeros(sh.m, NS, dtype=F32, device="cuda")
        ext.knnquery_cuda(sh.m, NS, xyz, new_xyz, off, noff, idx, dist2)
        arena.check_guards()
        arena.assert_written(dist2, "dist2")
        assert int(idx.min()) >= 0 and int(idx.max()) < sh.n
        idx = torch.zeros(sh.m, NS, dtype=I32, device="cuda")
        ext.ballquery_cuda(sh.m, 4.0, NS, xyz, new_xyz, off, noff, idx)
        arena.check_guards()
        assert int(idx.min()) >= 0 and int(idx.max()) < sh.n


def test_wrappers_refuse_mismatched_arguments(ext):
    sh = SHAPES["A"]
    xyz, q = torch.zeros(sh.n, 3, device="cuda"), torch.zeros(sh.m, 3, device="cuda")
    off, noff = dev(sh.offset), dev(sh.new_offset)
    idx, d2 = torch.zeros(sh.m, 4, dtype=I32, device="cuda"), torch.zeros(sh.m, 4, device="cuda")
    with pytest.raises(RuntimeError, match="shape"):
        ext.knnquery_cuda(sh.m + 1, 4, xyz, q, off, noff, idx, d2)
    with pytest.raises(RuntimeError, match="int tensor"):
        ext.knnquery_cuda(sh.m, 4, xyz, q, off.long(), noff, idx, d2)
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.knnquery_cuda(sh.m, 4, torch.zeros(3, sh.n, device="cuda").t(), q, off, noff, idx, d2)
    with pytest.raises(RuntimeError, match="CUDA"):
        ext.knnquery_cuda(sh.m, 4, xyz, q.cpu(), off, noff, idx, d2)
    with pytest.raises(RuntimeError, match="nsample"):  # the reference overruns its 100-entry arrays
        ext.knnquery_cuda(sh.m, 101, xyz, q, off, noff, torch.zeros(sh.m, 101, dtype=I32, device="cuda"),
                          torch.zeros(sh.m, 101, device="cuda"))
    with pytest.raises(RuntimeError, match="multiple"):
        z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
        ext.aggregation_forward_cuda(8, 2, 5, 2, z(8, 5), z(8, 2, 5), z(8, 2, 2), torch.zeros(8, 2, dtype=I32, device="cuda"), z(8, 5))
    assert not idx.any() and not d2.any()


# ---- deterministic mode ---------------------------------------------------------------------------------------------------
def test_deterministic_mode_refuses_the_scatters_only(ext):
    """the four entry points with an fp32-atomic scatter raise and write nothing; the forward passes run, and so do the
    fixed-order gradients (grad_input1, grad_position, grad_weight) when the scatter target is None"""
    import p2p_bridge_amd

    c, w_c, k = 5, 5, 3
    rng = np.random.default_rng(80)
    idx_g, idx_n = rng.integers(0, 100, (M, NS)).astype(np.int32), rng.integers(0, 60, (N, NS)).astype(np.int32)
    idx_k, w_k = rng.integers(0, M, (N, k)).astype(np.int32), sixteenths(rng, N, k)
    feat, gout_g = ints(rng, N, c), ints(rng, M, NS, c)
    in1, in2, gout_s = ints(rng, N, c), ints(rng, N, c), ints(rng, N, NS, c)
    inp, pos, w, gout_a = ints(rng, N, c), ints(rng, N, NS, c), sixteenths(rng, N, NS, w_c), ints(rng, N, c)
    zeros = lambda *s: torch.zeros(*s, dtype=F32, device="cuda")  # noqa: E731
    with p2p_bridge_amd.deterministic():
        targets = [zeros(N, c) for _ in range(4)] + [zeros(M, c)]
        with pytest.raises(RuntimeError, match="deterministic"):
            ext.grouping_backward_cuda(M, NS, c, dev(gout_g), dev(idx_g), targets[0])
        with pytest.raises(RuntimeError, match="deterministic"):
            ext.interpolation_backward_cuda(N, c, k, dev(feat), dev(idx_k), dev(w_k), targets[4])
        with pytest.raises(RuntimeError, match="deterministic"):
            ext.subtraction_backward_cuda(N, NS, c, dev(idx_n), dev(gout_s), targets[1], targets[2])
        gp, gw = zeros(N, NS, c), zeros(N, NS, w_c)
        with pytest.raises(RuntimeError, match="deterministic"):
            ext.aggregation_backward_cuda(N, NS, c, w_c, dev(inp), dev(pos), dev(w), dev(idx_n), dev(gout_a), targets[3], gp, gw)
        assert not any(bool(t.any()) for t in targets + [gp, gw])  # a refused call writes nothing

        out = zeros(M, NS, c)
        ext.grouping_forward_cuda(M, NS, c, dev(feat), dev(idx_g), out)
        same_bits(out, feat[idx_g], "grouping_forward")
        zc = np.zeros((N, c), np.float32)
        rsub, r1, _ = subtraction_refs(in1, in2, idx_n, gout_s, zc, zc)
        out = zeros(N, NS, c)
        ext.subtraction_forward_cuda(N, NS, c, dev(in1), dev(in2), dev(idx_n), out)
        same_bits(out, rsub.astype(np.float32), "subtraction_forward")
        ragg, _, rgp, rgw = aggregation_refs(inp, pos, w, idx_n, gout_a, zc, zc, np.zeros((N, NS, w_c), np.float32))
        out = zeros(N, c)
        ext.aggregation_forward_cuda(N, NS, c, w_c, dev(inp), dev(pos), dev(w), dev(idx_n), out)
        same_bits(out, ragg.astype(np.float32), "aggregation_forward")
        rint, _ = interpolation_refs(ints(np.random.default_rng(81), M, c), idx_k, w_k, feat, zc, np.zeros((M, c), np.float32))
        out = zeros(N, c)
        ext.interpolation_forward_cuda(N, c, k, dev(ints(np.random.default_rng(81), M, c)), dev(idx_k), dev(w_k), out)
        same_bits(out, rint.astype(np.float32), "interpolation_forward")

        g1 = zeros(N, c)
        ext.subtraction_backward_cuda(N, NS, c, dev(idx_n), dev(gout_s), g1, None)
        same_bits(g1, r1.astype(np.float32), "grad_input1 alone")
        ext.aggregation_backward_cuda(N, NS, c, w_c, dev(inp), dev(pos), dev(w), dev(idx_n), dev(gout_a), None, gp, gw)
        same_bits(gp, rgp.astype(np.float32), "grad_position alone")
        same_bits(gw, rgw.astype(np.float32), "grad_weight alone")
    assert not p2p_bridge_amd._lib.lib().p2pb_get_deterministic()


# ---- chamfer --------------------------------------------------------------------------------------------------------------
def chamfer_clouds():
    rng = np.random.default_rng(90)
    a, b_ = uniform(rng, 2, 300, 3), uniform(rng, 2, 257, 3)
    a[:, 100:110] = a[:, 0:10]  # duplicate points: the lower index must win both ways
    b_[:, 50:60] = a[:, 0:10]
    return a, b_


def test_chamfer_module_is_chamfer_3d_with_the_allocation_inside():
    from p2p_bridge_amd.metric_modules import chamfer, chamfer_3D

    a, b_ = (dev(v) for v in chamfer_clouds())
    d1, d2 = torch.empty(2, 300, device="cuda"), torch.empty(2, 257, device="cuda")
    i1, i2 = torch.empty(2, 300, dtype=I32, device="cuda"), torch.empty(2, 257, dtype=I32, device="cuda")
    assert chamfer_3D.forward(a, b_, d1, d2, i1, i2) == 1
    got = chamfer.forward(a, b_)
    assert isinstance(got, list) and len(got) == 4
    for g, w, what in zip(got, (d1, d2, i1, i2), ("dist1", "dist2", "idx1", "idx2")):
        same_bits(g, w.cpu().numpy(), what)
    assert bool((got[0][:, 100:110] == got[0][:, 0:10]).all()) and bool((got[3][:, 50:60] <= 9).all())
    rng = np.random.default_rng(91)
    gd1, gd2 = dev(uniform(rng, 2, 300)), dev(uniform(rng, 2, 257))
    g1, g2 = torch.zeros_like(a), torch.zeros_like(b_)
    assert chamfer_3D.backward(a, b_, g1, g2, gd1, gd2, i1, i2) == 1
    # (float operands: the gradient's atomics meet, in no fixed order, in the rows that several points chose -- to rounding
    #  here, bit for bit on exact operands in the next test)
    got = chamfer.backward(a, b_, i1, i2, gd1, gd2)
    assert isinstance(got, list) and len(got) == 2
    hits = max(most_hits(i1.cpu().numpy()), most_hits(i2.cpu().numpy())) + 1
    close(got[0], g1.cpu().numpy().astype(np.float64), sum_tol(hits, 8.0), "chamfer.backward grad_xyz1")  # |2 g (x1 - x2)| <= 8
    close(got[1], g2.cpu().numpy().astype(np.float64), sum_tol(hits, 8.0), "chamfer.backward grad_xyz2")


def test_chamfer_module_backward_is_chamfer_3d_backward_bit_for_bit():
    """exact-family operands: lattice clouds k/8 (with the duplicates of chamfer_clouds and the lattice's own equal distances)
    and integer grad_dist in [-8, 8]. Every term 2 g (x1 - x2) is an integer multiple of 1/4 below 2^6 and every sum of a few
    hundred of them is exact in fp32, so the order of the atomic adds does not show: forward and backward must both be
    bit-equal to chamfer_3D's."""
    from p2p_bridge_amd.metric_modules import chamfer, chamfer_3D

    rng = np.random.default_rng(92)
    ka, kb = rng.integers(-8, 9, (2, 300, 3)), rng.integers(-8, 9, (2, 257, 3))
    ka[:, 100:110] = ka[:, 0:10]
    kb[:, 50:60] = ka[:, 0:10]
    a, b_ = dev(cloud(ka)), dev(cloud(kb))
    gd1, gd2 = dev(ints(rng, 2, 300)), dev(ints(rng, 2, 257))
    d1, d2 = torch.empty(2, 300, device="cuda"), torch.empty(2, 257, device="cuda")
    i1, i2 = torch.empty(2, 300, dtype=I32, device="cuda"), torch.empty(2, 257, dtype=I32, device="cuda")
    assert chamfer_3D.forward(a, b_, d1, d2, i1, i2) == 1
    fwd = chamfer.forward(a, b_)
    for g, w, what in zip(fwd, (d1, d2, i1, i2), ("dist1", "dist2", "idx1", "idx2")):
        same_bits(g, w.cpu().numpy(), what)
    for j in range(2):  # and both are the brute-force minimum with the lowest index among equals
        dd = d2_int(ka[j], kb[j])
        same_bits(fwd[0][j], (dd.min(1) / 64.0).astype(np.float32), "dist1 against the integers")
        same_bits(fwd[2][j], dd.argmin(1).astype(np.int32), "idx1 against the integers")
        same_bits(fwd[3][j], dd.argmin(0).astype(np.int32), "idx2 against the integers")
    assert most_hits(i1.cpu().numpy()) > 1 and most_hits(i2.cpu().numpy()) > 1  # (the atomics do collide)
    g1, g2 = torch.zeros_like(a), torch.zeros_like(b_)
    assert chamfer_3D.backward(a, b_, g1, g2, gd1, gd2, i1, i2) == 1
    got = chamfer.backward(a, b_, fwd[2], fwd[3], gd1, gd2)
    same_bits(got[0], g1.cpu().numpy(), "chamfer.backward grad_xyz1")
    same_bits(got[1], g2.cpu().numpy(), "chamfer.backward grad_xyz2")
    # the same from the definition: d dist1_i / d x1_i = 2 (x1_i - x2_idx1[i]), and the mirror terms
    A, Bc = ka / 8.0, kb / 8.0
    G1, G2 = gd1.cpu().numpy().astype(np.float64), gd2.cpu().numpy().astype(np.float64)
    I1, I2 = i1.cpu().numpy(), i2.cpu().numpy()
    for j in range(2):
        t1 = 2 * G1[j][:, None] * (A[j] - Bc[j][I1[j]])
        t2 = 2 * G2[j][:, None] * (Bc[j] - A[j][I2[j]])
        # (accumulated into zero-filled targets like the kernel's: 0 + (-0) = +0, so a zero term leaves the sign the kernel leaves)
        w1 = scatter_add(0.0 + t1, I2[j], -t2)
        w2 = scatter_add(0.0 + t2, I1[j], -t1)
        same_bits(got[0][j], w1.astype(np.float32), "grad_xyz1 from the definition")
        same_bits(got[1][j], w2.astype(np.float32), "grad_xyz2 from the definition")


def test_chamfer_layers_against_float64():
    from p2p_bridge_amd import metrics

    a, b_ = chamfer_clouds()
    x, y = dev(a).requires_grad_(), dev(b_).requires_grad_()
    x64, y64 = t64(a).requires_grad_(), t64(b_).requires_grad_()
    d = ((x64[:, :, None, :] - y64[:, None, :, :]) ** 2).sum(-1)
    d1, d2 = d.min(2)[0], d.min(1)[0]
    l2 = metrics.ChamferDistanceL2()(x, y)
    # a mean of squared distances <= 12, each within MARGIN of float64 (module docstring), and the mean's own rounding
    tol = 2 * MARGIN + sum_tol(2, 12.0)
    assert abs(float(l2.detach()) - float((d1.mean() + d2.mean()).detach())) <= tol
    s1, s2 = metrics.ChamferDistanceL2_split()(x, y)
    assert abs(float(s1.detach()) - float(d1.detach().mean())) <= tol and abs(float(s2.detach()) - float(d2.detach().mean())) <= tol
    l2.backward()
    (d1.mean() + d2.mean()).backward()
    # d/dx = 2 (x - y) / n per chosen pair, |.| <= 4 / 257; a point chosen by `hits` others sums that many terms
    gtol = sum_tol(300, 4.0 / 257)
    close(x.grad, x64.grad.cpu().numpy(), gtol, "ChamferDistanceL2 grad xyz1")
    close(y.grad, y64.grad.cpu().numpy(), gtol, "ChamferDistanceL2 grad xyz2")
    # L1: the duplicates have distance 0, where the square root has no derivative: forward only. Per element, with the fp32
    # squared distance a within MARGIN of the float64 one d: |sqrt a - sqrt d| = |a - d| / (sqrt a + sqrt d) <= MARGIN / sqrt d
    # where d > MARGIN, and <= sqrt |a - d| <= sqrt MARGIN on the few others (the duplicates). The bound on the means is the
    # mean of these, plus the rounding of the fp32 square roots and of the two means of values <= sqrt 12.
    with torch.no_grad():
        l1 = metrics.ChamferDistanceL1()(x, y)

    def sqrt_bound(dd):
        dd = dd.detach()
        return torch.where(dd > MARGIN, MARGIN / dd.clamp_min(MARGIN).sqrt(), torch.full_like(dd, MARGIN ** 0.5)).mean()

    assert int((d1.detach() <= MARGIN).sum()) == 40 and int((d2.detach() <= MARGIN).sum()) == 20  # (the planted duplicates only)
    want = (d1.detach().sqrt().mean() + d2.detach().sqrt().mean()) / 2
    l1_tol = float(sqrt_bound(d1) + sqrt_bound(d2)) / 2 + sum_tol(2, 12.0 ** 0.5)
    print(f"ChamferDistanceL1: |error| = {abs(float(l1) - float(want)):.3g}, bound {l1_tol:.3g}")
    assert abs(float(l1) - float(want)) <= l1_tol


def test_chamfer_ignore_zeros_at_batch_size_one():
    from p2p_bridge_amd import metrics

    a, b_ = chamfer_clouds()
    a, b_ = a[:1].copy(), b_[:1].copy()
    a[0, 200:], b_[0, 180:] = 0.0, 0.0  # padding rows
    kept = metrics.ChamferDistanceL2(ignore_zeros=True)(dev(a), dev(b_))
    want = metrics.ChamferDistanceL2()(dev(a[:, :200]), dev(b_[:, :180]))
    padded = metrics.ChamferDistanceL2()(dev(a), dev(b_))
    assert float(kept) == float(want) and float(kept) != float(padded)
    two = metrics.ChamferDistanceL2(ignore_zeros=True)(dev(np.concatenate([a, a])), dev(np.concatenate([b_, b_])))
    assert abs(float(two) - float(padded)) <= sum_tol(2, 12.0)  # (batch size 2: nothing is dropped)


# ---- the drop-in ----------------------------------------------------------------------------------------------------------
def test_dropin_modules_expose_exactly_the_reference_surface():
    import p2p_bridge_amd

    p2p_bridge_amd.install_dropin()
    import chamfer
    import pointops_cuda

    public = lambda mod: sorted(k for k in vars(mod) if not k.startswith("__"))  # noqa: E731
    assert len(POINTOPS_NAMES) == 13 and public(pointops_cuda) == sorted(POINTOPS_NAMES)
    assert public(chamfer) == sorted(CHAMFER_NAMES)
    assert sys.modules["pointops_cuda"] is pointops_cuda and sys.modules["chamfer"] is chamfer
    # a call through the registered names reaches the kernels
    sh = SHAPES["A"]
    pts, qry = lattice_case("A")
    idx = torch.zeros(sh.m, 3, dtype=I32, device="cuda")
    dist2 = torch.zeros(sh.m, 3, dtype=F32, device="cuda")
    pointops_cuda.knnquery_cuda(sh.m, 3, dev(cloud(pts)), dev(cloud(qry)), dev(sh.offset), dev(sh.new_offset), idx, dist2)
    same_bits(idx, knn_ref(sh, lambda q, p: d2_int(qry[q], pts[p]), 3)[0], "pointops_cuda.knnquery_cuda")
    d1 = chamfer.forward(dev(cloud(pts))[None], dev(cloud(qry))[None])[0]
    same_bits(d1[0], (d2_int(pts, qry).min(1) / 64.0).astype(np.float32), "chamfer.forward dist1")
