"""Grid k-NN on the GPU against the existing brute force: denoise.knn_points(method="brute") / p2pb_knn_points, which
tests/test_denoise_gpu.py pins to scikit-learn. dist2 and idx must agree with it BIT FOR BIT -- there is no tolerance: both
keep the k smallest keys (sqdist3 bits << 32 | index), so ties break by ascending index on both sides."""
import numpy as np
import pytest
import torch

from oracle.poison_arena import PoisonArena
from p2p_bridge_amd import _lib, denoise, image_features, knn_grid
from p2p_bridge_amd.knn_grid import PointGrid

pytestmark = pytest.mark.gpu
I32, U8, F32 = torch.int32, torch.uint8, torch.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def brute(query, ref, k):
    """the yardstick: (dist2 f32[nq,k], idx i64[nq,k]) of the exhaustive search"""
    out = denoise.knn_points(query[None].contiguous(), ref[None].contiguous(), K=k, method="brute")
    return out.dists[0], out.idx[0]


def same_bits(got, want):
    """(dist2, idx) pairs equal bit for bit (the distances compared as their int32 patterns: -0 / NaN cannot hide)"""
    assert got[0].dtype == F32 and got[1].dtype == torch.int64 and got[0].shape == want[0].shape == got[1].shape
    assert torch.equal(got[1], want[1]), f"{int((got[1] != want[1]).any(1).sum())} of {got[1].shape[0]} index rows differ"
    assert torch.equal(got[0].view(I32), want[0].view(I32))


# ---- the clouds --------------------------------------------------------------------------------------------------
def lattice(shift):
    """12^3 points at spacing 0.25 (exact in fp32, shifted or not), rows shuffled with a fixed seed"""
    g = np.arange(12, dtype=np.float64) * 0.25
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    pts = pts[np.random.default_rng(12).permutation(len(pts))] + np.asarray(shift, dtype=np.float64)
    assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts)
    return pts.astype(np.float32)


def lattice_queries(pts, cell, shift):
    """all lattice points, 100 corners of the grid's cells and 100 points on its cell faces (one coordinate a multiple of the
    cell edge, as fp32 rounds it: either side of the face), inside the lattice's box"""
    rng = np.random.default_rng(34)
    lo = np.asarray(shift, dtype=np.float64)
    c0 = np.floor(lo / cell)
    span = int(np.ceil(2.75 / cell)) + 1
    corners = (c0 + rng.integers(0, span + 1, (100, 3))) * cell
    faces = lo + rng.uniform(0.0, 2.75, (100, 3))
    axis = rng.integers(0, 3, 100)
    faces[np.arange(100), axis] = (c0[axis] + rng.integers(0, span + 1, 100)) * cell
    return np.concatenate([pts, corners.astype(np.float32), faces.astype(np.float32)])


def surface(n_sphere=20000, n_plane=5000, n_far=30, seed=5):
    """a unit sphere shell and a plane patch of the same density below it, and n_far isolated points at distances 5..40
    -> (points f32[n,3] in that order, half edge of the patch)"""
    rng = np.random.default_rng(seed)
    s = rng.normal(size=(n_sphere, 3))
    s /= np.linalg.norm(s, axis=1, keepdims=True)
    half = 0.5 * np.sqrt(n_plane / (n_sphere / (4.0 * np.pi)))
    p = np.concatenate([rng.uniform(-half, half, (n_plane, 2)), np.full((n_plane, 1), -1.6)], 1)
    d = rng.normal(size=(n_far, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    far = d * np.linspace(5.0, 40.0, n_far)[:, None]
    return np.concatenate([s, p, far]).astype(np.float32), float(half)


@pytest.fixture(scope="module")
def shell():
    """case 3's cloud, its queries (the 30 isolated points first, then 3000 of the others) and the brute results per k:
    computed once and only read"""
    pts, half = surface()
    n_surf = len(pts) - 30
    pick = np.sort(np.random.default_rng(6).choice(n_surf, 3000, replace=False))
    rows = np.concatenate([np.arange(n_surf, len(pts)), pick])
    ref, query = dev(pts), dev(pts[rows])
    return {"pts": pts, "half": half, "rows": rows, "ref": ref, "query": query,
            "brute": {k: brute(query, ref, k) for k in (10, 20, 65, 128)}}


# ---- 1. ties -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [(0.0, 0.0, 0.0), (50.0, -50.0, 50.0)], ids=["origin", "shifted"])
@pytest.mark.parametrize("k", [1, 7, 10, 64, 65, 128])
def test_tie_lattice(k, shift):
    """every neighbour shell of a cubic lattice is a set of exact ties (6, 12, 8, 6, 24, ... points): k = 10, 64, 65, 128 cut
    through one, 64 / 65 on either side of the list's register boundary; the shifted copy has negative cells and quotients
    that round"""
    pts = lattice(shift)
    ref = dev(pts)
    grid = PointGrid(ref, k)
    query = dev(lattice_queries(pts, grid.cell, shift))
    want = brute(query, ref, k)
    if k in (10, 64, 65, 128):  # the case is what it claims: most rows tie across the k-th place
        wide = brute(query, ref, k + 1)[0]
        assert float((wide[:, k - 1] == wide[:, k]).float().mean()) > 0.5
    got = grid.knn(query, k, return_stats=True)
    print(f"lattice k={k} shift={shift}: cell {grid.cell:.4f} stats {got[2]}")
    same_bits(got[:2], want)
    assert sum(got[2]["ring"]) + got[2]["brute"] == query.shape[0]


# ---- 2. coincident points ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 128])
def test_coincident_points(k):
    """more than k points at distance 0: the indices are the k lowest rows among the copies"""
    rng = np.random.default_rng(7)
    pts = np.concatenate([np.tile([[0.3, -1.2, 2.5]], (300, 1)), rng.uniform(-3, 3, (40, 3))])
    pts = pts[rng.permutation(len(pts))].astype(np.float32)
    ref = dev(pts)
    got = knn_grid.knn(ref, ref, k)
    same_bits(got, brute(ref, ref, k))
    copies = np.nonzero((pts == np.array([0.3, -1.2, 2.5], dtype=np.float32)).all(1))[0]
    assert len(copies) == 300
    row = got[1][int(copies[5])].cpu().numpy()
    assert np.array_equal(row, copies[:k]) and float(got[0][int(copies[5])].abs().max()) == 0.0


# ---- 3. a surface with isolated points ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 20, 128])
def test_surface_with_isolated_points(shell, k):
    grid = PointGrid(shell["ref"], k)
    dist2, idx, stats = grid.knn(shell["query"], k, return_stats=True)
    same_bits((dist2, idx), shell["brute"][k])
    # the surface queries that may need more than the first level: points of the patch within three cell edges of its boundary
    q = shell["pts"][shell["rows"][30:]]
    on_patch = q[:, 2] == np.float32(-1.6)
    near_edge = int((on_patch & (np.abs(q[:, :2]).max(1) > shell["half"] - 3.0 * grid.cell)).sum())
    print(f"surface k={k}: cell {grid.cell:.4f} stats {stats} surface queries near the patch boundary {near_edge}")
    assert stats["brute"] <= 30
    assert stats["ring"][0] >= 3000 - near_edge
    assert sum(stats["ring"]) + stats["brute"] == 3030


def test_coarser_levels_resolve_what_the_first_leaves(shell, monkeypatch):
    """with the pair threshold out of the way the open queries repeat on the grids 4x and 16x coarser (built on first use,
    kept on the object) before the full walk: the same bits, whichever stage found a row"""
    monkeypatch.setattr(knn_grid, "KNN_BRUTE_PAIRS", 0)
    fitted = PointGrid(shell["ref"], 10).cell
    grid = PointGrid(shell["ref"], 10, cell=fitted / 8.0)
    dist2, idx, stats = grid.knn(shell["query"], 10, return_stats=True)
    print(f"levels: cell {grid.cell:.5f} stats {stats}")
    same_bits((dist2, idx), shell["brute"][10])
    assert len(grid._levels) == 3 and grid.level(2)[3] == pytest.approx(16.0 * grid.cell, rel=1e-6)
    assert stats["ring"][1] > 0 and sum(stats["ring"]) + stats["brute"] == 3030
    levels = [lv[0].data_ptr() for lv in grid._levels]
    same_bits(grid.knn(shell["query"], 10), shell["brute"][10])  # (again: the cached levels)
    assert [lv[0].data_ptr() for lv in grid._levels] == levels


# ---- 4. edges ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,nq", [(10, 10, 5), (11, 10, 5), (65, 65, 3), (129, 128, 4), (500, 7, 1)])
def test_small_counts(n, k, nq):
    rng = np.random.default_rng(n + k)
    ref, query = dev(rng.normal(size=(n, 3))), dev(rng.normal(size=(nq, 3)))
    same_bits(knn_grid.knn(query, ref, k), brute(query, ref, k))


def test_queries_far_outside_the_box():
    rng = np.random.default_rng(8)
    ref = dev(rng.uniform(0, 1, (2000, 3)))
    q = np.concatenate([rng.uniform(-0.2, 1.2, (50, 3)), rng.uniform(-1, 1, (20, 3)) * 100.0, [[1e6, -1e6, 3.0], [-5e4, 0, 0]]])
    query = dev(q)
    dist2, idx, stats = PointGrid(ref, 10).knn(query, 10, return_stats=True)
    same_bits((dist2, idx), brute(query, ref, 10))
    assert stats["brute"] >= 1


def test_query_cell_outside_the_key_range():
    """a tight cluster far from the origin under an explicit tiny cell: its cell indices stay below 2^20, the cell of one
    query does not -- that query is nobody's ring and must come back from the full walk"""
    rng = np.random.default_rng(9)
    ref = dev(1000.0 + rng.uniform(0, 0.01, (2000, 3)))
    q = np.concatenate([1000.0 + rng.uniform(0.002, 0.008, (40, 3)), [[3000.0, 1000.0, 1000.0]]])
    query = dev(q)
    grid = PointGrid(ref, 5, cell=2e-3)
    dist2, idx, stats = grid.knn(query, 5, return_stats=True)
    print(f"key range: stats {stats}")
    same_bits((dist2, idx), brute(query, ref, 5))
    assert stats["brute"] >= 1
    # the entry point alone: the query is reported unresolved
    pts, skeys, rows, cell = grid.level(0)
    d2, ix = torch.empty(41, 5, dtype=F32, device="cuda"), torch.empty(41, 5, dtype=I32, device="cuda")
    un = torch.empty(41, dtype=U8, device="cuda")
    _lib.call("p2pb_knn_grid", 41, 2000, 5, 3, None, _lib.ptr(query), _lib.ptr(pts), _lib.ptr(skeys), _lib.ptr(rows), cell,
              _lib.ptr(d2), _lib.ptr(ix), _lib.ptr(un), _lib.stream_ptr())
    assert int(un[40]) == 1 and set(un.tolist()) <= {0, 1}


def test_refusals():
    ref = dev(np.random.default_rng(10).normal(size=(50, 3)))
    with pytest.raises(ValueError, match="exceeds the 50 points"):
        knn_grid.knn(ref, ref, 51)
    with pytest.raises(ValueError, match="exceeds the 50 points"):
        PointGrid(ref, 10).knn(ref, 51)
    bad = ref.clone()
    bad[17, 1] = float("nan")
    with pytest.raises(ValueError):
        PointGrid(bad, 10)
    with pytest.raises(ValueError):
        PointGrid(bad, 10, cell=0.5)
    with pytest.raises(ValueError):
        PointGrid(ref * 1e4, 10, cell=1e-3)  # cell indices beyond 2^20
    with pytest.raises(RuntimeError):
        PointGrid(ref, 10).knn(ref.double(), 5)
    with pytest.raises(RuntimeError):
        PointGrid(ref, 10).knn(ref[::2], 5)  # not contiguous
    d2, ix = PointGrid(ref, 10).knn(ref[:0], 5)
    assert d2.shape == (0, 5) and ix.shape == (0, 5) and ix.dtype == torch.int64


# ---- 5. forced stages --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 65])
def test_forced_stages_give_the_same_bits(k):
    pts, _ = surface(4000, 1000, 0, seed=11)  # (no far points: every cell index at the tiny edge stays below 2^20)
    ref = dev(pts)
    fitted = PointGrid(ref, k).knn(ref, k, return_stats=True)
    same_bits(fitted[:2], brute(ref, ref, k))
    tiny = PointGrid(ref, k, cell=1e-5).knn(ref, k, return_stats=True)  # (k >= 2: no ring of such cells holds a second point)
    huge = PointGrid(ref, k, cell=100.0).knn(ref, k, return_stats=True)  # one cell holds everything
    print(f"forced k={k}: fitted {fitted[2]} tiny {tiny[2]} huge {huge[2]}")
    assert tiny[2] == {"ring": [0, 0, 0], "brute": len(pts)}
    assert huge[2] == {"ring": [len(pts), 0, 0], "brute": 0}
    same_bits(tiny[:2], fitted[:2])
    same_bits(huge[:2], fitted[:2])


# ---- 6. consumers ------------------------------------------------------------------------------------------------
def test_knn_points_grid_equals_brute():
    rng = np.random.default_rng(13)
    p2 = torch.stack([dev(surface(3000, 800, 5, seed=14)[0]), dev(rng.normal(size=(3805, 3)))])
    p1 = torch.stack([p2[0, ::7][:400], dev(rng.normal(size=(400, 3)))]).contiguous()
    want = denoise.knn_points(p1, p2, K=16, return_nn=True)
    got = denoise.knn_points(p1, p2, K=16, return_nn=True, method="grid")
    assert type(got) is type(want) and got.idx.dtype == torch.int64 and got.knn.shape == (2, 400, 16, 3)
    assert torch.equal(got.idx, want.idx)
    assert torch.equal(got.dists.view(I32), want.dists.view(I32)) and torch.equal(got.knn.view(I32), want.knn.view(I32))
    assert denoise.knn_points(p1, p2, K=3, method="grid").knn is None


def test_fill_stage_grid_equals_brute():
    """4 000 points, 8 channels, 30 % unobserved with a block of 200 adjacent unobserved points (their neighbours are
    unobserved too: several rounds): the same feature bits in the same number of rounds"""
    rng = np.random.default_rng(15)
    pts, _ = surface(3200, 800, 0, seed=16)
    n = len(pts)
    seen = rng.uniform(size=n) > 0.3 - 200.0 / n
    seen[np.argsort(((pts - pts[100]) ** 2).sum(1))[:200]] = False
    count = torch.from_numpy(seen.astype(np.int32) * 3).cuda()
    feats = torch.from_numpy((rng.uniform(0.1, 1.0, (n, 8)) * seen[:, None]).astype(np.float16)).cuda()
    points = dev(pts)
    a, rounds_a = image_features.interpolate_missing_features(feats.clone(), count, points, return_rounds=True)
    b, rounds_b = image_features.interpolate_missing_features(feats.clone(), count, points, return_rounds=True,
                                                              neighbours="grid")
    assert 0.25 < 1.0 - seen.mean() < 0.37 and rounds_a > 1
    assert rounds_a == rounds_b
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert not torch.equal(a, feats)


# ---- 7. memory discipline ----------------------------------------------------------------------------------------
def test_entry_points_inside_a_poisoned_arena(shell):
    """both entry points on case 3 with k = 65 (two registers per lane, the second half empty): nothing is written outside the
    outputs, the rows of unresolved queries keep the poison after the ring search alone, every row is written after the walk"""
    k, n, nq = 65, shell["ref"].shape[0], shell["query"].shape[0]
    pts, skeys, rows, cell = PointGrid(shell["ref"], k).level(0)
    want_d, want_i = shell["brute"][k]
    call, ptr = _lib.call, _lib.ptr
    with PoisonArena("cuda:0", 64 << 20) as arena:
        query, ref, pts, skeys, rows = (arena.put(t) for t in (shell["query"], shell["ref"], pts, skeys, rows))
        dist2, idx = torch.empty(nq, k, dtype=F32, device="cuda:0"), torch.empty(nq, k, dtype=I32, device="cuda:0")
        unresolved = torch.empty(nq, dtype=U8, device="cuda:0")
        assert arena.n_allocations >= 8  # (the outputs came out of the arena too)
        call("p2pb_knn_grid", nq, n, k, 3, None, ptr(query), ptr(pts), ptr(skeys), ptr(rows), cell, ptr(dist2), ptr(idx),
             ptr(unresolved), _lib.stream_ptr())
        arena.check_guards()
        assert set(unresolved.tolist()) <= {0, 1}
        open_ = unresolved.bool()
        assert 30 <= int(open_.sum()) < nq and bool(open_[:30].all())  # (the isolated points come first)
        assert bool((idx[open_] == -1).all()) and bool(torch.isnan(dist2[open_]).all())  # the poison, untouched
        assert torch.equal(idx[~open_].long(), want_i[~open_])
        assert torch.equal(dist2[~open_].view(I32), want_d[~open_].view(I32))
        left = arena.put(torch.nonzero(open_).flatten().to(I32))
        call("p2pb_knn_grid_brute", left.numel(), n, k, ptr(left), ptr(query), ptr(ref), ptr(dist2), ptr(idx),
             _lib.stream_ptr())
        arena.check_guards()
        arena.assert_written(dist2, "dist2")
        assert torch.equal(idx.long(), want_i) and torch.equal(dist2.view(I32), want_d.view(I32))
