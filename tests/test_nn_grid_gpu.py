"""Grid nearest point / Chamfer on the GPU against the code it restates: metrics.chamfer_3DDist (csrc/chamfer.hip, every pair)
and PointGrid.knn(., 1). Distances are compared as their int32 patterns, indices by torch.equal: there is no tolerance
anywhere -- all three keep the smallest key (sqdist3 bits << 32 | row), so the lowest row wins a tie on every side."""
import numpy as np
import pytest
import torch

from oracle.poison_arena import PoisonArena
from p2p_bridge_amd import _lib, knn_grid, metrics
from p2p_bridge_amd.knn_grid import PointGrid
from test_knn_grid_gpu import dev, lattice, lattice_queries, surface

pytestmark = pytest.mark.gpu
I32, I64, U8, F32 = torch.int32, torch.int64, torch.uint8, torch.float32


def brute(query, ref):
    """the yardstick: (dist2 f32[nq], idx i64[nq]) of csrc/chamfer.hip, query -> ref"""
    d1, _, i1, _ = metrics.chamfer_3DDist()(query[None], ref[None])
    assert i1.dtype == I32
    return d1[0], i1[0].long()


def same_bits(got, want):
    assert got[0].dtype == F32 and got[1].dtype == I64 and got[0].shape == want[0].shape == got[1].shape and got[0].dim() == 1
    assert torch.equal(got[1], want[1]), f"{int((got[1] != want[1]).sum())} of {got[1].shape[0]} indices differ"
    assert torch.equal(got[0].view(I32), want[0].view(I32))


def check(grid, query, **kw):
    """nearest == knn(., 1) squeezed == the Chamfer kernel; -> (dist2, idx, stats)"""
    d2, ix, stats = grid.nearest(query, return_stats=True, **kw)
    kd, ki = grid.knn(query, 1)
    assert kd.shape == (query.shape[0], 1)
    same_bits((d2, ix), (kd[:, 0], ki[:, 0]))
    same_bits((d2, ix), brute(query, grid.ref))
    assert sum(stats["ring"]) + stats["brute"] == query.shape[0]
    return d2, ix, stats


def entry(nq, grid, query, qidx, dist2, idx, unresolved, level=0):
    pts, skeys, rows, cell = grid.level(level)
    _lib.call("p2pb_nn_grid", nq, grid.ref.shape[0], 3, _lib.ptr(qidx), _lib.ptr(query), _lib.ptr(pts), _lib.ptr(skeys),
              _lib.ptr(rows), cell, _lib.ptr(dist2), _lib.ptr(idx), _lib.ptr(unresolved), _lib.stream_ptr())


def poisoned(nq):
    return (torch.full((nq,), float("nan"), dtype=F32, device="cuda"), torch.full((nq,), -1, dtype=I32, device="cuda"),
            torch.full((nq,), 255, dtype=U8, device="cuda"))


@pytest.fixture(scope="module")
def shell():
    """case 4's cloud (20 000 sphere + 5 000 plane + 30 isolated points), its queries (every surface point moved by seeded noise
    of 0.01; the 30 isolated points, which come last, moved out by half their distance from the origin: nothing within 2.5 of
    them, far beyond three rings of cells fitted to the surface) and the brute result: computed once and only read"""
    pts, _ = surface()
    q = pts.astype(np.float64) + 0.01 * np.random.default_rng(21).normal(size=pts.shape)
    q[-30:] = pts[-30:].astype(np.float64) * 1.5
    ref, query = dev(pts), dev(q)
    return {"ref": ref, "query": query, "brute": brute(query, ref)}


# ---- 1. ties -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [(0.0, 0.0, 0.0), (50.0, -50.0, 50.0)], ids=["origin", "shifted"])
def test_tie_lattice(shift):
    pts = lattice(shift)
    ref = dev(pts)
    grid = PointGrid(ref, 1)
    _, _, stats = check(grid, dev(lattice_queries(pts, grid.cell, shift)))
    print(f"lattice shift={shift}: cell {grid.cell:.4f} stats {stats}")
    # the lattice moved by half a spacing along x: the two lattice neighbours along x are exactly equidistant
    moved = pts.astype(np.float64) + np.array([0.125, 0.0, 0.0])
    assert np.array_equal(moved.astype(np.float32).astype(np.float64), moved)
    d = ((moved[:, None, :] - pts.astype(np.float64)[None, :, :]) ** 2).sum(-1)  # exact in fp64: multiples of 2^-6
    nearest = d.min(1)
    assert ((d == nearest[:, None]).sum(1) >= 2).mean() > 0.5
    d2, ix, _ = check(grid, dev(moved))
    assert np.array_equal(ix.cpu().numpy(), d.argmin(1))  # (argmin: the first = lowest row among the equal)
    assert np.array_equal(d2.cpu().numpy().astype(np.float64), nearest)


# ---- 2. coincident points ----------------------------------------------------------------------------------------
def test_coincident_points():
    rng = np.random.default_rng(7)
    pts = np.concatenate([np.tile([[0.3, -1.2, 2.5]], (300, 1)), rng.uniform(-3, 3, (40, 3))])
    pts = pts[rng.permutation(len(pts))].astype(np.float32)
    ref = dev(pts)
    d2, ix, _ = check(PointGrid(ref, 1), ref)
    copies = np.nonzero((pts == np.array([0.3, -1.2, 2.5], dtype=np.float32)).all(1))[0]
    assert len(copies) == 300
    assert bool((ix[torch.from_numpy(copies).cuda()] == int(copies[0])).all())
    assert torch.equal(d2.view(I32), torch.zeros_like(d2).view(I32))  # (+0, every point has itself or a copy)


# ---- 3. counts around the wave -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 500])
@pytest.mark.parametrize("nq", [1, 63, 64, 65, 257])
def test_counts_around_the_wave(nq, n):
    rng = np.random.default_rng(1000 * n + nq)
    ref, query = dev(rng.normal(size=(n, 3))), dev(rng.normal(size=(nq, 3)))
    grid = PointGrid(ref, 1)
    want = check(grid, query)
    # the entry point alone on a strict subset of the queries, in a shuffled order
    sub = torch.from_numpy(rng.permutation(nq)[:max(1, nq - 1 - nq // 3)].astype(np.int32)).cuda()
    d2, ix, un = poisoned(nq)
    entry(sub.numel(), grid, query, sub, d2, ix, un)
    inside = torch.zeros(nq, dtype=torch.bool, device="cuda")
    inside[sub.long()] = True
    assert bool((un[~inside] == 255).all()) and set(un[inside].tolist()) <= {0, 1}
    done = inside & (un == 0)
    assert bool((ix[~done] == -1).all()) and bool(torch.isnan(d2[~done]).all())  # the poison, untouched
    assert torch.equal(ix[done].long(), want[1][done]) and torch.equal(d2[done].view(I32), want[0][done].view(I32))


# ---- 4. order ----------------------------------------------------------------------------------------------------
def test_order_cannot_change_a_bit(shell):
    grid, query, nq = PointGrid(shell["ref"], 1), shell["query"], shell["query"].shape[0]
    d2, ix, stats = grid.nearest(query, return_stats=True)
    print(f"order: cell {grid.cell:.4f} stats {stats}")
    same_bits((d2, ix), shell["brute"])
    kd, ki = grid.knn(query, 1)
    same_bits((d2, ix), (kd[:, 0], ki[:, 0]))
    assert stats["ring"][0] > nq // 2 and sum(stats["ring"]) + stats["brute"] == nq
    identity = torch.arange(nq, dtype=I32, device="cuda")
    shuffled = torch.from_numpy(np.random.default_rng(22).permutation(nq).astype(np.int32)).cuda()
    for order in (identity, shuffled, identity.flip(0).contiguous()):
        got = grid.nearest(query, order=order, return_stats=True)
        same_bits(got[:2], shell["brute"])
        assert got[2] == stats
    with pytest.raises(ValueError, match="permutation"):
        grid.nearest(query, order=torch.zeros(nq, dtype=I32, device="cuda"))
    with pytest.raises(ValueError, match="permutation"):
        grid.nearest(query, order=identity + 1)
    with pytest.raises(ValueError):
        grid.nearest(query, order=identity[:-1].contiguous())
    with pytest.raises(RuntimeError):
        grid.nearest(query, order=identity.long())


# ---- 5. stages ---------------------------------------------------------------------------------------------------
def test_forced_stages_give_the_same_bits():
    """queries 0.05 off the surface along its normal. Sphere queries lie at radius 1.05: at least 0.05 from every sphere
    point and 0.55 above the plane (z = -1.6 against z >= -1.05); plane queries lie at z = -1.65: 0.05 below the plane and
    0.65 below the sphere. The fp32 rounding of coordinates below 2 moves a distance by less than 1e-6, so every nearest
    distance is above 0.0499, a hundred times the 4.8e-4 that three rings of the coarsest tiny cells reach."""
    pts, _ = surface(4000, 1000, 0, seed=11)
    q = pts.astype(np.float64)
    q[:4000] *= 1.05
    q[4000:, 2] -= 0.05
    ref, query = dev(pts), dev(q)
    nq = len(q)
    want = brute(query, ref)
    assert float(want[0].min()) >= 0.0499 ** 2
    assert 3 * 16 * 1e-5 < 0.0499
    fitted = check(PointGrid(ref, 1), query)
    tiny = check(PointGrid(ref, 1, cell=1e-5), query)
    huge = check(PointGrid(ref, 1, cell=100.0), query)
    print(f"forced: fitted {fitted[2]} tiny {tiny[2]} huge {huge[2]}")
    assert tiny[2] == {"ring": [0, 0, 0], "brute": nq}
    assert huge[2] == {"ring": [nq, 0, 0], "brute": 0}
    assert sum(fitted[2]["ring"]) + fitted[2]["brute"] == nq
    for got in (fitted, tiny, huge):
        same_bits(got[:2], want)


def test_coarser_levels_resolve_what_the_first_leaves(shell, monkeypatch):
    """with the pair threshold out of the way the open queries repeat on the grids 4x and 16x coarser before the full walk"""
    monkeypatch.setattr(knn_grid, "KNN_BRUTE_PAIRS", 0)
    grid = PointGrid(shell["ref"], 1, cell=PointGrid(shell["ref"], 1).cell / 8.0)
    d2, ix, stats = grid.nearest(shell["query"], return_stats=True)
    print(f"levels: cell {grid.cell:.5f} stats {stats}")
    same_bits((d2, ix), shell["brute"])
    assert len(grid._levels) == 3 and stats["ring"][1] > 0 and sum(stats["ring"]) + stats["brute"] == shell["query"].shape[0]


# ---- 6. range ----------------------------------------------------------------------------------------------------
def test_queries_far_outside_the_box():
    rng = np.random.default_rng(8)
    ref = dev(rng.uniform(0, 1, (2000, 3)))
    q = np.concatenate([rng.uniform(-0.2, 1.2, (50, 3)), rng.uniform(-1, 1, (20, 3)) * 100.0, [[1e6, -1e6, 3.0], [-5e4, 0, 0]]])
    _, _, stats = check(PointGrid(ref, 1), dev(q))
    assert stats["brute"] >= 1


def test_query_cell_outside_the_key_range():
    """a tight cluster far from the origin under an explicit tiny cell: the cell of one query lies beyond 2^20 -- the entry
    point reports it unresolved, nearest() answers it from the full walk"""
    rng = np.random.default_rng(9)
    ref = dev(1000.0 + rng.uniform(0, 0.01, (2000, 3)))
    query = dev(np.concatenate([1000.0 + rng.uniform(0.002, 0.008, (40, 3)), [[3000.0, 1000.0, 1000.0]]]))
    grid = PointGrid(ref, 1, cell=2e-3)
    _, _, stats = check(grid, query)
    assert stats["brute"] >= 1
    d2, ix, un = poisoned(41)
    entry(41, grid, query, None, d2, ix, un)
    assert int(un[40]) == 1 and set(un.tolist()) <= {0, 1} and int(ix[40]) == -1 and bool(torch.isnan(d2[40]))
    assert int((un == 0).sum()) > 0


def test_empty_query_and_refusals():
    ref = dev(np.random.default_rng(10).normal(size=(50, 3)))
    grid = PointGrid(ref, 1)
    d2, ix, stats = grid.nearest(ref[:0], return_stats=True)
    assert d2.shape == (0,) and ix.shape == (0,) and ix.dtype == I64 and d2.dtype == F32
    assert stats == {"ring": [0, 0, 0], "brute": 0}
    with pytest.raises(RuntimeError):
        grid.nearest(ref.double())
    with pytest.raises(RuntimeError):
        grid.nearest(ref[::2])  # not contiguous
    with pytest.raises(RuntimeError):
        grid.nearest(ref.cpu())
    with pytest.raises(ValueError):
        grid.nearest(ref[:, :2].contiguous())


# ---- 7. chamfer_grid ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair():
    """xyz1 f32[2,4000,3]: a noisy copy of 4 000 points of xyz2 f32[2,5000,3], two different surfaces"""
    clouds, copies = [], []
    for b in range(2):
        pts, _ = surface(4000 - 500 * b, 1000 + 500 * b, 0, seed=31 + b)
        rng = np.random.default_rng(33 + b)
        copies.append(pts[rng.permutation(5000)[:4000]] + 0.02 * rng.normal(size=(4000, 3)))
        clouds.append(pts)
    return dev(np.stack(copies)), dev(np.stack(clouds))


def same_four(got, want):
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.device == w.device
        assert torch.equal(g.view(I32), w.view(I32))


def test_chamfer_grid_equals_chamfer_3ddist(pair):
    xyz1, xyz2 = pair
    want = metrics.chamfer_3DDist()(xyz1, xyz2)
    assert want[0].shape == (2, 4000) and want[3].shape == (2, 5000) and want[2].dtype == I32
    same_four(metrics.chamfer_grid(xyz1, xyz2), want)
    one = metrics.chamfer_3DDist()(xyz1[1:], xyz2[1:])
    g1, g2 = PointGrid(xyz1[1], 1), PointGrid(xyz2[1], 1)
    same_four(metrics.chamfer_grid(xyz1[1:], xyz2[1:], grid1=g1, grid2=g2), one)
    same_four(metrics.chamfer_grid(xyz1[1:], xyz2[1:], grid2=g2), one)
    with pytest.raises(ValueError):
        metrics.chamfer_grid(xyz1, xyz2, grid2=g2)  # B = 2
    with pytest.raises(ValueError):
        metrics.chamfer_grid(xyz1[:1], xyz2[:1], grid2=g2)  # another cloud's grid
    with pytest.raises(RuntimeError, match="grad"):
        metrics.chamfer_grid(xyz1.clone().requires_grad_(), xyz2)
    bad = xyz1.clone()
    bad[1, 17, 2] = float("nan")
    with pytest.raises(ValueError):
        metrics.chamfer_grid(bad, xyz2)
    with pytest.raises(ValueError):
        metrics.chamfer_grid(xyz2, bad)


# ---- 8. cd_unit_sphere -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [True, False])
def test_cd_unit_sphere_grid_returns_the_same_floats(pair, normalize):
    gen, ref = pair[0][:1] * 3.0 + 2.0, pair[1][:1] * 3.0 + 2.0
    want = metrics.cd_unit_sphere(gen, ref, normalize=normalize)
    assert want == metrics.cd_unit_sphere(gen, ref, normalize=normalize, method="brute")
    assert all(type(v) is float and v > 0 for v in want)
    assert metrics.cd_unit_sphere(gen, ref, normalize=normalize, method="grid") == want
    index = metrics.cloud_point_grid(ref[0], normalize=normalize)
    assert isinstance(index, PointGrid)
    assert metrics.cd_unit_sphere(gen, ref, normalize=normalize, method="grid", ref_grid=index) == want
    with pytest.raises(ValueError):  # the index of the other normalisation
        metrics.cd_unit_sphere(gen, ref, normalize=not normalize, method="grid", ref_grid=index)
    with pytest.raises(ValueError):
        metrics.cd_unit_sphere(gen, ref, normalize=normalize, ref_grid=index)


# ---- 9. evaluate_rooms -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [False, True])
def test_evaluate_rooms_scores_the_same_csv(tmp_path, monkeypatch, normalize):
    from p2p_bridge_amd import evaluate_rooms as er
    from test_evaluate_rooms_gpu import write_ply_ascii
    from test_metrics_unit_sphere_gpu import icosphere

    verts, faces = icosphere(3)
    verts = (verts * 2.0 + torch.tensor([1.0, -2.0, 0.5])).double().numpy()
    rng = np.random.default_rng(41)

    def noisy(n, sigma):
        p = rng.normal(size=(n, 3))
        return p / np.linalg.norm(p, axis=1, keepdims=True) * 2.0 + [1.0, -2.0, 0.5] + sigma * rng.normal(size=(n, 3))

    iphone, good, more = noisy(600, 0.05), noisy(600, 0.01), noisy(900, 0.02)  # `more` is reduced to 600 points by FPS
    seen, grids = [], []
    real_scene, real_cd = er.calculate_model_metrics, metrics.cd_unit_sphere
    monkeypatch.setattr(er, "calculate_model_metrics", lambda data, *a: (seen.append(data), real_scene(data, *a))[1])
    monkeypatch.setattr(metrics, "cd_unit_sphere", lambda *a, **k: (grids.append(k.get("ref_grid")), real_cd(*a, **k))[1])
    texts = []
    for method in (None, "grid"):
        scene = tmp_path / (method or "absent") / "scene0"
        model = scene / "predictions" / "ours"
        (scene / "scans").mkdir(parents=True)
        model.mkdir(parents=True)
        write_ply_ascii(str(scene / "scans" / "iphone.ply"), iphone)
        write_ply_ascii(str(scene / "scans" / "mesh_aligned_0.05.ply"), verts, faces.tolist())
        np.savetxt(str(model / "steps5.xyz"), good)
        np.savetxt(str(model / "steps10.xyz"), more)
        args = {"dataset": "snpp", "normalize": normalize, "suffix": ""}
        if method:
            args["cd_method"] = method
        seen.clear(), grids.clear()
        er.handle_scene(str(scene), args)
        name = "metrics.csv" + ("_normalized.csv" if normalize else "")
        texts.append(open(str(model / name), "rb").read())
        assert len(seen) == 1 and len(grids) == 2
        if method:  # one grid of the ground truth for the scene, handed to both predictions
            index = seen[0]["cloud_index"]
            assert isinstance(index, PointGrid) and index.ref.shape == (len(verts), 3)
            assert grids[0] is index and grids[1] is index
        else:
            assert seen[0]["cloud_index"] is None and grids == [None, None]
    assert texts[0] == texts[1] and texts[0].count(b"\n") == 3


# ---- 10. memory discipline ---------------------------------------------------------------------------------------
def test_entry_point_inside_a_poisoned_arena(shell):
    """p2pb_nn_grid on case 4: nothing is written outside the outputs, the unresolved rows keep the poison after the ring
    search alone, every row is written after the walk"""
    n, nq = shell["ref"].shape[0], shell["query"].shape[0]
    grid = PointGrid(shell["ref"], 1)
    pts, skeys, rows, cell = grid.level(0)
    order = knn_grid.cell_grid.query_order(shell["query"], cell)
    want_d, want_i = shell["brute"]
    call, ptr = _lib.call, _lib.ptr
    with PoisonArena("cuda:0", 64 << 20) as arena:
        query, ref, pts, skeys, rows, order = (arena.put(t) for t in (shell["query"], shell["ref"], pts, skeys, rows, order))
        dist2, idx = torch.empty(nq, dtype=F32, device="cuda:0"), torch.empty(nq, dtype=I32, device="cuda:0")
        unresolved = torch.empty(nq, dtype=U8, device="cuda:0")
        assert arena.n_allocations >= 9  # (the outputs came out of the arena too)
        call("p2pb_nn_grid", nq, n, 3, ptr(order), ptr(query), ptr(pts), ptr(skeys), ptr(rows), cell, ptr(dist2), ptr(idx),
             ptr(unresolved), _lib.stream_ptr())
        arena.check_guards()
        assert set(unresolved.tolist()) <= {0, 1}
        open_ = unresolved.bool()
        assert 30 <= int(open_.sum()) < nq and bool(open_[-30:].all())  # (the isolated points come last)
        assert bool((idx[open_] == -1).all()) and bool(torch.isnan(dist2[open_]).all())  # the poison, untouched
        assert torch.equal(idx[~open_].long(), want_i[~open_])
        assert torch.equal(dist2[~open_].view(I32), want_d[~open_].view(I32))
        left = arena.put(torch.nonzero(open_).flatten().to(I32))
        call("p2pb_knn_grid_brute", left.numel(), n, 1, ptr(left), ptr(query), ptr(ref), ptr(dist2), ptr(idx),
             _lib.stream_ptr())
        arena.check_guards()
        arena.assert_written(dist2, "dist2")
        assert torch.equal(idx.long(), want_i) and torch.equal(dist2.view(I32), want_d.view(I32))
