"""The grid-accelerated point <-> triangle-mesh search (csrc/p2m_grid.hip, metrics.TriangleGrid, method="grid") against
oracle.cpu_ops.point_face_dist: torch.equal on the distances AND the indices, both directions, wherever the pruning bound, the
tie rule, the broad / unbounded lists or the fallback could go wrong. Every mesh here has at most a few thousand triangles."""
import pytest
import torch

from oracle import cpu_ops
from oracle.poison_arena import PoisonArena

pytestmark = pytest.mark.gpu

AREAS = (5e-3, 0.0)


@pytest.fixture(scope="module")
def M():
    from p2p_bridge_amd import metrics

    return metrics


def shell(P, seed, radius=1.0, spread=0.05):
    g = torch.Generator().manual_seed(seed)
    return (torch.nn.functional.normalize(torch.randn(P, 3, generator=g), dim=1) * radius
            * (1 + spread * torch.randn(P, 1, generator=g))).contiguous()


def sphere_tris(T, size, seed, radius=1.0):
    """T small triangles scattered over a sphere: first vertex on it, the other two within `size` per axis"""
    g = torch.Generator().manual_seed(seed)
    v0 = torch.nn.functional.normalize(torch.randn(T, 1, 3, generator=g), dim=2) * radius
    off = (torch.rand(T, 2, 3, generator=g) * 2 - 1) * size
    return torch.cat([v0, v0 + off], dim=1).contiguous()


def lattice(n, edge, origin=(0.0, 0.0, 0.0)):
    """n x n squares of `edge` in the plane z = origin[2], two right triangles each -> f32[2 n^2, 3, 3]"""
    i, j = torch.meshgrid(torch.arange(n, dtype=torch.float32), torch.arange(n, dtype=torch.float32), indexing="ij")
    x, y = origin[0] + i.flatten() * edge, origin[1] + j.flatten() * edge
    z = torch.full_like(x, origin[2])
    a = torch.stack([torch.stack([x, y, z], 1), torch.stack([x + edge, y, z], 1), torch.stack([x, y + edge, z], 1)], 1)
    b = torch.stack([torch.stack([x + edge, y + edge, z], 1), torch.stack([x, y + edge, z], 1), torch.stack([x + edge, y, z], 1)], 1)
    return torch.cat([a, b], 0).contiguous()


def check(M, pts, tris, area, grid=None):
    """both directions bit-equal to the oracle -> {0: (dist, idx, stats), 1: ...}, the oracle's outputs under "ref\""""
    dp, dt = pts.cuda(), tris.cuda()
    grid = grid or M.TriangleGrid(dt, area)
    out = {"ref": {}}
    for which, fn in ((0, grid.point_face), (1, grid.face_point)):
        d_ref, i_ref = cpu_ops.point_face_dist(pts.contiguous(), tris.contiguous(), area, which)
        d, i, stats = fn(dp, return_stats=True)
        assert i.dtype == torch.int64 and d.dtype == torch.float32
        assert torch.equal(i.cpu(), i_ref), f"which={which}: {int((i.cpu() != i_ref).sum())} indices differ"
        assert torch.equal(d.cpu(), d_ref), f"which={which}: {int((d.cpu() != d_ref).sum())} distances differ"
        out[which], out["ref"][which] = (d, i, stats), (d_ref, i_ref)
    return out


@pytest.mark.parametrize("area", AREAS)
def test_icosphere_shell(M, area):
    from test_metrics_unit_sphere_gpu import icosphere

    verts, faces = icosphere(3)
    tris = verts[faces].contiguous()
    assert tris.shape[0] == 1280
    pts = shell(4000, 11)
    out = check(M, pts, tris, area)
    for which in (0, 1):  # the grid did the work: few queries fell through to the brute force, no triangle is broad
        stats = out[which][2]
        assert stats["fallback"] <= 0.1 * stats["queries"], stats
        assert stats["broad"] == 0 and stats["incidences"] > 0, stats
    # the public door gives the same tensors as the index's methods, and as the brute force
    for fn in (M.point_face_distance, M.face_point_distance):
        d, i = fn(pts.cuda(), tris.cuda(), area, method="grid")
        d0, i0 = fn(pts.cuda(), tris.cuda(), area)
        assert torch.equal(d, d0) and torch.equal(i, i0)


@pytest.mark.parametrize("u", [1.5, 2.5])
@pytest.mark.parametrize("area", AREAS)
def test_rings_two_and_three_resolve(M, area, u):
    """Points u cell edges off the unit icosphere, 256 outside and 256 inside, u = 1.5 and u = 2.5: ring 1 alone resolves no
    query in either direction (max_ring = 1 sends all of them to the fallback), the plan's rings resolve every one (no
    fallback): the answers come out of the walk's "only the end cells of an inner column are new" branch, bit for bit."""
    from test_metrics_unit_sphere_gpu import icosphere

    verts, faces = icosphere(3)
    tris = verts[faces].contiguous()
    grid = M.TriangleGrid(tris.cuda(), area)
    cell = grid.plan.cell
    print(f"area={area} u={u}: cell={cell} max_ring={grid.plan.max_ring}")
    g = torch.Generator().manual_seed(int(10 * u))
    dirs = torch.nn.functional.normalize(torch.randn(512, 3, generator=g), dim=1)
    radius = torch.cat([torch.full((256, 1), 1 + u * cell), torch.full((256, 1), 1 - u * cell)])
    pts = (dirs * radius).contiguous()
    out = check(M, pts, tris, area, grid)
    print("rings:", out[0][2], out[1][2])
    assert out[0][2]["fallback"] == 0 and out[1][2]["fallback"] == 0
    grid.plan = grid.plan._replace(max_ring=1)
    out = check(M, pts, tris, area, grid)
    print("ring 1 only:", out[0][2], out[1][2])
    assert out[0][2]["fallback"] == 512 and out[1][2]["fallback"] == 1280


def _box_dist2(pts, tris):
    lo, hi = tris.min(dim=1).values, tris.max(dim=1).values  # [T,3]
    gap = torch.clamp(torch.maximum(lo[None] - pts[:, None], pts[:, None] - hi[None]), min=0)
    return (gap.double() ** 2).sum(-1)  # [P,T]


@pytest.mark.parametrize("edge", [0.01, 0.003])
def test_enlarged_inside_region(M, edge):
    """min_triangle_area = 0: the +1e-8 of the barycentric denominator enlarges the region that measures the PLANE distance
    (k = 2 at edge 0.01, about 124 at 0.003), so the winner is often not the triangle whose vertex box is nearest"""
    n = 32
    tris = lattice(n, edge, origin=(0.1, 0.2, 0.3))
    assert tris.shape[0] == 2048
    g = torch.Generator().manual_seed(3)
    P, side = 3000, n * edge
    margin = torch.tensor([0.5 * edge, 2 * edge, 0.1, 0.5])[torch.randint(0, 4, (P,), generator=g)]
    xy = torch.rand(P, 2, generator=g) * (side + 2 * margin[:, None]) - margin[:, None] + torch.tensor([0.1, 0.2])
    z = 0.3 + torch.where(torch.arange(P) % 2 == 0, torch.zeros(P), (torch.rand(P, generator=g) - 0.5) * 0.2 * edge)
    pts = torch.cat([xy, z[:, None]], 1).contiguous()
    d_ref, i_ref = cpu_ops.point_face_dist(pts, tris, 0.0, 0)
    bd = _box_dist2(pts, tris)
    naive_wrong = bd.gather(1, i_ref[:, None])[:, 0] > bd.min(dim=1).values + 1e-12
    assert int(naive_wrong.sum()) >= 10, "the case does not exercise the enlarged region"
    check(M, pts, tris, 0.0)


def test_degenerate_triangles(M):
    tris = sphere_tris(300, 0.1, 5)
    tris[17, 1] = tris[17, 0]
    tris[17, 2] = tris[17, 0]  # all three vertices equal
    tris[5, 1] = tris[5, 0]    # two equal
    pts = shell(1000, 6)
    out = check(M, pts, tris, 0.0)
    d, i, stats = out[0]
    assert bool((d == 0).all()) and bool((i == 5).all())  # denom is the epsilon alone: weights 0/0/1, distance 0 everywhere
    assert stats["unbounded"] >= 2
    check(M, pts, tris, 5e-3)


@pytest.mark.parametrize("area", AREAS)
def test_ties_resolve_to_the_lowest_index(M, area):
    tris = lattice(8, 0.125)
    tris = torch.cat([tris, tris], 0).contiguous()  # every triangle listed twice
    i, j = torch.meshgrid(torch.arange(17, dtype=torch.float32), torch.arange(17, dtype=torch.float32), indexing="ij")
    above = torch.stack([i.flatten() * 0.0625, j.flatten() * 0.0625, torch.full((289,), 0.05)], 1)  # over vertices and edges
    pts = torch.cat([above, above], 0).contiguous()  # every point listed twice
    out = check(M, pts, tris, area)
    assert int(out[0][1].max()) < 128 and int(out[1][1].max()) < 289  # the first copy wins
    d_ref = out["ref"][0][0]
    assert bool(torch.isclose(d_ref, torch.tensor(0.0025), rtol=1e-5).all())  # (the ties are real: every point is 0.05 above)


@pytest.mark.parametrize("area", AREAS)
@pytest.mark.parametrize("P,T", [(257, 1), (1, 255), (63, 65), (65, 63), (255, 257), (257, 255)])
def test_sizes_around_the_tiles(M, P, T, area):
    check(M, shell(P, P + T), sphere_tris(T, 0.1, T), area)


def room(seed=0):
    c = torch.tensor([[x, y, z] for z in (-1.0, 1.0) for y in (-1.0, 1.0) for x in (-1.0, 1.0)])
    f = torch.tensor([[0, 1, 3], [0, 3, 2], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                      [1, 3, 7], [1, 7, 5]])
    tris = torch.cat([sphere_tris(1500, 0.03, seed, 0.5), c[f], sphere_tris(1500, 0.03, seed + 1, 0.5)], 0).contiguous()
    g = torch.Generator().manual_seed(seed + 2)
    wall = torch.rand(2000, 3, generator=g) * 2 - 1
    wall[torch.arange(2000), torch.randint(0, 3, (2000,), generator=g)] = 0.99
    pts = torch.cat([shell(3000, seed + 3, 0.5, 0.02), wall], 0).contiguous()
    return pts, tris


@pytest.mark.parametrize("area", AREAS)
def test_room_with_broad_walls(M, area):
    pts, tris = room()
    out = check(M, pts, tris, area)
    stats = out[0][2]
    assert stats["broad"] >= 12 and (area == 0.0 or stats["broad"] == 12), stats  # the 12 walls span the whole box
    assert stats["fallback"] <= 0.2 * stats["queries"], stats


@pytest.mark.parametrize("area", AREAS)
def test_ring_limit_sends_queries_to_the_fallback(M, area):
    tris = sphere_tris(500, 0.05, 21)
    g = torch.Generator().manual_seed(22)
    far = torch.rand(600, 3, generator=g) + torch.tensor([3.0, 0.0, 0.0])
    far[:300, 0] += 27.0  # beyond the coordinates the index answers for, and merely beyond the rings
    out = check(M, far.contiguous(), tris, area)
    assert out[0][2]["fallback"] == 600 and out[1][2]["fallback"] == 500
    # a mesh far larger than the cloud
    big = sphere_tris(3000, 0.02, 23, 5.0)
    small = ((torch.rand(200, 3, generator=g) - 0.5) * 0.02).contiguous()
    out = check(M, small, big, area)
    assert out[0][2]["fallback"] == 200 and out[1][2]["fallback"] > 2000
    # a cloud of identical points
    check(M, torch.tensor([[0.6, 0.0, 0.8]]).repeat(300, 1).contiguous(), sphere_tris(1000, 0.05, 24), area)


@pytest.mark.parametrize("area", AREAS)
def test_non_finite_and_out_of_range(M, area):
    tris = sphere_tris(500, 0.1, 31)
    pts = shell(500, 32)
    pts[7, 0] = float("nan")
    pts[9, 1] = 1e30
    pts[11, 2] = float("inf")
    tris[3, 2, 2] = float("nan")
    tris[4, 0, 0] = float("nan")
    tris[6, 1, 1] = float("inf")
    check(M, pts, tris, area)
    # a cloud of nothing but such points, and a mesh of nothing but such triangles: brute-force semantics throughout
    check(M, pts[[7, 9, 11]].contiguous(), tris, area)
    check(M, pts, tris[[3, 4, 6]].contiguous(), area)


@pytest.mark.parametrize("case", ["icosphere", "room"])
def test_inside_the_poisoned_arena(M, case):
    """workspaces (boxes, counts, incidence keys and ids, point keys) and results carved out of a poisoned arena: intact
    guards, no NaN from an over-read, parity as above"""
    if case == "icosphere":
        from test_metrics_unit_sphere_gpu import icosphere

        verts, faces = icosphere(3)
        pts, tris, area = shell(4000, 11), verts[faces].contiguous(), 0.0
    else:
        (pts, tris), area = room(), 5e-3
    with PoisonArena("cuda", 64 << 20) as arena:
        dp, dt = arena.put(pts), arena.put(tris)
        grid = M.TriangleGrid(dt, area)
        before = arena.n_allocations
        assert before >= 7  # box, shrink, class, counts, wide, keys, ids
        for which, fn in ((0, grid.point_face), (1, grid.face_point)):
            d, i = fn(dp)
            arena.check_guards()
            arena.assert_written(d, "squared distance")
            d_ref, i_ref = cpu_ops.point_face_dist(pts, tris, area, which)
            assert torch.equal(i.cpu(), i_ref) and torch.equal(d.cpu(), d_ref)
        assert arena.n_allocations >= before + 6


def test_evaluate_rooms_uses_one_index_per_scene(M, monkeypatch):
    import numpy as np

    from p2p_bridge_amd import evaluate_rooms as er
    from p2p_bridge_amd import p2m_grid
    from test_metrics_unit_sphere_gpu import icosphere

    verts, faces = icosphere(2)
    verts = verts * 2.0 + torch.tensor([1.0, -2.0, 0.5])
    mesh = {"points": verts.double().numpy(), "faces": faces.numpy()}
    preds = {f"steps{k}": (shell(700, 40 + k, 2.0, 0.03) + torch.tensor([1.0, -2.0, 0.5])).double().numpy() for k in (5, 10)}
    built = []
    real = p2m_grid.TriangleGrid.__init__
    monkeypatch.setattr(p2m_grid.TriangleGrid, "__init__", lambda self, *a, **k: (built.append(1), real(self, *a, **k))[1])
    for normalize in (True, False):
        base = {"dataset": "snpp", "normalize": normalize, "suffix": ""}
        data = {"faro": mesh["points"], "faro_mesh": mesh, "models": {"m": preds}}
        built.clear()
        got = er.calculate_model_metrics(data, "m", dict(base, p2m_method="grid"))
        assert len(built) == 1  # one mesh index for the scene's two predictions
        want = er.calculate_model_metrics(dict(data), "m", dict(base, p2m_method="brute"))
        assert len(built) == 1
        for cfg in preds:
            assert got[cfg] == want[cfg] and got[cfg]["point_dist"] > 0 and np.isfinite(got[cfg]["face_dist"])
            one = er.get_mectrics(dict(base, p2m_method="grid"), mesh["points"], preds[cfg], gt_mesh=mesh)
            assert one == want[cfg]
    with pytest.raises(ValueError):
        er.get_mectrics(dict(base, p2m_method="octree"), mesh["points"], preds["steps5"], gt_mesh=mesh)
