"""The packed point <-> mesh operators with gradients (p2p_bridge_amd/p2m.py, csrc/p2m_packed.hip) on the GPU: forwards bit-equal to
the one-pair kernels of csrc/p2m.hip, gradients of the four kinds against fp64 autograd of tests/p2m_ref.py with fp32 torch
autograd of the same restatement as the yardstick (err_hip <= 4 err_fp32 + 1e-7: the 4 is for another association of the same
fp32 formulas and the scatter's summation order), exact edge cases, deterministic mode, the batched losses, memory discipline
and refusals. Inputs: tests/p2m_ref.py (held to the near-boundary cap by tests/test_p2m_packed.py)."""
import pytest
import torch

import p2m_ref as R
from oracle.poison_arena import PoisonArena

pytestmark = pytest.mark.gpu

CASES = [(name, kind, area) for name in R.SHAPES for kind in R.KINDS for area in R.AREAS if "face" in kind or area == R.AREAS[0]]
IDS = lambda c: f"{c[0]}-{c[1]}-{c[2]}"  # noqa: E731
MARGIN, FLOOR = 4.0, 1e-7


@pytest.fixture(scope="module")
def P():
    from p2p_bridge_amd import p2m

    return p2m


def apply(P, kind, points, pfirst, prims, tfirst, area):
    """the operator as the reference calls it: max_* = the largest example's query count"""
    total = (points if kind.startswith("point") else prims).shape[0]
    first = (pfirst if kind.startswith("point") else tfirst).tolist() + [total]
    maxq = max(b - a for a, b in zip(first[:-1], first[1:]))
    args = (points, pfirst, prims, tfirst, maxq) + ((area,) if "face" in kind else ())
    return getattr(P, kind + "_distance")(*args)


def run(P, b, kind, area, det=False, seed=5):
    """forward + backward on the GPU -> dict(dist, idx, gp, gs) on the host"""
    import p2p_bridge_amd

    pts = b["points"].cuda().requires_grad_()
    prims = R.kind_prims(b, kind).cuda().requires_grad_()
    d = apply(P, kind, pts, b["pfirst"].cuda(), prims, b["tfirst"].cuda(), area)
    idx = d.grad_fn.saved_tensors[2]
    assert idx.dtype == torch.int64 and d.dtype == torch.float32 and d.shape == idx.shape
    g = R.grad_dist(d.shape[0], seed).cuda()
    if det:
        with p2p_bridge_amd.deterministic():
            gp, gs = torch.autograd.grad(d, (pts, prims), g)
    else:
        gp, gs = torch.autograd.grad(d, (pts, prims), g)
    assert gp.shape == pts.shape and gs.shape == prims.shape
    return dict(dist=d.detach().cpu(), idx=idx.cpu(), gp=gp.cpu(), gs=gs.cpu(), g=g.cpu())


@pytest.fixture(scope="module")
def hip(P):
    """case -> (default run, deterministic run, second deterministic run), computed once"""
    out = {}
    for c in CASES:
        b = R.batch(c[0])
        out[c] = (run(P, b, c[1], c[2]), run(P, b, c[1], c[2], det=True), run(P, b, c[1], c[2], det=True))
    return out


@pytest.fixture(scope="module")
def ref():
    """case, idx -> the fp64 reference and the fp32 yardstick on the kernel's own idx (computed once per case)"""
    cache = {}

    def get(case, idx, g):
        if case not in cache:
            cache[case] = reference(R.batch(case[0]), case[1], case[2], idx, g)
        return cache[case]

    return get


def reference(b, kind, area, idx, g):
    """query rows and target rows of both gradients in fp64 and in fp32 (the fp64 run's selections), the per-pair flag, the
    rows that may be compared"""
    qp = kind.startswith("point")
    p, prim = R.gather_pairs(b, kind, idx)
    gp64, gs64, _, sel, flag = R.pair_grads(p, prim, g, area, torch.float64)
    gp32, gs32, _, _, _ = R.pair_grads(p, prim, g, area, torch.float32, sel)
    nt = R.kind_prims(b, kind).shape[0] if qp else b["points"].shape[0]
    out = {"flag": flag, "keep_q": ~flag, "chosen": R.scatter_rows(torch.ones(idx.shape[0]), idx, nt) > 0,
           "keep_t": R.scatter_rows(flag.float(), idx, nt) == 0}
    for tag, (gp, gs) in (("64", (gp64, gs64)), ("32", (gp32, gs32))):
        q_rows, t_rows = (gp, gs) if qp else (gs, gp)
        out["q" + tag], out["t" + tag] = q_rows, R.scatter_rows(t_rows, idx, nt)
    return out


def check_grads(label, got, r, kind):
    """the bound of the gradient tests on one run (got: dict of run()) against reference r"""
    qp = kind.startswith("point")
    got_q, got_t = (got["gp"], got["gs"]) if qp else (got["gs"], got["gp"])
    assert bool(torch.isfinite(got_q).all()) and bool(torch.isfinite(got_t).all()), label
    for what, g_hip, g64, g32, keep in (("query rows", got_q, r["q64"], r["q32"], r["keep_q"]),
                                        ("target rows", got_t, r["t64"], r["t32"], r["keep_t"])):
        e_hip, e_32 = R.rel_err(g_hip, g64, keep), R.rel_err(g32, g64, keep)
        print(f"{label} {what}: err_hip {e_hip:.3e}  err_fp32ref {e_32:.3e}  rows compared {int(keep.sum())} of {keep.numel()}")
        assert int(keep.sum()) > 0
        assert e_hip <= MARGIN * e_32 + FLOOR, (label, what, e_hip, e_32)
    # a target nobody chose: an exact zero row
    assert bool((got_t[~r["chosen"]] == 0).all()), label


# ---- 1, 2: forwards -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_packed_forward_equals_a_loop_of_single_pair_calls(P, hip, case):
    """faces: metrics.point_face_distance / face_point_distance per example, bit for bit, idx offset by the example's first
    index. edges (a, b): the same face kernels on the triangles (a, b, b) with min_triangle_area = 3e38."""
    from p2p_bridge_amd import metrics

    name, kind, area = case
    b = R.batch(name)
    got = hip[case][0]
    tris = R.as_triangles(R.kind_prims(b, kind))
    single = metrics.point_face_distance if kind.startswith("point") else metrics.face_point_distance
    for ps, ts in R.examples(b):
        d, i = single(b["points"][ps].cuda(), tris[ts].cuda(), area if "face" in kind else 3e38)
        qs, first = (ps, ts.start) if kind.startswith("point") else (ts, ps.start)
        assert torch.equal(got["dist"][qs], d.cpu()), (case, qs)
        assert torch.equal(got["idx"][qs], i.cpu() + first), (case, qs)
    d_ref, i_ref = R.oracle_chosen(b, kind, area)  # (and so the oracle's, which the host tests build on)
    assert torch.equal(got["dist"], d_ref) and torch.equal(got["idx"], i_ref)


# ---- 3, 5: gradients, both modes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gradients_against_fp64_autograd(hip, ref, case):
    got = hip[case][0]
    check_grads(f"{IDS(case)} default", got, ref(case, got["idx"], got["g"]), case[1])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_deterministic_mode_repeats_its_bits_and_meets_the_bound(hip, ref, case):
    default, det1, det2 = hip[case]
    for k in ("gp", "gs"):
        assert torch.equal(det1[k], det2[k]), (case, k)
    assert torch.equal(det1["idx"], default["idx"])
    check_grads(f"{IDS(case)} deterministic", det1, ref(case, default["idx"], default["g"]), case[1])


# ---- 4: edge cases, exact expectations ----------------------------------------------------------------------------------------
def single(P, kind, points, prims, area=0.0, det=False, g=None):
    """one example, every query's upstream gradient 1 (or g) -> (dist, idx, grad_points, grad_prims) on the host"""
    import p2p_bridge_amd

    pts, pr = points.cuda().requires_grad_(), prims.cuda().requires_grad_()
    zero = torch.zeros(1, dtype=torch.int64, device="cuda")
    d = apply(P, kind, pts, zero, pr, zero, area)
    idx = d.grad_fn.saved_tensors[2].cpu()
    g = torch.ones_like(d) if g is None else g.cuda()
    with p2p_bridge_amd.deterministic(det):
        gp, gs = torch.autograd.grad(d, (pts, pr), g)
    return d.detach().cpu(), idx, gp.cpu(), gs.cpu()


TRI = torch.tensor([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]])
SEG = torch.tensor([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]])


@pytest.mark.parametrize("det", (False, True))
def test_edge_cases_have_exact_gradients(P, det):
    # a point on a vertex: distance 0, every gradient exactly 0 (faces with and without the inside test, edges)
    for kind, prims, area in (("point_face", TRI, 0.0), ("face_point", TRI, 0.0), ("point_face", TRI, 3e38),
                              ("point_edge", SEG, 0.0), ("edge_point", SEG, 0.0)):
        for v in range(prims.shape[1]):
            d, _, gp, gs = single(P, kind, prims[0, v:v + 1].clone(), prims, area, det)
            assert float(d) == 0.0 and bool((gp == 0).all()) and bool((gs == 0).all()), (kind, area, v)
    # a collapsed triangle at min_triangle_area = 0: finite, zero
    flat = torch.full((1, 3, 3), 0.25)
    for kind in ("point_face", "face_point"):
        d, _, gp, gs = single(P, kind, torch.tensor([[0.5, 0.75, 1.0]]), flat, 0.0, det)
        assert bool(torch.isfinite(d).all()) and bool((gp == 0).all()) and bool((gs == 0).all()), kind
    # a zero-length segment: the point v1; gradient to p and v1 only
    p = torch.tensor([[0.5, 0.75, 1.0]])
    dot = torch.tensor([[[0.25, 0.25, 0.25], [0.25, 0.25, 0.25]]])
    for kind in ("point_edge", "edge_point"):
        d, _, gp, gs = single(P, kind, p, dot, 0.0, det)
        want = 2.0 * (p[0] - dot[0, 1])
        assert torch.equal(gp[0], want) and torch.equal(gs[0, 1], -want) and bool((gs[0, 0] == 0).all()), kind
        assert torch.equal(d, ((p[0] - dot[0, 1]) ** 2).sum().reshape(1))
    # a clamped t: the far end point gets a zero row (segments, and a triangle's nearest side)
    for kind, prims, area in (("point_edge", SEG, 0.0), ("edge_point", SEG, 0.0), ("point_face", TRI, 3e38)):
        for q, near, far in ((torch.tensor([[-1.0, -0.5, 0.0]]), 0, 1), (torch.tensor([[2.0, -0.5, 0.0]]), 1, 0)):
            _, _, gp, gs = single(P, kind, q, prims, area, det)
            want = 2.0 * (q[0] - prims[0, near])
            assert torch.equal(gp[0], want) and torch.equal(gs[0, near], -want), (kind, near)
            assert bool((gs[0, far] == 0).all()) and bool((gs[0, 2:] == 0).all()), (kind, far)


@pytest.mark.parametrize("det", (False, True))
def test_600_points_on_one_triangle_sum_into_one_row(P, det):
    """every contribution lands in one target row: its sum against fp64 under the bound of the gradient tests. No pair of this
    seeded input is near a boundary (asserted), so the whole row is compared."""
    g = torch.Generator().manual_seed(31)
    pts = R.cube_points(600, g)
    tri = torch.tensor([[[0.1, 0.2, 0.4], [0.9, 0.3, 0.5], [0.4, 0.8, 0.6]]])
    up = R.grad_dist(600, 7)
    d, idx, gp, gs = single(P, "point_face", pts, tri, 5e-3, det, up)
    assert bool((idx == 0).all())
    gp64, gs64, d64, sel, flag = R.pair_grads(pts, tri.repeat(600, 1, 1), up, 5e-3, torch.float64)
    gp32, gs32, _, _, _ = R.pair_grads(pts, tri.repeat(600, 1, 1), up, 5e-3, torch.float32, sel)
    assert int(flag.sum()) == 0 and 0 < int(sel["inside"].sum()) < 600
    row64, row32 = gs64.sum(0, keepdim=True), R.scatter_rows(gs32, idx, 1)
    for what, a, r64, r32 in (("grad_points", gp, gp64, gp32), ("grad_tris row", gs, row64, row32)):
        e_hip, e_32 = R.rel_err(a, r64), R.rel_err(r32, r64)
        print(f"600 on one triangle, det={det}, {what}: err_hip {e_hip:.3e}  err_fp32ref {e_32:.3e}")
        assert e_hip <= MARGIN * e_32 + FLOOR, (what, e_hip, e_32)
    assert R.rel_err(d, d64) <= 1e-6


# ---- 6: the batched losses ----------------------------------------------------------------------------------------------------
def mesh_lists(b, dtype=torch.float32, device="cpu", grad=False):
    """the batch as lists: every triangle its own three vertices -> (verts list, faces list, points list)"""
    verts, faces, points = [], [], []
    for ps, ts in R.examples(b):
        t = b["tris"][ts]
        verts.append(t.reshape(-1, 3).to(device=device, dtype=dtype).requires_grad_(grad))
        faces.append(torch.arange(3 * t.shape[0], device=device).reshape(-1, 3))
        points.append(b["points"][ps].to(device=device, dtype=dtype).requires_grad_(grad))
    return verts, faces, points


def loss_reference(P, b, which, idx, dtype, sels=None):
    """the loss of metrics/p2m.py from the restatement on the kernels' chosen pairs idx = (point -> prim, prim -> point), in
    dtype on the host -> (loss, verts grads, points grads, selections, flags)"""
    verts, faces, points = mesh_lists(b, dtype, grad=True)
    m, c = P.Meshes(verts, faces), P.Pointclouds(points)
    prims = m.verts_packed()[m.faces_packed() if which == "face" else m.edges_packed()]
    pk = c.points_packed()
    n = len(m)
    d_q, s_q, f_q = R.pair_d2(pk, prims[idx[0]], 5e-3, None if sels is None else sels[0])
    d_t, s_t, f_t = R.pair_d2(pk[idx[1]], prims, 5e-3, None if sels is None else sels[1])
    np_, ns = c.num_points_per_cloud(), (m.num_faces_per_mesh() if which == "face" else m.num_edges_per_mesh())
    to_mesh = m.faces_packed_to_mesh_idx() if which == "face" else m.edges_packed_to_mesh_idx()
    loss = ((d_q / np_[c.packed_to_cloud_idx()].to(dtype)).sum() + (d_t / ns[to_mesh].to(dtype)).sum()) / n
    grads = torch.autograd.grad(loss, verts + points)
    return loss.detach(), torch.cat(grads[:n]), torch.cat(grads[n:]), (s_q, s_t), (f_q, f_t)


@pytest.mark.parametrize("which", ("face", "edge"))
def test_batched_losses_and_their_gradients(P, which):
    b = R.batch("three")
    verts, faces, points = mesh_lists(b, device="cuda", grad=True)
    m, c = P.Meshes(verts, faces), P.Pointclouds(points)
    if which == "face":
        pd, fd = P.point_mesh_face_distance_custom(m, c)
        loss = pd + fd
    else:
        loss = P.point_mesh_edge_distance(m, c)
    loss.backward()
    # the chosen pairs, from the operators themselves
    prims = (m.verts_packed()[m.faces_packed() if which == "face" else m.edges_packed()]).detach()
    pf, sf = c.cloud_to_packed_first_idx(), (m.mesh_to_faces_packed_first_idx() if which == "face"
                                              else m.mesh_to_edges_packed_first_idx())
    idx = []
    for kind in (f"point_{which}", f"{which}_point"):
        d = apply(P, kind, c.points_packed().detach().requires_grad_(), pf, prims, sf, 5e-3)
        idx.append(d.grad_fn.saved_tensors[2].cpu())
    l64, gv64, gp64, sels, flags = loss_reference(P, b, which, idx, torch.float64)
    l32, gv32, gp32, _, _ = loss_reference(P, b, which, idx, torch.float32, sels)
    assert int(flags[0].sum()) + int(flags[1].sum()) == 0  # a condition on the seeded input: every row is compared
    gv, gp = torch.cat([v.grad for v in verts]).cpu(), torch.cat([p.grad for p in points]).cpu()
    for what, a, r64, r32 in (("loss", loss.detach().cpu().reshape(1), l64.reshape(1), l32.reshape(1)),
                              ("verts.grad", gv, gv64, gv32), ("points.grad", gp, gp64, gp32)):
        e_hip, e_32 = R.rel_err(a, r64), R.rel_err(r32, r64)
        print(f"point_mesh_{which}: {what}: err_hip {e_hip:.3e}  err_fp32ref {e_32:.3e}")
        assert e_hip <= MARGIN * e_32 + FLOOR, (what, e_hip, e_32)


def test_face_loss_of_one_pair_equals_the_metric(P):
    """N = 1: sum of 1 / count weights against the metric's mean is the only difference"""
    from p2p_bridge_amd import metrics

    b = R.batch("one")
    verts, faces, points = mesh_lists(b, device="cuda")
    for area in R.AREAS:
        pd, fd = P.point_mesh_face_distance_custom(P.Meshes(verts, faces), P.Pointclouds(points), area)
        pd0, fd0 = metrics.point_mesh_face_distance(points[0], verts[0], faces[0], area)
        torch.testing.assert_close(pd, pd0, rtol=1e-6, atol=0)
        torch.testing.assert_close(fd, fd0, rtol=1e-6, atol=0)


# ---- 7: memory discipline -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.SHAPES))
def test_operators_stay_inside_their_buffers(P, name):
    import p2p_bridge_amd

    b = R.batch(name)
    with PoisonArena("cuda:0", 64 << 20) as arena:
        pfirst, tfirst = arena.put(b["pfirst"]), arena.put(b["tfirst"])
        for kind in R.KINDS:
            for det in (False, True):
                pts, prims = arena.put(b["points"]).requires_grad_(), arena.put(R.kind_prims(b, kind)).requires_grad_()
                d = apply(P, kind, pts, pfirst, prims, tfirst, 5e-3)
                idx = d.grad_fn.saved_tensors[2]
                g = arena.put(R.grad_dist(d.shape[0]))
                with p2p_bridge_amd.deterministic(det):
                    gp, gs = torch.autograd.grad(d, (pts, prims), g)
                arena.check_guards()
                for t, what in ((d, "dist"), (gp, "grad_points"), (gs, "grad_prims")):
                    arena.assert_written(t, f"{kind} det={det} {what}")
                assert int(idx.min()) >= 0 and int(idx.max()) < (prims if kind.startswith("point") else pts).shape[0]
        assert arena.n_allocations >= 1 + 8 * 4  # dist, idx and both gradients of every call came out of the arena


# ---- 8: refusals --------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_before_any_launch(P):
    b = R.batch("three")
    pts, tris, pf, tf = b["points"].cuda(), b["tris"].cuda(), b["pfirst"].cuda(), b["tfirst"].cuda()
    ok = P.point_face_distance(pts, pf, tris, tf, 600)
    assert ok.shape == (858,)
    with pytest.raises(RuntimeError):
        P.point_face_distance(b["points"], pf, tris, tf, 600)  # a CPU tensor
    with pytest.raises(RuntimeError):
        P.point_face_distance(pts.double(), pf, tris, tf, 600)  # a wrong dtype
    with pytest.raises(RuntimeError):
        P.point_face_distance(pts, pf.int(), tris, tf, 600)
    with pytest.raises(RuntimeError):
        P.point_face_distance(pts.t().contiguous().t(), pf, tris, tf, 600)  # not contiguous
    with pytest.raises(ValueError):
        P.point_edge_distance(pts, pf, tris, tf, 600)  # triangles where segments belong
    with pytest.raises(ValueError):
        P.point_face_distance(pts, torch.tensor([0, 1, 1], device="cuda"), tris, tf, 857)  # an empty example
    with pytest.raises(ValueError):
        P.face_point_distance(pts, pf, tris, torch.tensor([0, 513, 769], device="cuda"), 513)  # first index at the end
    with pytest.raises(ValueError):
        P.point_face_distance(pts, pf, tris, tf[:2].contiguous(), 600)  # two batch sizes
    with pytest.raises(ValueError):
        P.point_face_distance(pts, pf, tris, tf, 599)  # max_points below the largest example
    with pytest.raises(ValueError):
        P.point_mesh_edge_distance(P.Meshes([tris[0]], [torch.tensor([[0, 1, 2]], device="cuda")]),
                                   P.Pointclouds([pts[:4], pts[4:8]]))
