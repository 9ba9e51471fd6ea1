"""Host half of the packed point <-> mesh loss (p2p_bridge_amd/p2m.py, csrc/p2m_packed.hip): the fp64 reference of
tests/p2m_ref.py is tied to the oracle the forward kernels are pinned against, the seeded inputs of the GPU tests are held to the
cap on near-boundary pairs (a condition on the inputs: it keeps tests/test_p2m_packed_gpu.py from excusing itself), and the
Meshes / Pointclouds accessors are checked against hand-written expectations. No GPU."""
import pytest
import torch

import p2m_ref as R

CASES = [(name, kind, area) for name in R.SHAPES for kind in R.KINDS for area in R.AREAS if "face" in kind or area == R.AREAS[0]]


@pytest.fixture(scope="module")
def chosen():
    """(batch name, kind, area) -> the oracle's (dist, packed idx): the pairs the kernels choose, bit for bit"""
    return {c: R.oracle_chosen(R.batch(c[0]), c[1], c[2]) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_fp64_forward_agrees_with_the_oracle(chosen, case):
    """the restatement evaluated in fp64 on the oracle's chosen pairs gives the oracle's fp32 distances to 1e-6, as max-norm
    error over the max-norm of the distances -- the measure of the gradient tests. (Elementwise a small distance cannot agree
    that well: t^2 = ((v0 - p).n)^2 carries the fp32 rounding of a dot product of terms of size |v0 - p|, 2.6e-5 relative at
    the worst pair of these inputs.) And the chosen target is the nearest of the example in fp64 too, to the same margin."""
    name, kind, area = case
    b = R.batch(name)
    d32, idx = chosen[case]
    p, prim = R.gather_pairs(b, kind, idx)
    d64, _, _ = R.pair_d2(p.double(), prim.double(), area)
    err = R.rel_err(d32, d64)
    print(f"{case}: max-norm relative error of the oracle's distances against fp64 = {err:.3e}")
    assert err <= 1e-6
    # no other target of the example is nearer than the chosen one by more than that margin
    prims = R.kind_prims(b, kind)
    scale = float(d64.max())
    for ps, ts in R.examples(b):
        qs, tsl = (ps, ts) if kind.startswith("point") else (ts, ps)
        for q in range(qs.start, qs.stop, 37):
            if kind.startswith("point"):
                pp, tt = b["points"][q:q + 1].expand(tsl.stop - tsl.start, 3), prims[tsl]
            else:
                pp, tt = b["points"][tsl], prims[q:q + 1].expand(tsl.stop - tsl.start, *prims.shape[1:])
            allq, _, _ = R.pair_d2(pp.double(), tt.double(), area)
            assert float(allq.min()) >= float(d64[q]) - 1e-6 * scale


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_near_boundary_pairs_stay_under_the_cap(chosen, case):
    name, kind, area = case
    b = R.batch(name)
    p, prim = R.gather_pairs(b, kind, chosen[case][1])
    _, _, flag = R.pair_d2(p.double(), prim.double(), area)
    share = float(flag.float().mean())
    print(f"{case}: {int(flag.sum())} of {flag.numel()} chosen pairs flagged ({share:.4f})")
    assert share <= R.MAX_FLAGGED


def test_flags_fire_on_constructed_boundaries():
    """the flag is not vacuous: a foot on a triangle's side, a foot at a segment's end, equidistant sides, a segment of length^2
    near eps and a triangle of area near min_triangle_area are flagged; a plain interior pair is not"""
    tri = torch.tensor([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]], dtype=torch.float64)
    f = lambda p, t=tri, a=0.0: bool(R.pair_d2(torch.tensor([p], dtype=torch.float64), t, a)[2])
    assert not f([0.25, 0.25, 0.3])
    assert f([0.5, 0.00001, 0.3])  # barycentric weight within 1e-4 of 0
    assert f([0.5, -0.2, 0.0]) is False and f([1.00001, -0.2, 0.0])  # parameter of the nearest side within 1e-4 of 1
    assert f([-0.3, -0.3, 0.0]) is False  # both nearest sides end in vertex 0: the same expression, not a boundary
    iso = torch.tensor([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 1.0, 0.0]]], dtype=torch.float64)
    assert f([0.5, 0.9, 0.0], iso, 1e9)  # area test fails -> sides; v0v2 and v1v2 equidistant, both feet interior
    assert f([0.5, 0.3, 0.2], tri, 0.5 * (1 + 5e-5))  # area 0.5 within 1e-4 relative of min_triangle_area
    seg = torch.tensor([[[0.0, 0.0, 0.0], [1.2e-4, 0.0, 0.0]]], dtype=torch.float64)  # l2 = 1.44e-8, within 2x of eps
    assert f([0.3, 0.3, 0.0], seg)
    assert not f([0.5, 0.3, 0.0], tri[:, :2].contiguous())


def two_meshes():
    """a square of two faces that list their shared edge 1-2 in both directions, and a single face that starts at its last vertex"""
    va = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 0.0]])
    fa = torch.tensor([[0, 1, 2], [2, 1, 3]])
    vb = torch.tensor([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0]])
    fb = torch.tensor([[2, 0, 1]])
    return [va, vb], [fa, fb]


def test_meshes_accessors_on_a_two_mesh_batch():
    from p2p_bridge_amd.p2m import Meshes

    verts, faces = two_meshes()
    m = Meshes(verts, faces)
    eq = lambda t, want: t.dtype == torch.int64 and t.tolist() == want
    assert len(m) == 2
    assert torch.equal(m.verts_packed(), torch.cat(verts))
    assert eq(m.faces_packed(), [[0, 1, 2], [2, 1, 3], [6, 4, 5]])
    assert eq(m.edges_packed(), [[0, 1], [0, 2], [1, 2], [1, 3], [2, 3], [4, 5], [4, 6], [5, 6]])
    assert eq(m.mesh_to_faces_packed_first_idx(), [0, 2]) and eq(m.mesh_to_edges_packed_first_idx(), [0, 5])
    assert eq(m.num_faces_per_mesh(), [2, 1]) and eq(m.num_edges_per_mesh(), [5, 3])
    assert eq(m.faces_packed_to_mesh_idx(), [0, 0, 1]) and eq(m.edges_packed_to_mesh_idx(), [0, 0, 0, 0, 0, 1, 1, 1])
    # the packed vertices are a cat of the list: a gradient on them reaches the list's tensors
    v = [x.clone().requires_grad_() for x in verts]
    Meshes(v, faces).verts_packed()[Meshes(v, faces).edges_packed()].sum().backward()
    assert v[0].grad.tolist() == [[2.0] * 3, [3.0] * 3, [3.0] * 3, [2.0] * 3] and v[1].grad.tolist() == [[2.0] * 3] * 3


def test_pointclouds_accessors():
    from p2p_bridge_amd.p2m import Pointclouds

    pts = [torch.zeros(2, 3), torch.ones(3, 3)]
    c = Pointclouds(pts)
    eq = lambda t, want: t.dtype == torch.int64 and t.tolist() == want
    assert len(c) == 2 and torch.equal(c.points_packed(), torch.cat(pts))
    assert eq(c.cloud_to_packed_first_idx(), [0, 2]) and eq(c.num_points_per_cloud(), [2, 3])
    assert eq(c.packed_to_cloud_idx(), [0, 0, 1, 1, 1])


def test_empty_examples_raise_value_error():
    from p2p_bridge_amd.p2m import Meshes, Pointclouds

    verts, faces = two_meshes()
    with pytest.raises(ValueError):
        Pointclouds([torch.zeros(2, 3), torch.zeros(0, 3)])
    with pytest.raises(ValueError):
        Meshes(verts, [faces[0], torch.zeros(0, 3, dtype=torch.int64)])
    with pytest.raises(ValueError):
        Meshes([verts[0], torch.zeros(0, 3)], faces)
    with pytest.raises(ValueError):
        Meshes(verts, [faces[0], torch.tensor([[0, 1, 3]])])  # a vertex the mesh does not have


def test_operators_refuse_cpu_tensors():
    """no CPU path: the wrapper's checks raise before any call into the library"""
    from p2p_bridge_amd import p2m

    b = R.batch("one")
    for fn, prims in ((p2m.point_face_distance, b["tris"]), (p2m.face_point_distance, b["tris"]),
                      (p2m.point_edge_distance, b["segms"]), (p2m.edge_point_distance, b["segms"])):
        with pytest.raises(RuntimeError):
            fn(b["points"], b["pfirst"], prims, b["tfirst"], 256)
