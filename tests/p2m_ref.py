"""A torch restatement of the two pair functions of csrc/p2m_geom.h for the tests (a plain helper module, not a conftest):
point-segment and point-triangle squared distance over M pairs at once, in the dtype of its inputs, with the BRANCH SELECTIONS
either made here or passed in from outside, so that the fp64 evaluation (the reference), an fp32 evaluation (the yardstick for
fp32 rounding) and the kernels all sit on the same branch. Autograd through it gives the gradients. Every pair also gets a
near-boundary flag: there the branch is a matter of rounding and the gradients of the two sides differ by O(1), so a
comparison would measure the tie-break and not the arithmetic.

Also the seeded inputs of tests/test_p2m_packed.py (no GPU) and tests/test_p2m_packed_gpu.py.
"""
import torch

EPS = 1e-8  # P2M_EPS
FLAG_W = 1e-4  # a barycentric weight or a segment parameter this close to 0 or 1
FLAG_SIDE = 1e-6  # best and second-best side distance this close, relative
FLAG_AREA = 1e-4  # the triangle's area this close to min_triangle_area, relative
MAX_FLAGGED = 0.02  # the share of (query, chosen target) pairs the reference may flag on a seeded input


def _dot(a, b):
    return (a * b).sum(-1)


def _near01(x):
    return (x.abs() < FLAG_W) | ((x - 1).abs() < FLAG_W)


def segment_d2(p, v0, v1, sel=None):
    """p, v0, v1 [M,3] -> (d2 [M], sel, flag). sel = dict(collapsed bool[M], clamp i64[M]: 0 t <= 0, 1 t >= 1, 2 interior)"""
    d = v1 - v0
    l2 = _dot(d, d)
    own = sel is None
    collapsed = (l2 <= EPS) if own else sel["collapsed"]
    l2s = torch.where(collapsed, torch.ones_like(l2), l2)  # (no 0/0 on the branch not taken)
    t_raw = _dot(d, p - v0) / l2s
    if own:
        clamp = torch.full_like(l2, 2, dtype=torch.int64)
        clamp[t_raw.detach() >= 1] = 1
        clamp[~(t_raw.detach() > 0)] = 0
        sel = dict(collapsed=collapsed, clamp=clamp)
    clamp = sel["clamp"]
    t = torch.where(clamp == 2, t_raw, (clamp == 1).to(p.dtype))  # a clamped t is the constant 0 or 1
    q = torch.where(collapsed[:, None], p - v1, p - (v0 + t[:, None] * d))
    flag = (~collapsed & _near01(t_raw.detach())) | ((l2.detach() > EPS / 2) & (l2.detach() < EPS * 2))
    return _dot(q, q), sel, flag


def triangle_d2(p, v0, v1, v2, min_area, sel=None):
    """-> (d2 [M], sel, flag). sel = dict(inside bool[M], side i64[M]: 0 v0v1, 1 v0v2, 2 v1v2 (first minimum), seg = the
    selections of segment_d2 on that side)"""
    c = torch.linalg.cross(v2 - v0, v1 - v0)
    cc = _dot(c, c)
    nn = torch.where(cc > 0, torch.where(cc > 0, cc, torch.ones_like(cc)).sqrt(), torch.zeros_like(cc))
    n = c / (nn + EPS)[:, None]
    t = _dot(v0 - p, n)
    p0 = p + t[:, None] * n
    e0, e1, e2 = v1 - v0, v2 - v0, p0 - v0
    d00, d01, d11, d20, d21 = _dot(e0, e0), _dot(e0, e1), _dot(e1, e1), _dot(e2, e0), _dot(e2, e1)
    denom = d00 * d11 - d01 * d01 + EPS
    w1, w2 = (d11 * d20 - d01 * d21) / denom, (d00 * d21 - d01 * d20) / denom
    w = torch.stack([1 - w1 - w2, w1, w2], 1).detach()
    area_ok = (0.5 * nn.detach() >= min_area)
    own = sel is None
    sides = ((v0, v1), (v0, v2), (v1, v2))
    per_side = [segment_d2(p, a, b) for a, b in sides]
    ds = torch.stack([s[0] for s in per_side], 1).detach()
    # the feature of the triangle a side's foot lies on: vertex 0, 1 or 2 for a clamped (or collapsed) side, else the side itself
    ends = ((0, 1), (0, 2), (1, 2))
    feat = torch.stack([torch.where(s[1]["collapsed"] | (s[1]["clamp"] == 1), e[1],
                                    torch.where(s[1]["clamp"] == 0, e[0], 3 + k))
                        for k, (s, e) in enumerate(zip(per_side, ends))], 1)
    if own:
        inside = area_ok & ((w >= 0) & (w <= 1)).all(1)
        side = torch.zeros_like(inside, dtype=torch.int64)
        best = ds[:, 0].clone()
        for k in (1, 2):
            better = ds[:, k] < best
            side[better], best[better] = k, ds[better, k]
    else:
        inside, side = sel["inside"], sel["side"]
    a = torch.where((side == 2)[:, None], v1, v0)
    b = torch.where((side == 0)[:, None], v1, v2)
    d_out, seg, seg_flag = segment_d2(p, a, b, None if own else sel["seg"])
    # best and second-best side: a near tie is a boundary UNLESS both feet are the same vertex of the triangle -- two sides that
    # meet in the nearest vertex give the same distance expression |p - v|^2 and the same gradient, whichever is selected (and
    # that tie is exact in every precision: the nearest feature of most outside points)
    srt, order = ds.sort(dim=1)
    f0, f1 = feat.gather(1, order[:, :1])[:, 0], feat.gather(1, order[:, 1:2])[:, 0]
    tie = ((srt[:, 1] - srt[:, 0]) < FLAG_SIDE * srt[:, 1]) & ~((f0 == f1) & (f0 < 3))
    flag = area_ok & _near01(w).any(1)
    flag |= ~inside & (seg_flag | tie)
    flag |= (0.5 * nn.detach() - min_area).abs() < FLAG_AREA * min_area
    return torch.where(inside, t * t, d_out), dict(inside=inside, side=side, seg=seg), flag


def pair_d2(p, prim, min_area, sel=None):
    """p [M,3], prim [M,3,3] (triangles) or [M,2,3] (segments) -> (d2, sel, flag)"""
    if prim.shape[1] == 3:
        return triangle_d2(p, prim[:, 0], prim[:, 1], prim[:, 2], min_area, sel)
    return segment_d2(p, prim[:, 0], prim[:, 1], sel)


def pair_grads(p, prim, g, min_area, dtype, sel=None):
    """d (sum_m g[m] d2[m]) / d (p, prim) in `dtype` by autograd: -> (grad_p [M,3], grad_prim [M,PV,3], d2, sel, flag), one row
    per PAIR (nothing is scattered here)"""
    p = p.detach().to(dtype).requires_grad_()
    prim = prim.detach().to(dtype).requires_grad_()
    d2, sel, flag = pair_d2(p, prim, min_area, sel)
    gp, gs = torch.autograd.grad((d2 * g.to(dtype)).sum(), (p, prim))
    return gp, gs, d2.detach(), sel, flag


def scatter_rows(rows, idx, n):
    """out[t] = sum of rows[m] with idx[m] == t, in ascending m, in the dtype of rows"""
    return torch.zeros((n,) + tuple(rows.shape[1:]), dtype=rows.dtype).index_add_(0, idx, rows)


def rel_err(got, ref, keep=None):
    """max-norm error over the max-norm of the reference, over the rows `keep` (bool) only; no row kept: 0"""
    got, ref = got.double(), ref.double()
    if keep is not None:
        got, ref = got[keep], ref[keep]
    if ref.numel() == 0:
        return 0.0
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


# ---- the seeded inputs --------------------------------------------------------------------------------------------------------
SHAPES = {  # name -> (points per example, faces per example): both straddle the 256-wide tile; three examples = grid axis y
    "three": ((1, 257, 600), (513, 1, 255)),
    "one": ((256,), (256,)),
}
SEEDS = {"three": 23, "one": 21}  # "one" has a flagged pair (the exemption is exercised), "three" has none (every row is compared)
AREAS = (5e-3, 0.0)


def cube_points(n, g):
    return torch.rand(n, 3, generator=g)


def cube_tris(n, g, side=0.2):
    """first vertex uniform in the unit cube, the other two within `side` per axis of it"""
    v0 = torch.rand(n, 1, 3, generator=g)
    return torch.cat([v0, v0 + (torch.rand(n, 2, 3, generator=g) * 2 - 1) * side], 1).contiguous()


def batch(name):
    """-> dict(points f32[P,3], tris f32[T,3,3], segms f32[T,2,3] (the triangles' first sides), pfirst, tfirst i64[N],
    pcount, tcount tuples): packed, seeded"""
    pc, tc = SHAPES[name]
    g = torch.Generator().manual_seed(SEEDS[name])
    points = torch.cat([cube_points(n, g) for n in pc], 0).contiguous()
    tris = torch.cat([cube_tris(n, g) for n in tc], 0).contiguous()
    first = lambda c: torch.tensor([sum(c[:i]) for i in range(len(c))], dtype=torch.int64)
    return dict(points=points, tris=tris, segms=tris[:, :2].contiguous(), pfirst=first(pc), tfirst=first(tc), pcount=pc,
                tcount=tc)


def examples(b):
    """[(point slice, primitive slice)] of the batch's examples"""
    out, p0, t0 = [], 0, 0
    for n, m in zip(b["pcount"], b["tcount"]):
        out.append((slice(p0, p0 + n), slice(t0, t0 + m)))
        p0, t0 = p0 + n, t0 + m
    return out


KINDS = ("point_face", "face_point", "point_edge", "edge_point")


def kind_prims(b, kind):
    return b["tris"] if "face" in kind else b["segms"]


def gather_pairs(b, kind, idx):
    """the (point, primitive) rows of the pairs (query q, target idx[q]) -> (p [Q,3], prim [Q,PV,3])"""
    prims = kind_prims(b, kind)
    if kind.startswith("point"):
        return b["points"], prims[idx]
    return b["points"][idx], prims


def as_triangles(prims):
    """segments (a, b) as the triangles (a, b, b): with min_triangle_area = 3e38 the face function is the first minimum of
    seg(a, b), seg(a, b), seg(b, b), and seg(b, b) is the distance to b, never below seg(a, b)"""
    return prims if prims.shape[1] == 3 else torch.cat([prims, prims[:, 1:]], 1).contiguous()


def oracle_chosen(b, kind, area):
    """(dist f32[Q], packed idx i64[Q]) of the four operators from oracle.cpu_ops.point_face_dist, one example at a time"""
    from oracle import cpu_ops

    which = 0 if kind.startswith("point") else 1
    tris = as_triangles(kind_prims(b, kind))
    ds, idxs = [], []
    for ps, ts in examples(b):
        d, i = cpu_ops.point_face_dist(b["points"][ps].contiguous(), tris[ts].contiguous(), area if "face" in kind else 3e38, which)
        ds.append(d)
        idxs.append(i + (ts.start if which == 0 else ps.start))
    return torch.cat(ds), torch.cat(idxs)


def grad_dist(nq, seed=5):
    """upstream gradient of the distances: positive, of order 1"""
    return (0.5 + torch.rand(nq, generator=torch.Generator().manual_seed(seed))).float()
