"""The operator families below inside a poisoned arena (oracle/poison_arena.py): WHERE the kernels read and write.

Each case builds its inputs on the host, `put`s them into the arena (poison on both sides of every input), calls the
existing Python wrapper while the wrapper's torch.empty / torch.zeros / ... are carved out of the arena, and then asserts
  1. the guards around every output and workspace are intact (no write past a buffer or a sizing function's promise),
  2. every returned floating-point tensor is free of NaN (no element left unwritten, no input over-read that counts),
  3. the wrapper allocated through the patch (at least one carve per call),
  4. parity with the reference the suite already uses for that operator, at the tolerance stated in the file named
     next to each family (nothing here widens one) -- NaN propagates, so this is what turns an over-read into a failure.
`test_planted_overrun_is_caught` proves the net is live on the device. Workspaces are exempt from 2, not from 1; so are the two
results that the ABI header documents as written in part (`listed_only`, `active_only`: the cases cite the header).
Wrappers of fused.py that no case calls here are held in tests/test_fused_discipline_gpu.py, same arena, same four checks, host
references only: interp_add, pw_conv_pool_gather, voxel_sort / voxelize_cl_gather, conv3d_presplit and the `pre=True`
convolutions, conv3d_far_field_gn, pvconv_tail, minmax_act_pool_gn, affine_act, and the arms this file passes by (pw_conv's
point_major / ci_lo, ci_hi / fin= / wide-layer pre-pass, devoxelize_affine's add=, minmax_act and affine_act_max on host-built
inputs); the arms of the voxel gathers and of the channels-last devoxelize that only an A/B switch reaches, in
tests/test_voxel_switch_arms_gpu.py. Still NOT held of fused.py: no wrapper that launches a kernel; operand_audit is a diagnostic around the wrappers
above whose own arithmetic is torch's.

Run time on an MI355X: 111 cases in 9.3 s on their own; the whole `-m gpu` suite took 293.9 s with this file in it (710 tests),
so about 285 s without it (the parent commit's 599 tests, same box, same run).
"""
import pytest
import torch

from oracle import cpu_ops, net_ref
from oracle.poison_arena import GuardViolation, PoisonArena

pytestmark = pytest.mark.gpu

ARENA_BYTES = 64 << 20  # enough for every shape below (the largest case, avg_voxelize at r = 32, carves ~30 MiB)
TOL = 1e-4  # test_fused_gpu.py


@pytest.fixture
def arena():
    with PoisonArena("cuda", ARENA_BYTES) as a:
        yield a


@pytest.fixture(scope="module")
def ext():
    from p2p_bridge_amd import pointnet2_batch_cuda

    return pointnet2_batch_cuda


@pytest.fixture(scope="module")
def met():
    from p2p_bridge_amd import metric_modules

    return metric_modules


@pytest.fixture(scope="module")
def fused():
    from p2p_bridge_amd import fused as f

    return f


def _tensors(out):
    if torch.is_tensor(out):
        return [out]
    if isinstance(out, (list, tuple)):
        return [t for o in out for t in _tensors(o)]
    return []


def run(arena, fn, *args, partial=(), **kwargs):
    """one wrapper call under the arena's checks 1-3; `partial`: positions in the flattened result that the ABI header
    documents as written in part (the caller cites the line and checks the written part itself)"""
    n0 = arena.n_allocations
    out = fn(*args, **kwargs)
    assert arena.n_allocations >= n0 + 1, f"{getattr(fn, '__name__', fn)} did not allocate through the arena"
    arena.check_guards()
    for k, t in enumerate(_tensors(out)):
        if k not in partial:
            arena.assert_written(t, f"{getattr(fn, '__name__', fn)} result {k}")
    return out


def put_module(arena, m):
    """a fresh nn module's parameters into the arena (poison around the weights too)"""
    for p in m.parameters():
        p.data = arena.put(p.data)
    return m


def eq(a, b, what=""):
    a, b = a.cpu(), b.cpu()
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert torch.equal(a, b), f"{what}: {(a != b).sum().item()} of {a.numel()} differ"


def rel_err(a, ref):
    a, ref = a.double().cpu(), ref.double().cpu()
    return ((a - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def cloud(B, N, seed=0):
    return net_ref.synthetic_patches(B, N, seed=seed)[0]


def swish(x):
    return x * torch.sigmoid(x)


def stats_of(st):
    s = st.double().cpu().sum(1)
    return s[..., 0], s[..., 1]


def test_planted_overrun_is_caught(arena, ext):
    """the net is live on the device: one float written one element past a returned output (through the arena's base
    tensor, no kernel altered) fails the guard check, and names that output: the input `c` has the same shape and type, so the
    message is held to the line that made the allocation too (the wrapper's, not this file's `put`)"""
    c = arena.put(cloud(1, 77, seed=77))
    norm, vox = run(arena, ext.voxel_coords, c, 4)
    r = [r for r in arena.records if r["start"] == norm.storage_offset() * 4][0]
    assert "pointnet2_batch_cuda.py:" in r["where"] and r["shape"] == (1, 3, 77)
    arena.base[r["end"]:r["end"] + 4].view(torch.float32)[0] = 1.0
    with pytest.raises(GuardViolation, match=r"last damaged byte at \+4 bytes from the allocation \(1, 3, 77\) float32 "
                                             rf"\[{r['start']}, {r['end']}\) made at \S*pointnet2_batch_cuda\.py:\d+"):
        arena.check_guards()
    arena.check_guards()


# ---- pointnet2_batch_cuda (references and tolerances: test_ops_parity_gpu.py, test_fps_grid_gpu.py) -----------------

@pytest.mark.parametrize("B,N,r", [(1, 77, 4), (2, 1001, 8)])
def test_voxel_coords(arena, ext, B, N, r):
    c = cloud(B, N, seed=N)
    n0, v0 = cpu_ops.voxel_coords(c, r)
    n1, v1 = run(arena, ext.voxel_coords, arena.put(c), r)
    eq(v1, v0, "vox"), eq(n1, n0, "norm")


@pytest.mark.parametrize("B,C,N,r", [(2, 5, 301, 4), (1, 7, 1001, 8), (2, 35, 1000, 32)])
def test_avg_voxelize(arena, ext, B, C, N, r):
    g = torch.Generator().manual_seed(N)
    c = cloud(B, N, seed=1)
    _, vox = cpu_ops.voxel_coords(c, r)
    f = torch.randn(B, C, N, generator=g)
    o0, i0, c0 = cpu_ops.avg_voxelize_forward(f, vox, r)
    o1, i1, c1 = run(arena, ext.avg_voxelize_forward, arena.put(f), arena.put(vox), r)
    eq(i1, i0, "ind"), eq(c1, c0, "cnt"), eq(o1, o0, "out")
    gy = torch.randn(B, C, r ** 3, generator=g)
    eq(run(arena, ext.avg_voxelize_backward, arena.put(gy), i1, c1), cpu_ops.avg_voxelize_backward(gy, i0, c0), "grad")


@pytest.mark.parametrize("B,C,N,r", [(1, 3, 77, 4), (2, 9, 1001, 8)])
@pytest.mark.parametrize("training", [False, True])
def test_trilinear_devoxelize(arena, ext, B, C, N, r, training):
    g = torch.Generator().manual_seed(r)
    c = cloud(B, N, seed=2)
    norm, _ = cpu_ops.voxel_coords(c, r)
    norm[:, :, :5] = torch.round(norm[:, :, :5])
    feat = torch.randn(B, C, r ** 3, generator=g)
    o0, i0, w0 = cpu_ops.trilinear_devoxelize_forward(r, training, norm, feat)
    o1, i1, w1 = run(arena, ext.trilinear_devoxelize_forward, r, training, arena.put(norm), arena.put(feat))
    eq(o1, o0, "outs")
    if training:
        eq(i1, i0, "inds"), eq(w1, w0, "wgts")
        gy = torch.randn(B, C, N, generator=g)
        g0 = cpu_ops.trilinear_devoxelize_backward(gy, i0, w0, r)
        g1 = run(arena, ext.trilinear_devoxelize_backward, arena.put(gy), i1, w1, r)
        assert torch.allclose(g1.cpu(), g0, rtol=1e-4, atol=1e-5)
    else:
        assert i1.numel() == 1 and w1.numel() == 1


@pytest.mark.parametrize("B,N,M,radius,U", [(1, 70, 9, 0.0, 32), (2, 301, 37, 0.4, 16)])
def test_ball_query_and_grouping(arena, ext, B, N, M, radius, U):
    c = cloud(B, N, seed=3)
    centers = cpu_ops.gather_features_forward(c, cpu_ops.furthest_point_sampling_forward(c, M))
    i0 = cpu_ops.ball_query(centers, c, radius, U)
    i1 = run(arena, ext.ball_query, arena.put(centers), arena.put(c), radius, U)
    eq(i1, i0, "ball idx")
    f = torch.randn(B, 19, N, generator=torch.Generator().manual_seed(5))
    eq(run(arena, ext.grouping_forward, arena.put(f), i1), cpu_ops.grouping_forward(f, i0), "grouping")
    gy = torch.randn(B, 19, M, U, generator=torch.Generator().manual_seed(6))
    g1 = run(arena, ext.grouping_backward, arena.put(gy), i1, N)
    assert torch.allclose(g1.cpu(), cpu_ops.grouping_backward(gy, i0, N), rtol=1e-4, atol=1e-4)
    g2 = run(arena, ext.grouping_backward_pitched, arena.put(gy), i1, N)
    assert torch.allclose(g2.cpu(), cpu_ops.grouping_backward(gy, i0, N), rtol=1e-4, atol=1e-4)


# (B, N, M, form): the wrapper takes the one-workgroup kernel up to 16384 points, above it `fps_big` picks the grid form
# (default), the cooperative form or the single-workgroup kernel with its distance workspace: 16385 is the smallest n of each
@pytest.mark.parametrize("B,N,M,form", [(2, 33, 1, None), (1, 1001, 257, None), (2, 16385, 5, "grid"), (2, 16385, 5, "coop"),
                                        (1, 16385, 5, "single"), (5, 16385, 3, "coop")])
def test_fps_and_gather(arena, ext, B, N, M, form, monkeypatch):
    if form is not None:
        monkeypatch.setenv("P2PB_EXPERIMENT", f"fps_big={form}")
    c = cloud(B, N, seed=N + M)
    i0 = cpu_ops.furthest_point_sampling_forward(c, M)
    dc = arena.put(c)
    monkeypatch.setattr(ext, "_last_coop_flags", None)
    n0 = arena.n_allocations
    i1 = run(arena, ext.furthest_point_sampling_forward, dc, M)
    eq(i1, i0, "fps idx")
    # the form asked for is the form that ran (the wrapper falls back to the single-workgroup kernel when the cooperative launch
    # is refused, and p2pb_fps_coop_ws_bytes would then be held to nothing): each form carves a workspace of its own kind
    made = [(r["dtype"], r["shape"]) for r in arena.records[n0:]]
    assert (ext._last_coop_flags is not None) == (form == "coop"), "cooperative FPS: launch refused, or taken unasked"
    if form == "coop":
        assert ext._last_coop_flags.numel() == B
        assert (torch.uint8, (int(ext.lib().p2pb_fps_coop_ws_bytes(B, N)),)) in made
    elif form == "grid":
        assert (torch.uint8, (int(ext.lib().p2pb_fps_grid_ws_bytes(B, N)),)) in made
    elif form == "single":
        assert (torch.float32, (B, N)) in made
    else:
        assert made == [(torch.int32, (B, M))]
    eq(run(arena, ext.gather_features_forward, dc, i1), cpu_ops.gather_features_forward(c, i0), "gather")
    gy = torch.randn(B, 3, M, generator=torch.Generator().manual_seed(1))
    eq(run(arena, ext.gather_features_backward, arena.put(gy), i1, N), cpu_ops.gather_features_backward(gy, i0, N), "gather grad")


# (B, C, M, N, cells): the wrapper's grid search (with its workspace) starts at 256 centres; 255 / 256 straddle it
@pytest.mark.parametrize("B,C,M,N,cells", [(1, 8, 1, 10, "0"), (2, 40, 37, 301, "0"), (2, 40, 37, 301, "1"), (2, 5, 255, 301, "1"),
                                           (2, 5, 256, 301, "1"), (1, 5, 257, 1001, "1")])
def test_three_nn_and_interpolate(arena, ext, B, C, M, N, cells, monkeypatch):
    monkeypatch.setenv("P2PB_EXPERIMENT", f"nn_cells={cells}")
    c = cloud(B, N, seed=7)
    centers = cpu_ops.gather_features_forward(c, cpu_ops.furthest_point_sampling_forward(c, M))
    f = torch.randn(B, C, M, generator=torch.Generator().manual_seed(8))
    o0, i0, w0 = cpu_ops.three_nearest_neighbors_interpolate_forward(c, centers, f)
    dc, dcen, df = arena.put(c), arena.put(centers), arena.put(f)
    i2, w2 = run(arena, ext.three_nn, dc, dcen)
    eq(i2, i0, "3nn idx (search)"), eq(w2, w0, "3nn w (search)")
    eq(run(arena, ext.three_interpolate, df, i2, w2), o0, "interp (half)")
    o1, i1, w1 = run(arena, ext.three_nearest_neighbors_interpolate_forward, dc, dcen, df)
    eq(i1, i0, "3nn idx"), eq(w1, w0, "3nn w"), eq(o1, o0, "interp")
    gy = torch.randn(B, C, N, generator=torch.Generator().manual_seed(9))
    g0 = cpu_ops.three_nearest_neighbors_interpolate_backward(gy, i0, w0, M)
    g1 = run(arena, ext.three_nearest_neighbors_interpolate_backward, arena.put(gy), i1, w1, M)
    assert torch.allclose(g1.cpu(), g0, rtol=1e-4, atol=1e-4)
    g2 = run(arena, ext.three_nearest_neighbors_interpolate_backward_pitched, arena.put(gy), i1, w1, M)
    assert torch.allclose(g2.cpu(), g0, rtol=1e-4, atol=1e-4)


def test_group_concat(arena, ext):
    """[xyz[idx] - centre ; f[idx]] (test_fused_gpu.py uses it as a reference itself): one fp32 subtraction per element, so the
    plain torch restatement is exact"""
    B, C, N, M, U = 2, 5, 300, 77, 16
    g = torch.Generator().manual_seed(N + C)
    xyz, f, centers = torch.randn(B, 3, N, generator=g), torch.randn(B, C, N, generator=g), torch.randn(B, 3, M, generator=g)
    idx = torch.randint(0, N, (B, M, U), generator=g, dtype=torch.int32)
    got = run(arena, ext.group_concat, arena.put(xyz), arena.put(centers), arena.put(f), arena.put(idx))
    take = lambda t: torch.gather(t, 2, idx.long().view(B, 1, M * U).expand(-1, t.shape[1], -1)).view(B, -1, M, U)
    eq(got, torch.cat([take(xyz) - centers[:, :, :, None], take(f)], 1), "group_concat")


# ---- metric_modules / metrics (references and tolerances: test_ops_parity_gpu.py) ------------------------------------

# (1, 1000, 4096): a small batch whose targets are split over several workgroups (test_chamfer_ties_across_target_chunks)
@pytest.mark.parametrize("B,N,M", [(1, 1, 7), (2, 100, 301), (1, 1000, 4096)])
def test_chamfer(arena, B, N, M):
    from p2p_bridge_amd import metrics

    g = torch.Generator().manual_seed(N)
    a, b_ = torch.rand(B, N, 3, generator=g), torch.rand(B, M, 3, generator=g)
    z = lambda n, dt: torch.zeros(B, n, dtype=dt)
    d1, d2, i1, i2 = z(N, torch.float32), z(M, torch.float32), z(N, torch.int32), z(M, torch.int32)
    cpu_ops.chamfer_forward(a, b_, d1, d2, i1, i2)
    da, db = arena.put(a).requires_grad_(), arena.put(b_).requires_grad_()
    D1, D2, I1, I2 = run(arena, metrics.chamfer_3DFunction.apply, da, db)
    eq(I1, i1, "idx1"), eq(I2, i2, "idx2"), eq(D1.detach(), d1, "dist1"), eq(D2.detach(), d2, "dist2")
    gd1, gd2 = torch.rand(B, N, generator=g), torch.rand(B, M, generator=g)
    g1, g2 = torch.zeros(B, N, 3), torch.zeros(B, M, 3)
    cpu_ops.chamfer_backward(a, b_, g1, g2, gd1, gd2, i1, i2)
    G1, G2 = run(arena, torch.autograd.grad, [D1, D2], [da, db], [arena.put(gd1), arena.put(gd2)])
    assert torch.allclose(G1.cpu(), g1, rtol=1e-4, atol=1e-5) and torch.allclose(G2.cpu(), g2, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("B,N,M", [(2, 300, 200), (1, 1024, 2048)])  # (the second takes the chunked launches)
def test_approxmatch_matchcost(arena, met, B, N, M):
    g = torch.Generator().manual_seed(0)
    a, b_ = torch.rand(B, N, 3, generator=g), torch.rand(B, M, 3, generator=g)
    m0 = cpu_ops.approxmatch_forward(a, b_)
    c0 = cpu_ops.matchcost_forward(a, b_, m0)
    da, db = arena.put(a), arena.put(b_)
    m1 = run(arena, met.emd_cuda.approxmatch_forward, da, db)
    c1 = run(arena, met.emd_cuda.matchcost_forward, da, db, m1)
    assert torch.allclose(m1.cpu(), m0, rtol=2e-3, atol=2e-5), (m1.cpu() - m0).abs().max()
    assert torch.allclose(c1.cpu(), c0, rtol=2e-3)
    gc = torch.rand(B, generator=g)
    r0 = cpu_ops.matchcost_backward(gc, a, b_, m0)
    r1 = run(arena, met.emd_cuda.matchcost_backward, arena.put(gc), da, db, m1)
    for x0, x1 in zip(r0, r1):
        assert torch.allclose(x1.cpu(), x0, rtol=5e-3, atol=1e-4)


def _auction(mod, x1, x2, eps, iters, device):
    b, n, _ = x1.shape
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=device)
    dist, assignment, inv = z(b, n), z(b, n, dt=torch.int32) - 1, z(b, n, dt=torch.int32) - 1
    rc = mod.forward(x1.to(device), x2.to(device), dist, assignment, z(b, n), inv, z(b, n, dt=torch.int32), z(b, n),
                     z(b, n), z(b * n, dt=torch.int32), z(512, dt=torch.int32), z(512, dt=torch.int32),
                     z(512, dt=torch.int32), z(b * n, dt=torch.int32), eps, iters)
    return rc, dist.cpu(), assignment.cpu()


@pytest.mark.parametrize("B,N", [(1, 128), (2, 256)])
def test_auction(arena, B, N):
    """the properties test_ops_parity_gpu.py::test_auction holds the (schedule-dependent) assignment to.
    Outside the net here: metrics.emdFunction builds `assignment` and `assignment_inv` as `torch.zeros(...) - 1`, and the result of
    that subtraction is allocated below Python, by the caching allocator: the returned assignment and its inverse have no guards
    (they are held by the value checks alone). The distances and the ten other buffers of the launch are carved and guarded."""
    from p2p_bridge_amd import metrics

    g = torch.Generator().manual_seed(0)
    x1, x2 = torch.rand(B, N, 3, generator=g), torch.rand(B, N, 3, generator=g)
    rc0, d0, _ = _auction(cpu_ops.emd_assignment, x1, x2, 0.01, 100, "cpu")
    assert rc0 == 1
    dx1, dx2 = arena.put(x1).requires_grad_(), arena.put(x2)
    d1, a1 = run(arena, metrics.emdFunction.apply, dx1, dx2, 0.01, 100)
    a = a1.long().cpu()
    assert a.min() >= 0 and a.max() < N
    x2a = torch.gather(x2, 1, a.unsqueeze(-1).expand(-1, -1, 3))
    assert torch.allclose(((x1 - x2a) ** 2).sum(-1), d1.detach().cpu(), atol=1e-6)
    for bi in range(B):
        assert a[bi].unique().numel() >= int(0.97 * N)
    c0, c1 = d0.sqrt().mean().item(), d1.detach().cpu().sqrt().mean().item()
    assert abs(c0 - c1) <= 0.03 * c0, (c0, c1)
    gd = torch.rand(B, N, generator=g)
    (gx,) = run(arena, torch.autograd.grad, [d1], [dx1], [arena.put(gd)])
    g0 = torch.zeros(B, N, 3)
    cpu_ops.auction_backward(x1, x2, g0, gd, a1.cpu())
    assert torch.allclose(gx.cpu(), g0, rtol=1e-5, atol=1e-6)


# ---- fused (references and tolerances: test_fused_gpu.py) -------------------------------------------------------------

@pytest.mark.parametrize("math", ["fp32", "bf16x6"])
@pytest.mark.parametrize("B,ci,co,P", [(3, 1, 7, 4), (2, 16, 16, 1021), (1, 259, 128, 516), (2, 67, 64, 333), (1, 8, 8, 513)])
def test_pw_conv(arena, fused, monkeypatch, math, B, ci, co, P):
    """(1, 8, 8, 513): one position more than a 512-position block, rows of 2052 bytes (no multiple of 16)"""
    monkeypatch.setattr(fused, "PW_SPLIT_MIN_CIN", 1)
    monkeypatch.setattr(fused, "PW_SPLIT_MIN_COUT", 1)
    torch.manual_seed(B * 1000 + ci + co + P)
    x = torch.randn(B, ci, P)
    conv = torch.nn.Conv1d(ci, co, 1)
    sc, sh, bias_b = torch.rand(B, ci) + 0.5, torch.randn(B, ci), torch.randn(B, co)
    with torch.no_grad():
        w, bias = conv.weight.double(), conv.bias.double()
        ref = torch.nn.functional.conv1d(x.double(), w, bias)
        ref2 = torch.nn.functional.conv1d(swish(x * sc[:, :, None] + sh[:, :, None]).double(), w, bias) + bias_b[:, :, None]
        ref3 = torch.nn.functional.conv1d((x * sc[:, :, None] + sh[:, :, None]).double(), w, bias)
        put_module(arena, conv)
        dx, dsc, dsh, dbb = arena.put(x), arena.put(sc), arena.put(sh), arena.put(bias_b)
        y0, st0 = run(arena, fused.pw_conv, dx, conv, stats=False, math=math)  # first: nothing left over from a stats call
        assert st0 is None and rel_err(y0, ref) < TOL
        y, st = run(arena, fused.pw_conv, dx, conv, math=math)
        assert torch.equal(y0, y)
        s1, s2 = stats_of(st)
        assert rel_err(s1, ref.sum(2)) < TOL * 10 or (s1 - ref.sum(2)).abs().max() < 1e-3
        assert rel_err(s2, (ref * ref).sum(2)) < TOL
        y2, st2 = run(arena, fused.pw_conv, dx, conv, dsc, dsh, swish=True, bias_b=dbb, math=math)
        assert rel_err(y2, ref2) < TOL
        assert rel_err(stats_of(st2)[1], (ref2 * ref2).sum(2)) < TOL
        assert rel_err(run(arena, fused.pw_conv, dx, conv, dsc, dsh, swish=False, math=math)[0], ref3) < TOL


@pytest.mark.parametrize("math", ["fp32", "bf16x6"])
def test_pw_conv_neighbour_pool(arena, fused, monkeypatch, math):
    monkeypatch.setattr(fused, "PW_SPLIT_MIN_CIN", 1)
    monkeypatch.setattr(fused, "PW_SPLIT_MIN_COUT", 1)
    B, ci, co, M, U = 1, 16, 200, 24, 16
    torch.manual_seed(M * U + ci)
    P = M * U
    assert fused.pool_supported(P, U)
    x = torch.randn(B, ci, P) * 2
    conv = torch.nn.Conv2d(ci, co, 1)
    sc, sh = torch.randn(B, co), torch.randn(B, co)
    with torch.no_grad():
        raw = torch.nn.functional.conv1d(x.double(), conv.weight.double().view(co, ci, 1), conv.bias.double())
        put_module(arena, conv)
        dx, dsc, dsh = arena.put(x), arena.put(sc), arena.put(sh)
        yfull, st_full = run(arena, fused.pw_conv, dx, conv, math=math)
        assert rel_err(yfull, raw) < TOL
        ref = swish(yfull.double().cpu() * sc[:, :, None].double() + sh[:, :, None].double()).view(B, co, M, U).amax(3)
        for store in (False, True):
            y, st, mm = run(arena, fused.pw_conv, dx, conv, pool_u=U, store=store, math=math)
            assert (y is None) == (not store)
            if store:
                assert torch.equal(y, yfull)
            assert torch.equal(st, st_full)
            got = run(arena, fused.minmax_act, mm, dsc, dsh)
            assert got.shape == (B, co, M) and rel_err(got, ref) < 1e-5


@pytest.mark.parametrize("math", ["fp32", "bf16x6"])
def test_pw_conv_global_pool(arena, fused, monkeypatch, math):
    monkeypatch.setattr(fused, "PW_SPLIT_MIN_CIN", 1)
    monkeypatch.setattr(fused, "PW_SPLIT_MIN_COUT", 1)
    B, ci, co, P = 1, 16, 24, 4
    torch.manual_seed(P + co)
    x = torch.randn(B, ci, P)
    conv = torch.nn.Conv2d(ci, co, 1)
    sc, sh = torch.randn(B, co), torch.randn(B, co)
    with torch.no_grad():
        put_module(arena, conv)
        dx, dsc, dsh = arena.put(x), arena.put(sc), arena.put(sh)
        y, st, mm = run(arena, fused.pw_conv, dx, conv, pool_u=0, store=False, math=math)
        yfull, st_full = run(arena, fused.pw_conv, dx, conv, math=math)
        assert y is None and torch.equal(st, st_full)
        ref = swish(yfull.double().cpu() * sc[:, :, None].double() + sh[:, :, None].double()).amax(2)
        got = run(arena, fused.minmax_act, mm, dsc, dsh, global_pool=True)
        assert got.shape == (B, co) and rel_err(got, ref) < 1e-5
        assert rel_err(got, run(arena, fused.affine_act_max, yfull, dsc, dsh, P, 0)) < 1e-5


@pytest.mark.parametrize("cl", [False, True])
@pytest.mark.parametrize("math", ["bf16x6", "fp32"])
@pytest.mark.parametrize("B,ci,co,r,compact", [(2, 11, 8, 8, False), (3, 3, 70, 8, False), (2, 8, 16, 4, False), (2, 35, 32, 32, True)])
def test_conv3d_k3(arena, fused, B, ci, co, r, compact, math, cl):
    torch.manual_seed(r + ci)
    x = torch.randn(B, ci, r, r, r)
    x[:, :, : r // 2] = 0  # an all-zero slab exercises the zero-tile skip
    conv = torch.nn.Conv3d(ci, co, 3, padding=1)
    sc, sh = torch.rand(B, ci) + 0.5, torch.randn(B, ci)
    back = (lambda t: t.permute(0, 4, 1, 2, 3)) if cl else (lambda t: t)
    kw = dict(compact=compact, math=math, force_split=math == "bf16x6", channels_last=cl)
    with torch.no_grad():
        ref = torch.nn.functional.conv3d(x.double(), conv.weight.double(), conv.bias.double(), padding=1)
        xin = swish(x * sc[:, :, None, None, None] + sh[:, :, None, None, None])
        ref2 = torch.nn.functional.conv3d(xin.double(), conv.weight.double(), conv.bias.double(), padding=1)
        put_module(arena, conv)
        xi = arena.put(x.permute(0, 2, 3, 4, 1) if cl else x)
        dsc, dsh = arena.put(sc), arena.put(sh)
        for skip in (False, True):
            y, st = run(arena, fused.conv3d_k3, xi, conv, skip_zero=skip, **kw)
            assert rel_err(back(y), ref) < TOL
            assert rel_err(stats_of(st)[1], (ref * ref).flatten(2).sum(2)) < TOL
        y2, _ = run(arena, fused.conv3d_k3, xi, conv, dsc, dsh, swish=True, **kw)
        assert rel_err(back(y2), ref2) < TOL


@pytest.mark.parametrize("r,C,C1,C2,N", [(8, 24, 160, 40, 300), (16, 19, 64, 200, 600)])
def test_conv3d_lists_compact_and_sparse(arena, fused, ext, r, C, C1, C2, N):
    """the list builders' outputs and workspaces, and the compact / sparse-list forms they drive, against the dense form
    (test_conv3d_compact_matches_dense, test_conv3d_sparse_lists_match_dense) and fp64"""
    torch.manual_seed(r + C)
    B = 3
    pts = torch.nn.functional.normalize(torch.randn(B, 3, N), dim=1) * 0.8 + 0.05 * torch.randn(B, 3, N)
    f = torch.randn(B, C, N)
    conv1, conv2 = torch.nn.Conv3d(C, C1, 3, padding=1), torch.nn.Conv3d(C1, C2, 3, padding=1)
    sc, sh = torch.rand(B, C1) + 0.5, torch.randn(B, C1)
    with torch.no_grad():
        w1, b1, w2, b2 = conv1.weight.double(), conv1.bias.double(), conv2.weight.double(), conv2.bias.double()
        put_module(arena, conv1), put_module(arena, conv2)
        _, vox = run(arena, ext.voxel_coords, arena.put(pts), r)
        grid, cnt = run(arena, fused.voxelize_cl, arena.put(f), vox, r)
        lists, counts = run(arena, fused.active_lists, cnt, r)
        nb = lists.shape[2]
        assert torch.equal(lists.long().sort(dim=-1).values, torch.arange(256, device="cuda").expand_as(lists))
        occ = (cnt.view(B, 1, r, r, r) > 0).float()
        d1 = torch.nn.functional.max_pool3d(occ, 3, 1, 1)
        d2 = torch.nn.functional.max_pool3d(d1, 3, 1, 1)
        for which, dset in enumerate((d1, d2)):
            bricks = dset.view(B, r // 4, 4, r // 8, 8, r // 8, 8).permute(0, 1, 3, 5, 2, 4, 6).reshape(B, nb, 256)
            assert torch.equal(bricks.sum(-1).int(), counts[which])
        ref1 = torch.nn.functional.conv3d(grid.double().cpu().permute(0, 4, 1, 2, 3), w1, b1, padding=1)
        y1d, st1d = run(arena, fused.conv3d_k3, grid, conv1, compact=True, channels_last=True, math="bf16x6")
        y1c, st1c = run(arena, fused.conv3d_k3_compact, grid, conv1, lists, counts, 0)
        assert torch.equal(y1c, y1d) and rel_err(y1c.permute(0, 4, 1, 2, 3), ref1) < TOL
        assert rel_err(stats_of(st1c)[1], stats_of(st1d)[1]) < 1e-5
        dsc, dsh = arena.put(sc), arena.put(sh)
        a, k = run(arena, fused.conv3d_far_field, conv1.bias, conv2, dsc, dsh, True)
        y2d, st2d = run(arena, fused.conv3d_k3, y1d, conv2, dsc, dsh, swish=True, compact=True, channels_last=True, math="bf16x6",
                        in_sub=a, out_class=k)
        y2c, st2c = run(arena, fused.conv3d_k3_compact, y1c, conv2, lists, counts, 1, dsc, dsh, True, in_sub=a, out_class=k)
        assert torch.equal(y2c, y2d)
        assert rel_err(stats_of(st2c)[1], stats_of(st2d)[1]) < 1e-5
        xin = swish(y1d.double().cpu() * sc[:, None, None, None, :] + sh[:, None, None, None, :]).permute(0, 4, 1, 2, 3)
        assert rel_err(y2c.permute(0, 4, 1, 2, 3), torch.nn.functional.conv3d(xin, w2, b2, padding=1)) < TOL
        # listed_only: y is written in part. include/p2pb_hip.h, p2pb_conv3d_k3_forward_compact: "flags bit 5 (32 ...): the
        # constants of the UNLISTED voxels are left unwritten (statistics still exact)". The listed part (D2) and the statistics
        # are held to the full form's bits; the guards are checked as for every other call.
        y2l, st2l = run(arena, fused.conv3d_k3_compact, y1c, conv2, lists, counts, 1, dsc, dsh, True, in_sub=a, out_class=k,
                        listed_only=True, partial=(0,))
        in_d2 = (d2.view(B, r, r, r) > 0)
        assert torch.equal(st2l, st2c) and torch.equal(y2l[in_d2], y2c[in_d2])


def _brick_any(mask, r):
    """mask bool[B,r,r,r] -> bool[B * NBRICK]: does the 4x8x8 brick (sample * NBRICK + brick, as the brick lists number them) hold
    a voxel of the mask"""
    B = mask.shape[0]
    return mask.view(B, r // 4, 4, r // 8, 8, r // 8, 8).permute(0, 1, 3, 5, 2, 4, 6).reshape(B * (r // 4) * (r // 8) ** 2, 256).any(1)


_SPARSE = {}


def sparse_case(B, ci, co, r):
    """host inputs and the fp64 result of one list-driven convolution, built once per shape and shared by its cases (never
    modified): an occupancy that leaves bricks without work -- a sparse slab that ends one voxel past a brick face, of another
    depth in every sample, and one voxel in the far corner --, features on the occupied voxels only"""
    key = (B, ci, co, r)
    if key not in _SPARSE:
        g = torch.Generator().manual_seed(r + ci)
        occ = torch.zeros(B, r, r, r, dtype=torch.bool)
        for b in range(B):
            k = r // 4 + 1 + b
            occ[b, :k, : r // 2 + 1, : r // 2 - 1] = torch.rand(k, r // 2 + 1, r // 2 - 1, generator=g) < 0.1
        occ[-1, -1, -1, -1] = True
        x = torch.randn(B, ci, r, r, r, generator=g) * occ[:, None]
        w, bias = torch.randn(co, ci, 3, 3, 3, generator=g) / (27 * ci) ** 0.5, torch.randn(co, generator=g)
        ref = torch.nn.functional.conv3d(x.double(), w.double(), bias.double(), padding=1)
        d1 = torch.nn.functional.max_pool3d(occ[:, None].float(), 3, 1, 1)
        d2 = torch.nn.functional.max_pool3d(d1, 3, 1, 1)
        active = [_brick_any(d[:, 0] > 0, r).nonzero().flatten().int() for d in (d1, d2)]  # work <=> occupancy within brick +- 1 / 2
        _SPARSE[key] = (x, occ.view(B, -1).int(), w, bias, ref, active)
    return _SPARSE[key]


def _conv_from(w, bias):
    conv = torch.nn.Conv3d(w.shape[1], w.shape[0], 3, padding=1)  # a fresh module per case: packs are cached on it
    with torch.no_grad():
        conv.weight.copy_(w), conv.bias.copy_(bias)
    return conv


def _check_brick_lists(lists, counts, active, total):
    """the builder's four lists against the occupancy: {active, inactive} of the first and of the second convolution partition
    the (sample, brick) pairs, and the active ones are those within one / two voxels of an occupied voxel. The entries behind
    a list's count are scratch."""
    for which in (0, 1):
        na, ni = int(counts[2 * which]), int(counts[2 * which + 1])
        assert na + ni == total and 0 < na < total, (which, na, ni)
        eq(lists[2 * which, :na].sort().values, active[which], f"active bricks, convolution {which}")
        both = torch.cat([lists[2 * which, :na], lists[2 * which + 1, :ni]]).sort().values
        eq(both, torch.arange(total, dtype=torch.int32), f"brick partition, convolution {which}")


# the list-driven sparse form behind brick_lists (r in {16, 32}): the one shape of the table it accepts, and the r = 16 case
@pytest.mark.parametrize("cl", [False, True])
@pytest.mark.parametrize("math", ["bf16x6", "fp32"])
@pytest.mark.parametrize("B,ci,co,r", [(2, 35, 32, 32), (3, 19, 64, 16)])
def test_conv3d_k3_sparse(arena, fused, B, ci, co, r, math, cl):
    """list-driven sparse form == dense form (bits) and == fp64 (TOL), as test_conv3d_sparse_lists_match_dense, in the
    channel-major layout (y f32[B,Cout,r,r,r], no flag 8) and the voxel-major one, in both maths"""
    x, cnt, w, bias, ref, active = sparse_case(B, ci, co, r)
    conv = put_module(arena, _conv_from(w, bias))
    back = (lambda t: t.permute(0, 4, 1, 2, 3)) if cl else (lambda t: t)
    with torch.no_grad():
        xi = arena.put(x.permute(0, 2, 3, 4, 1) if cl else x)
        lists, counts = run(arena, fused.brick_lists, arena.put(cnt), r)
        assert lists.shape == (4, B * {32: 128, 16: 16}[r])
        _check_brick_lists(lists, counts, active, lists.shape[1])
        ys, sts = run(arena, fused.conv3d_k3_sparse, xi, conv, lists, counts, 0, math=math, channels_last=cl)
        yd, std = run(arena, fused.conv3d_k3, xi, conv, compact=True, math=math, channels_last=cl)
        assert ys.shape == ((B, r, r, r, co) if cl else (B, co, r, r, r))
        assert torch.equal(ys, yd)
        assert rel_err(back(ys), ref) < TOL
        assert rel_err(stats_of(sts)[1], stats_of(std)[1]) < 1e-6
        assert rel_err(stats_of(sts)[1], (ref * ref).flatten(2).sum(2)) < TOL


@pytest.mark.parametrize("math", ["bf16x6", "fp32"])
def test_conv3d_k3_sparse_second_convolution_and_active_only(arena, fused, math):
    """a PVConv's second convolution in list-driven far-field form (in_sub / out_class of conv3d_far_field, halo-2 lists) against
    the dense far-field form (bits) and fp64 (TOL), then `active_only`, whose y is written in part. include/p2pb_hip.h,
    p2pb_conv3d_k3_forward_sparse: "flags bit 5 (32): the inactive bricks' STATISTICS only -- their outputs are left unwritten,
    for a caller that reads `out` inside the active bricks alone". The active bricks and the statistics are held to the full
    form's bits."""
    B, ci, c1, c2, r = 3, 19, 24, 40, 16
    x, cnt, w, bias, _, active = sparse_case(B, ci, c1, r)
    g = torch.Generator().manual_seed(c2)
    w2, bias2 = torch.randn(c2, c1, 3, 3, 3, generator=g) / (27 * c1) ** 0.5, torch.randn(c2, generator=g)
    sc, sh = torch.rand(B, c1, generator=g) + 0.5, torch.randn(B, c1, generator=g)
    conv1, conv2 = put_module(arena, _conv_from(w, bias)), put_module(arena, _conv_from(w2, bias2))
    with torch.no_grad():
        lists, counts = run(arena, fused.brick_lists, arena.put(cnt), r)
        _check_brick_lists(lists, counts, active, lists.shape[1])
        y1, _ = run(arena, fused.conv3d_k3_sparse, arena.put(x.permute(0, 2, 3, 4, 1)), conv1, lists, counts, 0, math=math,
                    channels_last=True)
        dsc, dsh = arena.put(sc), arena.put(sh)
        a, k = run(arena, fused.conv3d_far_field, conv1.bias, conv2, dsc, dsh, True)
        kw = dict(in_sub=a, out_class=k, math=math, channels_last=True)
        y2, st2 = run(arena, fused.conv3d_k3_sparse, y1, conv2, lists, counts, 1, dsc, dsh, True, **kw)
        y2d, st2d = run(arena, fused.conv3d_k3, y1, conv2, dsc, dsh, swish=True, compact=True, **kw)
        assert torch.equal(y2, y2d) and rel_err(stats_of(st2)[1], stats_of(st2d)[1]) < 1e-6
        xin = swish(y1.double().cpu() * sc[:, None, None, None, :] + sh[:, None, None, None, :]).permute(0, 4, 1, 2, 3)
        assert rel_err(y2.permute(0, 4, 1, 2, 3), torch.nn.functional.conv3d(xin, w2.double(), bias2.double(), padding=1)) < TOL
        y2a, st2a = run(arena, fused.conv3d_k3_sparse, y1, conv2, lists, counts, 1, dsc, dsh, True, active_only=True, partial=(0,),
                        **kw)
        on = torch.zeros(lists.shape[1], dtype=torch.bool)
        on[active[1].long()] = True
        bricks = lambda t: t.cpu().view(B, r // 4, 4, r // 8, 8, r // 8, 8, c2).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(-1, 256, c2)
        assert torch.equal(st2a, st2) and torch.equal(bricks(y2a)[on], bricks(y2)[on])


@pytest.mark.parametrize("B,C,N,r", [(1, 16, 64, 4), (3, 200, 300, 8)])
def test_voxelize_cl_devoxelize_cl(arena, fused, ext, B, C, N, r):
    torch.manual_seed(N + C)
    pts, f = torch.randn(B, 3, N), torch.randn(B, C, N)
    a, b = torch.randn(B, C), torch.randn(B, C)
    dense = torch.randn(B, C, r, r, r)
    vc0, vox0 = cpu_ops.voxel_coords(pts, r)
    grid_ref, _, cnt_ref = cpu_ops.avg_voxelize_forward(f, vox0, r)
    plain = cpu_ops.trilinear_devoxelize_forward(r, False, vc0, dense.view(B, C, -1).contiguous())[0]
    vcoords, vox = run(arena, ext.voxel_coords, arena.put(pts), r)
    grid, cnt = run(arena, fused.voxelize_cl, arena.put(f), vox, r)
    assert grid.shape == (B, r, r, r, C)
    eq(cnt, cnt_ref, "cnt"), eq(grid.permute(0, 4, 1, 2, 3).reshape(B, C, -1), grid_ref, "grid")
    da, db, dd = arena.put(a), arena.put(b), arena.put(dense)
    dcl = arena.put(dense.permute(0, 2, 3, 4, 1))
    want = run(arena, fused.devoxelize_affine, dd, vcoords, r, da, db)
    got = run(arena, fused.devoxelize_affine, dcl, vcoords, r, da, db, channels_last=True)
    assert torch.equal(got, want)
    assert rel_err(want, plain.double() * a[:, :, None].double() + b[:, :, None].double()) < 1e-5
    ones, zeros = arena.put(torch.ones(B, C)), arena.put(torch.zeros(B, C))
    eq(run(arena, fused.devoxelize_affine, dcl, vcoords, r, ones, zeros, channels_last=True), plain, "identity affine")


@pytest.mark.parametrize("groups,style,want_mean", [(8, False, False), (8, True, False), (4, True, True), (8, False, True)])
def test_gn_affine_params(arena, fused, groups, style, want_mean):
    torch.manual_seed(11)
    B, C, P = 3, 64, 1000
    x = torch.randn(B, C, P) * 3 + 1
    conv = torch.nn.Conv1d(C, C, 1)
    gn = torch.nn.GroupNorm(groups, C)
    bank = torch.randn(B, 2 * C + 40)
    with torch.no_grad():
        gn.weight.normal_(), gn.bias.normal_()
        y0 = conv(x)
        ref = gn(y0)
        if style:
            ref = ref * bank[:, 24:24 + C, None] + bank[:, 24 + C:24 + 2 * C, None]
        put_module(arena, conv), put_module(arena, gn)
        y, st = run(arena, fused.pw_conv, arena.put(x), conv)
        dbank = arena.put(bank)
        sty = dbank[:, 24:24 + 2 * C] if style else None
        sc, sh, mean = run(arena, fused.gn_affine_params, st, P, groups, gn.weight, gn.bias, sty, gn.eps, want_mean=want_mean)
        assert rel_err(y * sc[:, :, None] + sh[:, :, None], ref) < TOL
        if want_mean:  # per-(sample, channel) mean of the normalised output
            assert rel_err(mean, ref.mean(2)) < TOL


@pytest.mark.parametrize("b,ci,co,wide", [(1, 1024, 96, 0), (2, 64, 64, 0), (5, 256, 512, 128), (17, 4, 3, 4)])
def test_linear_rows(arena, fused, b, ci, co, wide):
    """(17, 4, 3, 4): the smallest row the ABI takes (cin % 4 == 0, 16-byte aligned rows: include/p2pb_hip.h), 17 batch rows,
    output rows of 12 bytes"""
    torch.manual_seed(b + ci + co)
    x = torch.randn(b, ci)
    wfull = torch.randn(co, wide + ci) / ci ** 0.5
    bias = torch.randn(co) if co % 2 == 0 else None
    w = wfull[:, wide:]
    ref = x.double() @ w.double().t() + (bias.double() if bias is not None else 0.0)
    mag = x.double().abs() @ w.double().abs().t() + 1.0
    dw = arena.put(wfull)[:, wide:]
    y = run(arena, fused.linear_rows, arena.put(x), dw, arena.put(bias) if bias is not None else None)
    assert y.shape == (b, co)
    assert ((y.double().cpu() - ref).abs() / mag).max().item() < 2e-6


@pytest.mark.parametrize("b,c,n,m,u", [(1, 24, 64, 5, 8), (2, 7, 33, 3, 43)])
def test_group_sub(arena, fused, b, c, n, m, u):
    """(2, 7, 33, 3, 43): 129 positions = one more than a 128-position statistics slot, 28-byte rows"""
    torch.manual_seed(b * 100 + c)
    zt, cxt = torch.randn(b, n, c), torch.randn(b, m, c)
    idx = torch.randint(0, n, (b, m, u), dtype=torch.int32)
    g = zt.double()[torch.arange(b)[:, None, None], idx.long()] - cxt.double()[:, :, None, :]  # [b, m, u, c]
    ref = torch.stack([g.sum(dim=(1, 2)), (g * g).sum(dim=(1, 2))], dim=-1)  # [b, c, 2]
    dz, dcx, didx = arena.put(zt), arena.put(cxt), arena.put(idx)
    none, st = run(arena, fused.group_sub, dz, dcx, didx, point_major=True, stats_only=True)
    assert none is None and st.shape == (b, (m * u + 127) // 128, c, 2)
    y, st_full = run(arena, fused.group_sub, dz, dcx, didx, point_major=True)
    got = st.double().cpu().sum(1)
    assert torch.allclose(got, ref, rtol=1e-5, atol=1e-3), (got - ref).abs().max().item()
    assert torch.allclose(got, st_full.double().cpu().sum(1), rtol=1e-5, atol=1e-3)
    assert torch.allclose(y.double().cpu(), g.permute(0, 3, 1, 2).reshape(b, c, m * u), atol=1e-6)
    y_cm, st_cm = run(arena, fused.group_sub, arena.put(zt.transpose(1, 2)), arena.put(cxt.transpose(1, 2)), didx)
    assert torch.allclose(y_cm.double().cpu(), g.permute(0, 3, 1, 2).reshape(b, c, m * u), atol=1e-6)
    assert torch.allclose(st_cm.double().cpu().sum(1), ref, rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("B,C", [(1, 40), (3, 64)])
def test_se_gate_affine(arena, fused, B, C):
    torch.manual_seed(C)
    fc = torch.nn.Sequential(torch.nn.Linear(C, C // 8, bias=False), torch.nn.ReLU(), torch.nn.Linear(C // 8, C, bias=False),
                             torch.nn.Sigmoid())
    mean, sc, sh = (torch.randn(B, C) for _ in range(3))
    with torch.no_grad():
        gate = fc(mean)
        put_module(arena, fc)
        a, b = run(arena, fused.se_gate_affine, arena.put(mean), fc[0].weight, fc[2].weight, arena.put(sc), arena.put(sh))
        assert rel_err(a, sc * gate) < 1e-5 and rel_err(b, sh * gate) < 1e-5


# ---- dense (references and tolerances: test_dense_train_gpu.py, default P2PB_TRAIN_MATH = bf16x3) -----------------------

def _rel(a, b):
    return (a.double().cpu() - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def _grads(arena, outs, leaves, gouts):
    """autograd through the hand-written backward, inside the arena: every gradient buffer and workspace is carved"""
    return run(arena, torch.autograd.grad, outs, leaves, gouts)


@pytest.mark.parametrize("b,ci,co,r", [(2, 11, 8, 8), (3, 3, 70, 8), (2, 8, 16, 4)])
def test_dense_conv3d_k3(arena, b, ci, co, r):
    from p2p_bridge_amd import dense

    torch.manual_seed(b * 1000 + ci + co + r)
    conv = torch.nn.Conv3d(ci, co, 3, padding=1)
    x = torch.randn(b, ci, r, r, r) * (torch.rand(b, 1, r, r, r) < 0.3).float()
    gy = torch.randn(b, co, r, r, r)
    x64 = x.double().requires_grad_(True)
    w64, b64 = conv.weight.detach().double().requires_grad_(True), conv.bias.detach().double().requires_grad_(True)
    y64 = torch.nn.functional.conv3d(x64, w64, b64, padding=1)
    y64.backward(gy.double())
    put_module(arena, conv)
    dx = arena.put(x).requires_grad_()
    y = run(arena, dense.conv3d_k3, dx, conv)
    gx, gw, gb = _grads(arena, [y], [dx, conv.weight, conv.bias], [arena.put(gy)])
    assert _rel(y.detach(), y64.detach()) < 5e-6
    assert _rel(gx, x64.grad) < 1e-4 and _rel(gw, w64.grad) < 1e-4 and _rel(gb, b64.grad) < 5e-6


def test_dense_conv3d_occupied_voxel_weight_gradient(arena):
    from p2p_bridge_amd import dense, layers as L

    b, ci, co, r, n = 2, 24, 40, 16, 300
    torch.manual_seed(b * 1000 + ci)
    feats = torch.randn(b, ci, n)
    vox = torch.randint(0, r, (b, 3, n), dtype=torch.int32)
    vox[:, :, : n // 8] = torch.randint(0, 2, (b, 3, n // 8), dtype=torch.int32) * (r - 1)  # corners / faces
    conv = torch.nn.Conv3d(ci, co, 3, padding=1)
    gy = torch.randn(b, co, r, r, r)
    w64, b64 = conv.weight.detach().double().requires_grad_(True), conv.bias.detach().double().requires_grad_(True)
    put_module(arena, conv)
    dfe, dvox = arena.put(feats).requires_grad_(), arena.put(vox)
    x = run(arena, L.avg_voxelize, dfe, dvox, r)
    assert getattr(x, "_p2pb_occ", None) is not None
    y = run(arena, dense.conv3d_k3, x, conv)
    gw, gb, gf = _grads(arena, [y], [conv.weight, conv.bias, dfe], [arena.put(gy)])
    y64 = torch.nn.functional.conv3d(x.detach().double().cpu(), w64, b64, padding=1)
    rw, rb = torch.autograd.grad(y64, [w64, b64], gy.double())
    scale = rw.abs().max().item() + 1e-30
    assert (gw.double().cpu() - rw).abs().max().item() < 2e-6 * scale * max(1.0, (n * b) ** 0.5 / 10)
    assert torch.allclose(gb.double().cpu(), rb, rtol=1e-4, atol=1e-3 * rb.abs().max().item())


@pytest.mark.parametrize("b,ci,co,shape", [(1, 256, 384, (8, 1)), (3, 67, 64, (128, 32)), (8, 128, 3, (2048,)), (2, 5, 7, (513,))])
def test_dense_pointwise(arena, b, ci, co, shape):
    """(2, 5, 7, (513,)): odd channel counts, one position past a 512-position block, 2052-byte rows"""
    from p2p_bridge_amd import dense

    torch.manual_seed(ci + co)
    conv = (torch.nn.Conv1d if len(shape) == 1 else torch.nn.Conv2d)(ci, co, 1)
    x, gy = torch.randn(b, ci, *shape), torch.randn(b, co, *shape)
    x64 = x.double().reshape(b, ci, -1).requires_grad_(True)
    w64 = conv.weight.detach().double().reshape(co, ci).requires_grad_(True)
    b64 = conv.bias.detach().double().requires_grad_(True)
    y64 = torch.einsum("oc,bcp->bop", w64, x64) + b64[None, :, None]
    y64.backward(gy.double().reshape(b, co, -1))
    put_module(arena, conv)
    dx = arena.put(x).requires_grad_()
    y = run(arena, dense.pointwise, dx, conv)
    assert y.shape == gy.shape
    gx, gw, gb = _grads(arena, [y], [dx, conv.weight, conv.bias], [arena.put(gy)])
    assert _rel(y.detach().reshape(b, co, -1), y64.detach()) < 5e-6
    assert _rel(gx.reshape(b, ci, -1), x64.grad) < 1e-4
    assert _rel(gw.reshape(co, ci), w64.grad) < 1e-4
    assert _rel(gb, b64.grad) < 5e-6


@pytest.mark.parametrize("kind,b,ci,co,shape", [("gn1d", 2, 24, 40, (300,)), ("adagn3d", 2, 16, 64, (8, 8, 8))])
@pytest.mark.parametrize("act", [True, False])
def test_dense_conv_norm_act(arena, kind, b, ci, co, shape, act):
    from p2p_bridge_amd import dense
    from p2p_bridge_amd.pvcnn_unet import AdaGN

    F = torch.nn.functional
    torch.manual_seed(len(kind) * 100 + co)
    conv = {"3d": torch.nn.Conv3d(ci, co, 3, padding=1), "1d": torch.nn.Conv1d(ci, co, 1)}[kind[-2:]]
    norm = AdaGN(co, 48, len(shape), 8) if kind.startswith("adagn") else torch.nn.GroupNorm(8, co)
    cond = torch.randn(b, 48) if kind.startswith("adagn") else None
    gn = norm.norm if isinstance(norm, AdaGN) else norm
    with torch.no_grad():
        gn.weight.uniform_(0.5, 1.5)
        gn.bias.normal_()
    x = torch.randn(b, ci, *shape)
    d = lambda t: t.detach().double().requires_grad_(True)
    x64, w64, cb64, ga64, be64 = d(x), d(conv.weight), d(conv.bias), d(gn.weight), d(gn.bias)
    h = F.conv3d(x64, w64, cb64, padding=1) if kind.endswith("3d") else F.conv1d(x64, w64, cb64)
    h = F.group_norm(h, gn.num_groups, ga64, be64, gn.eps)
    ref = {"x": x64, "w": w64, "cb": cb64, "gamma": ga64, "beta": be64}
    if cond is not None:
        c64, ew64, eb64 = d(cond), d(norm.emd.weight), d(norm.emd.bias)
        fac, bia = F.linear(c64, ew64, eb64).reshape(b, 2 * co, *([1] * len(shape))).chunk(2, 1)
        h = h * fac + bia
        ref.update(cond=c64, ew=ew64, eb=eb64)
    y64 = h * torch.sigmoid(h) if act else h
    gy = torch.randn(y64.shape)
    y64.backward(gy.double())
    put_module(arena, conv), put_module(arena, norm)
    dx = arena.put(x).requires_grad_()
    dcond = arena.put(cond).requires_grad_() if cond is not None else None
    y = run(arena, dense.conv_norm_act, dx, conv, norm, dcond, act)
    leaves = {"x": dx, "w": conv.weight, "cb": conv.bias, "gamma": gn.weight, "beta": gn.bias}
    if cond is not None:
        leaves.update(cond=dcond, ew=norm.emd.weight, eb=norm.emd.bias)
    got = dict(zip(leaves, _grads(arena, [y], list(leaves.values()), [arena.put(gy)])))
    assert _rel(y.detach(), y64.detach()) < 1e-5
    for k, v in ref.items():
        if k == "cb":  # sums of dx over a channel: heavy cancellation (test_conv_norm_act_forward_backward)
            err = (got[k].double().cpu() - v.grad).abs().max().item()
            assert err < 1e-5 * max(1.0, got["x"].abs().max().item() * x[0, 0].numel() ** 0.5), (k, err)
            continue
        assert _rel(got[k], v.grad) < (2e-4 if k == "w" else 5e-5), (k, _rel(got[k], v.grad))


@pytest.mark.parametrize("shape", [(5, 7, 33), (2, 3, 1), (1, 2, 300, 6)])
def test_dense_row_max(arena, shape):
    from p2p_bridge_amd import dense

    torch.manual_seed(sum(shape))
    x = torch.randn(*shape)
    x[..., 0, :] = x[..., 0, :].round()  # exact ties in the first row of every slab
    vb, _ = x.max(dim=-1)
    gy = torch.randn(vb.shape)
    first = (x == vb.unsqueeze(-1)).float().argmax(dim=-1)
    want = torch.zeros_like(x).scatter_(-1, first.unsqueeze(-1), gy.unsqueeze(-1))
    dx = arena.put(x).requires_grad_()
    ya = run(arena, dense.row_max, dx)
    eq(ya.detach(), vb, "row max")
    (gx,) = _grads(arena, [ya], [dx], [arena.put(gy)])
    eq(gx, want, "row max grad")


def test_dense_se_gate(arena):
    from p2p_bridge_amd import dense
    from p2p_bridge_amd.pvcnn_unet import SE3d

    b, c = 2, 32
    torch.manual_seed(c + b)
    se = SE3d(c)
    mean, dg = torch.randn(b, c), torch.randn(b, c)
    m64 = mean.double().requires_grad_(True)
    w1, w2 = (se.fc[i].weight.detach().double().requires_grad_(True) for i in (0, 2))
    g64 = torch.sigmoid(torch.relu(m64 @ w1.t()) @ w2.t())
    g64.backward(dg.double())
    put_module(arena, se)
    dm = arena.put(mean).requires_grad_()
    g = run(arena, dense.se_gate, dm, se.fc)
    gm, g1, g2 = _grads(arena, [g], [dm, se.fc[0].weight, se.fc[2].weight], [arena.put(dg)])
    assert _rel(g.detach(), g64.detach()) < 1e-6
    assert _rel(gm, m64.grad) < 1e-5 and _rel(g1, w1.grad) < 1e-5 and _rel(g2, w2.grad) < 1e-5


# ---- denoise, denoise_room (references: test_denoise_gpu.py, test_room_gpu.py -- all bit-exact) -----------------------

def room(n, seed=0):
    """a synthetic room: floor + two walls + clutter, metres (test_room_gpu.py)"""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(n, 3, generator=g)
    which = torch.randint(0, 4, (n,), generator=g)
    p = torch.stack([u[:, 0] * 4.0, u[:, 1] * 3.0, u[:, 2] * 2.5], 1)
    p[which == 0, 2] = 0.0
    p[which == 1, 0] = 0.0
    p[which == 2, 1] = 3.0
    return (p + 0.005 * torch.randn(n, 3, generator=g)).contiguous()


@pytest.mark.parametrize("B,S,N,K", [(1, 1, 100, 37), (2, 3, 700, 1), (1, 2, 700, 700), (1, 5, 1025, 513)])
def test_knn_points(arena, B, S, N, K):
    from p2p_bridge_amd import denoise as dn

    pts = torch.stack([room(N, seed=10 * B + i) for i in range(B)])
    q = pts[:, torch.arange(S) * (N // S)].contiguous()
    d_ref, i_ref, nn_ref = cpu_ops.knn_points(q, pts, K)
    dq, dp = arena.put(q), arena.put(pts)
    out = run(arena, dn.knn_points, dq, dp, K=K, return_nn=True)
    eq(out.idx, i_ref, "knn idx"), eq(out.dists, d_ref, "knn dists"), eq(out.knn, nn_ref, "knn points")
    out = run(arena, dn.knn_points, dq, dp, K=K)
    assert out.knn is None
    eq(out.idx, i_ref, "knn idx"), eq(out.dists, d_ref, "knn dists")


@pytest.mark.parametrize("n,s,r", [(777, 3, 10.0), (1000, 5, 0.0), (1000, 5, 0.3)])
def test_radius_query(arena, n, s, r):
    from p2p_bridge_amd import denoise_room as R

    pts = room(n, seed=n)
    cen = pts[torch.randperm(n, generator=torch.Generator().manual_seed(1))[:s]].contiguous()
    ref_idx, ref_off = cpu_ops.radius_query(cen, pts, r)
    idx, off = run(arena, R.radius_query, arena.put(cen), arena.put(pts), r)
    eq(off, ref_off, "offsets"), eq(idx, ref_idx, "radius idx")


def test_merge_accumulate_and_finish(arena):
    from p2p_bridge_amd import denoise_room as R

    pts = room(3001, seed=3)
    cidx = cpu_ops.furthest_point_sampling_forward(pts.t().contiguous()[None], 7)[0].long()
    idx_flat, offsets = cpu_ops.radius_query(pts[cidx].contiguous(), pts, 0.5)
    ref_xyz, ref_idx, ref_cuts = cpu_ops.room_create_patches(pts, idx_flat, offsets, 256, torch.Generator().manual_seed(7))
    pred = ref_xyz + 0.01 * torch.randn(ref_xyz.shape, generator=torch.Generator().manual_seed(9))
    den, num = cpu_ops.room_merge(pts, pred, ref_idx, ref_cuts)
    m = run(arena, R.RunningMean, arena.put(pts))
    half = pred.shape[0] // 2  # two batches add into the same accumulators
    m.update(arena.put(pred[:half]), arena.put(ref_idx[:half]), ref_cuts[:half])
    m.update(arena.put(pred[half:]), arena.put(ref_idx[half:]), ref_cuts[half:])
    out = run(arena, m.result).cpu()
    assert torch.equal(m.counts.cpu().long(), num.long())
    assert (out.double() - den).abs().max().item() < 1e-6
    assert torch.equal(out[num == 0], pts[num == 0])


# ---- attention (references: test_sampler_features_gpu.py, test_softmax_attention_gpu.py) ------------------------------

@pytest.mark.parametrize("b,heads,n", [(1, 4, 8), (3, 12, 195)])
def test_linear_attention_core(arena, b, heads, n):
    from p2p_bridge_amd.pvcnn_unet import _LinearAttentionCore

    torch.manual_seed(b * 100 + n)
    qkv = torch.randn(b, 3 * heads * 32, n) * 2
    q64 = qkv.double().requires_grad_(True)
    q, k, v = q64.view(b, 3, heads, 32, n).unbind(1)
    ref = torch.einsum("bhde,bhdn->bhen", torch.einsum("bhdn,bhen->bhde", k.softmax(dim=-1), v), q).reshape(b, -1, n)
    gy = torch.randn(ref.shape)
    ref.backward(gy.double())
    dqkv = arena.put(qkv).requires_grad_()
    out = run(arena, _LinearAttentionCore.apply, dqkv, heads)
    (g,) = _grads(arena, [out], [dqkv], [arena.put(gy)])
    assert (out.detach().cpu().double() - ref.detach()).abs().max().item() < 1e-5 * max(1.0, ref.abs().max().item())
    assert (g.cpu().double() - q64.grad).abs().max().item() < 2e-5 * max(1.0, q64.grad.abs().max().item())


@pytest.mark.parametrize("b,heads,n", [(1, 4, 1), (1, 4, 8), (3, 12, 195)])  # (195 keys: a ragged last key tile)
def test_softmax_attention_core(arena, b, heads, n):
    from p2p_bridge_amd.pvcnn_unet import _SoftmaxAttentionCore
    from test_attention_types import core64

    torch.manual_seed(b * 100 + n)
    q, kv = torch.randn(b, heads * 32, n) * 2, torch.randn(b, 2 * heads * 32, n) * 2
    q64, kv64 = q.double().requires_grad_(True), kv.double().requires_grad_(True)
    ref = core64(q64, kv64, heads)
    gy = torch.randn(ref.shape)
    rq, rkv = torch.autograd.grad(ref, (q64, kv64), gy.double())
    ref = ref.detach()
    dq, dkv = arena.put(q).requires_grad_(), arena.put(kv).requires_grad_()
    out = run(arena, _SoftmaxAttentionCore.apply, dq, dkv, heads)
    gq, gkv = _grads(arena, [out], [dq, dkv], [arena.put(gy)])
    assert (out.detach().cpu().double() - ref).abs().max().item() < 1e-5 * max(1.0, ref.abs().max().item())
    assert (gq.cpu().double() - rq).abs().max().item() < 2e-5 * max(1.0, rq.abs().max().item())
    assert (gkv.cpu().double() - rkv).abs().max().item() < 2e-5 * max(1.0, rkv.abs().max().item())
    with torch.no_grad():  # the inference form (no log-sum-exp output) computes the same bits
        assert torch.equal(run(arena, _SoftmaxAttentionCore.apply, dq.detach(), dkv.detach(), heads), out.detach())


# ---- optimiser (reference and tolerances: test_optim_gpu.py::test_matches_torch_over_steps at its first step) ---------

def test_clip_adamw_step(arena):
    from p2p_bridge_amd._lib import lib
    from p2p_bridge_amd.optim import ClipAdamW

    chunk = int(lib().p2pb_optim_chunk())
    shapes = [(1,), (3,), (17, 5), (chunk - 1,), (chunk,), (chunk + 1,), (7, 257), (2 * chunk + 3,)]  # chunks end unevenly
    g = torch.Generator().manual_seed(0)
    host = [torch.randn(s, generator=g) * 0.1 for s in shapes]
    grads = [torch.randn(s, generator=g) * 30.0 for s in shapes]  # far above the clipping threshold
    a = [torch.nn.Parameter(h.clone().cuda()) for h in host]
    b = [torch.nn.Parameter(arena.put(h)) for h in host]
    ref = torch.optim.AdamW(a, lr=3e-4, betas=(0.9, 0.999), weight_decay=1e-5)
    n0 = arena.n_allocations
    opt = ClipAdamW(b, lr=3e-4, betas=(0.9, 0.999), weight_decay=1e-5, max_norm=1.0, decoupled=True)
    for p, q, gr in zip(a, b, grads):
        p.grad, q.grad = gr.clone().cuda(), arena.put(gr)
    norm = torch.nn.utils.clip_grad_norm_(a, 1.0)
    ref.step()
    opt.step()
    assert arena.n_allocations > n0
    arena.check_guards()
    assert abs(opt.grad_norm() - float(norm)) <= 2e-6 * float(norm)
    for p, q in zip(a, b):
        arena.assert_written(q.grad, "clipped gradient"), arena.assert_written(q.data, "parameter")
        torch.testing.assert_close(q.grad, p.grad, rtol=1e-6, atol=0)
        for key in ("exp_avg", "exp_avg_sq"):
            x, y = opt.state[q][key], ref.state[p][key]
            arena.assert_written(x, key)
            assert (x - y).abs().max().item() <= 2e-6 * y.abs().max().item()
        torch.testing.assert_close(q, p, rtol=0, atol=2e-8)
    assert opt.steps_applied() == 1


# ---- set metrics and point-to-mesh (references: test_set_metrics_gpu.py, test_metrics_unit_sphere_gpu.py) --------------

def test_pairwise_chamfer_and_emd(arena):
    """the smallest sets of test_set_metrics_gpu.py (test_pairwise_emd_unequal_sizes: 5 x 4 clouds of 256 / 128 points) against
    the existing per-batch ops on expanded inputs: chamfer to one fp32 ulp, EMD to 2e-3 relative"""
    import numpy as np

    from p2p_bridge_amd import evaluation_metrics_fast as E, metrics
    from test_set_metrics_gpu import G, assert_one_ulp, cd_by_existing_op

    hA, hB = torch.from_numpy(G["smp"])[:5].contiguous(), torch.from_numpy(G["ref"])[:4, :128].contiguous()
    A, B = arena.put(hA), arena.put(hB)
    for X, Y in ((A, B), (B, A)):
        cd = run(arena, E.pairwise_chamfer, X, Y)
        assert_one_ulp(cd.cpu().numpy(), cd_by_existing_op(X, Y), "pairwise chamfer")
        M = run(arena, E.pairwise_emd, X, Y)
        old = torch.stack([metrics.earth_mover_distance_nograd(X[i:i + 1].expand(Y.shape[0], -1, -1).contiguous(), Y, transpose=False)
                           for i in range(X.shape[0])])
        np.testing.assert_allclose(M.cpu().numpy(), old.cpu().numpy(), rtol=2e-3, atol=0)
        small = run(arena, E.pairwise_emd, X, Y, ws_bytes=3 * (3 * X.shape[1] + 2 * Y.shape[1]) * 4)  # chunks of 3 pairs
        assert torch.equal(small, M)


@pytest.mark.parametrize("res,in_sphere", [(None, True), (12, False)])
def test_occupancy_counts(arena, res, in_sphere):
    """the JSD occupancy grid with its workspace (p2pb_occupancy_ws_bytes): the sphere-clipped grid against the fixture, the
    unclipped one against the host path (test_occupancy_counts_vs_fixture, test_occupancy_counts_unclipped_grid_vs_host_path)"""
    import numpy as np

    from p2p_bridge_amd import evaluation_metrics_fast as E
    from test_set_metrics_gpu import G

    res = int(G["resolution"]) if res is None else res
    counters, bernoulli = run(arena, E.occupancy_counts, arena.put(torch.from_numpy(G["jsd_set"])), res, in_sphere)
    if in_sphere:
        want = G["jsd_set_counters"], G["jsd_set_bernoulli"].astype(np.float64)
    else:
        want = E.occupancy_counts(G["jsd_set"], res, False)
    assert np.array_equal(counters, want[0]) and np.array_equal(bernoulli, want[1])
    assert counters.sum() > 0


@pytest.mark.parametrize("P,sub,area", [(777, 1, 0.0), (1, 1, 5e-3)])
def test_point_face_and_face_point(arena, P, sub, area):
    """the smallest mesh of test_metrics_unit_sphere_gpu.py (an icosphere subdivided once: 80 faces), bit-exact"""
    from p2p_bridge_amd import metrics as M
    from test_metrics_unit_sphere_gpu import icosphere

    verts, faces = icosphere(sub)
    g = torch.Generator().manual_seed(P)
    pts = torch.nn.functional.normalize(torch.randn(P, 3, generator=g), dim=1) * (1 + 0.05 * torch.randn(P, 1, generator=g))
    tris = verts[faces].contiguous()
    dp, dt = arena.put(pts), arena.put(tris)
    for which, fn in ((0, M.point_face_distance), (1, M.face_point_distance)):
        d_ref, i_ref = cpu_ops.point_face_dist(pts.contiguous(), tris, area, which)
        d, i = run(arena, fn, dp, dt, area)
        eq(i, i_ref, "face / point index"), eq(d, d_ref, "squared distance")
