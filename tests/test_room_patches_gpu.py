"""The batched room patch builder (p2p_bridge_amd/denoise_room.py fps_jobs / create_patches_batched, csrc/room_patches.hip)
against the oracle loop (oracle/cpu_ops.py room_create_patches and its FPS restatement: swap, sample, map back) and against the
loop builder on the GPU: the same bits, in a bounded number of launches, inside the buffers it was given."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import cpu_ops, net_ref
from test_memory_discipline_gpu import arena, eq, run  # noqa: F401  (arena: the PoisonArena fixture)
from test_room_gpu import _Stand, _Stub, room

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    from p2p_bridge_amd import denoise_room

    return denoise_room


def oracle_job(pts, lst, start, m):
    """cpu_ops.room_create_patches' FPS subset (oracle/cpu_ops.py:384-387) -> positions within the list"""
    q = pts[lst.long()].clone()
    q[[0, start]] = q[[start, 0]]
    f = cpu_ops.furthest_point_sampling_forward(q.t().contiguous()[None], m)[0].long()
    return torch.where(f == 0, torch.full_like(f, start), torch.where(f == start, torch.zeros_like(f), f))


def starts_of(L, seed):
    """the boundary starts: both ends, the key order's period (512) and its neighbours, one random"""
    rnd = int(torch.randint(0, L, (1,), generator=torch.Generator().manual_seed(seed)))
    return sorted({s for s in (0, L - 1, 511, 512, 513, rnd) if 0 <= s < L})


def make_jobs(n, lengths, seed):
    """hand-made lists (random order, not ascending) of the given lengths, every boundary start of each -> idx_flat i32,
    offsets i64, and the job tables"""
    g = torch.Generator().manual_seed(seed)
    idx = torch.cat([torch.randperm(n, generator=g)[:L] for L in lengths]).int()
    off = torch.zeros(len(lengths) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.tensor(lengths), 0)
    jo, jl, js = [], [], []
    for c, L in enumerate(lengths):
        for s in starts_of(L, seed + c):
            jo.append(int(off[c])), jl.append(L), js.append(s)
    return idx, off, jo, jl, js


def check_jobs(R, pts, idx, jo, jl, js, m):
    got = R.fps_jobs(pts.cuda(), idx.cuda(), jo, jl, js, m).cpu()
    assert got.shape == (len(jo), m) and got.dtype == torch.int32
    for j, (o, L, s) in enumerate(zip(jo, jl, js)):
        ref = oracle_job(pts, idx[o:o + L], s, m)
        assert torch.equal(got[j].long(), ref), f"job {j}: list of {L}, start {s}, m {m}: {(got[j].long() != ref).sum().item()} picks differ"
    return got


@pytest.mark.parametrize("m", [64, 256, 1024])
def test_fps_jobs_match_the_oracle_on_every_tier(R, m):
    """one call mixes all tiers (per-tier launches and output rows together); lengths on and behind every tier edge"""
    edges = list(R.FPS_JOB_TIERS)
    assert edges[-1] == 16384
    lengths = [m, m + 1, 2 * m - 1] + [L for e in edges for L in (e, e + 1)] + ([20011] if m == 256 else [])
    lengths = [L for L in dict.fromkeys(lengths) if L >= m]
    pts = room(21000, seed=m)
    idx, off, jo, jl, js = make_jobs(pts.shape[0], lengths, seed=m)
    assert not bool((idx[1:off[1]] > idx[:off[1] - 1]).all())  # (not in ascending room order)
    order = torch.randperm(len(jo), generator=torch.Generator().manual_seed(1)).tolist()  # tiers interleaved in the call
    jo, jl, js = [jo[i] for i in order], [jl[i] for i in order], [js[i] for i in order]
    check_jobs(R, pts, idx, jo, jl, js, m)


def test_fps_jobs_refuses_a_table_that_leaves_the_lists(R):
    pts, idx = room(100, seed=1).cuda(), torch.arange(50, dtype=torch.int32).cuda()
    for jo, jl, js in [([0], [51], [0]), ([40], [11], [0]), ([0], [10], [10]), ([0], [0], [0]), ([-1], [5], [0]), ([0], [5], [-1])]:
        with pytest.raises(ValueError):
            R.fps_jobs(pts, idx, jo, jl, js, 4)
    assert R.fps_jobs(pts, idx, [], [], [], 4).shape == (0, 4)


def tie_clouds():
    g = torch.Generator().manual_seed(5)
    a = torch.rand(700, 3, generator=g)
    lat = torch.stack(torch.meshgrid(*[torch.arange(17.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    plane = torch.stack(torch.meshgrid(torch.arange(60.0), torch.arange(50.0), indexing="ij"), -1).reshape(-1, 2)
    return {"every point three times": a.repeat(3, 1), "lattice 17^3": lat, "all identical": torch.full((1500, 3), 0.25),
            "coplanar": torch.cat([plane * 0.5, torch.full((3000, 1), 1.0)], 1)}


@pytest.mark.parametrize("name", sorted(tie_clouds()))
def test_fps_jobs_tie_geometry(R, name):
    """equal distances everywhere: the virtual swap has to land exactly on the key order at every boundary start"""
    pts = tie_clouds()[name].contiguous()
    n = pts.shape[0]
    idx, off, jo, jl, js = make_jobs(n, [n, n - 1, 600], seed=n)
    check_jobs(R, pts, idx, jo, jl, js, 256)


def room_lists(n, seed, centres, radius):
    pts = room(n, seed=seed)
    cidx = cpu_ops.furthest_point_sampling_forward(pts.t().contiguous()[None], centres)[0].long()
    idx_flat, offsets = cpu_ops.radius_query(pts[cidx].contiguous(), pts, radius)
    return pts, idx_flat, offsets


_ROOM = {}


def room_case():
    """room(30000, seed 3), 24 centres, r = 0.5, patches of 256, generator seed 7 (tests/test_room_gpu.py) and its oracle patches"""
    if not _ROOM:
        pts, idx_flat, offsets = room_lists(30000, 3, 24, 0.5)
        g = torch.Generator().manual_seed(7)
        ref = cpu_ops.room_create_patches(pts, idx_flat, offsets, 256, g)
        _ROOM.update(pts=pts, idx_flat=idx_flat, offsets=offsets, ref=ref, state=g.get_state())
    return _ROOM


def test_batched_patches_match_the_oracle_on_a_room(R):
    c = room_case()
    ref_xyz, ref_idx, ref_cuts = c["ref"]
    assert (ref_cuts < 256).any() and (ref_cuts == 256).any()  # both branches occur
    g = torch.Generator().manual_seed(7)
    got = R.create_patches_batched(c["pts"].cuda(), c["idx_flat"].cuda(), c["offsets"].cuda(), 256, g)
    eq(got["cuts"], ref_cuts, "cuts"), eq(got["idx"], ref_idx, "idx"), eq(got["xyz"], ref_xyz, "xyz")
    assert torch.equal(g.get_state(), c["state"])
    assert got["rgb"] is None and got["feats"] is None


def test_batched_patches_match_the_oracle_on_hand_made_lists(R):
    """L in {1, 2, patch - 1, patch, patch + 1}; L == 1 has level 0, so its duplicates are exact copies"""
    patch = 64
    pts = room(500, seed=2)
    g0 = torch.Generator().manual_seed(4)
    lengths = [1, 2, patch - 1, patch, patch + 1, 1, 3 * patch]
    idx = torch.cat([torch.randperm(500, generator=g0)[:L] for L in lengths]).int()
    off = torch.zeros(len(lengths) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.tensor(lengths), 0)
    g_ref, g = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    ref_xyz, ref_idx, ref_cuts = cpu_ops.room_create_patches(pts, idx, off, patch, g_ref)
    got = R.create_patches_batched(pts.cuda(), idx.cuda(), off.cuda(), patch, g)
    eq(got["cuts"], ref_cuts, "cuts"), eq(got["idx"], ref_idx, "idx"), eq(got["xyz"], ref_xyz, "xyz")
    assert torch.equal(g.get_state(), g_ref.get_state())
    one = got["xyz"][0].cpu()
    assert ref_cuts[0] == 1 and torch.equal(one, one[:1].expand(patch, 3))


def test_batched_patches_equal_the_loop_with_colours_and_features(R):
    c = room_case()
    n = c["pts"].shape[0]
    g0 = torch.Generator().manual_seed(1)
    colors, feats = torch.rand(n, 3, generator=g0).cuda(), torch.randn(n, 5, generator=g0).cuda()
    args = (c["pts"].cuda(), c["idx_flat"].cuda(), c["offsets"].cuda(), 256)
    g_loop, g = torch.Generator().manual_seed(7), torch.Generator().manual_seed(7)
    loop = R.create_patches(*args, g_loop, colors, feats)
    got = R.create_patches_batched(*args, g, colors, feats, gather=True)
    assert sorted(got) == sorted(loop)
    for key in ("xyz", "idx", "cuts", "rgb", "feats"):
        eq(got[key], loop[key], key)
    assert got["feats"].shape == (loop["xyz"].shape[0], 256, 5)
    assert torch.equal(g.get_state(), g_loop.get_state())
    lazy = R.create_patches_batched(*args, torch.Generator().manual_seed(7), colors, feats, gather=False)
    assert lazy["rgb"] is None and lazy["feats"] is None
    eq(lazy["xyz"], loop["xyz"], "xyz, gather=False"), eq(lazy["idx"], loop["idx"], "idx, gather=False")


def test_two_runs_give_the_same_bits(R):
    c = room_case()
    args = (c["pts"].cuda(), c["idx_flat"].cuda(), c["offsets"].cuda(), 256)
    a = R.create_patches_batched(*args, torch.Generator().manual_seed(7))
    b = R.create_patches_batched(*args, torch.Generator().manual_seed(7))
    eq(a["xyz"], b["xyz"], "xyz"), eq(a["idx"], b["idx"], "idx"), eq(a["cuts"], b["cuts"], "cuts")
    pts = room(17000, seed=6)
    idx, off, jo, jl, js = make_jobs(17000, [300, 1500, 16391], seed=3)
    p1 = R.fps_jobs(pts.cuda(), idx.cuda(), jo, jl, js, 64)
    p2 = R.fps_jobs(pts.cuda(), idx.cuda(), jo, jl, js, 64)
    eq(p1, p2, "picks")


@pytest.mark.parametrize("lengths,m", [([77, 1025, 4099, 9001], 33), ([16391, 301, 16385], 9)])
def test_fps_jobs_inside_a_poisoned_arena(R, arena, lengths, m):
    """mixed register tiers; the streaming tier with its workspace (every streamed job owns 4 L floats of it, L odd): guards intact, picks equal the oracle's (a pick never written reads -1)"""
    pts = room(17001, seed=m)
    idx, off, jo, jl, js = make_jobs(pts.shape[0], lengths, seed=m)
    dp, di = arena.put(pts), arena.put(idx)
    n0 = arena.n_allocations
    got = run(arena, R.fps_jobs, dp, di, jo, jl, js, m)
    made = [(r["dtype"], r["shape"]) for r in arena.records[n0:]]
    assert (torch.int32, (len(jo), m)) in made
    streamed = sum(L for L in jl if L > R.FPS_JOB_TIERS[-1])
    ws_floats = int(R.lib().p2pb_room_fps_jobs_ws_bytes(streamed)) // 4
    assert ws_floats >= 4 * streamed and ((torch.float32, (ws_floats,)) in made) == (streamed > 0)
    for j, (o, L, s) in enumerate(zip(jo, jl, js)):
        eq(got[j].long(), oracle_job(pts, idx[o:o + L], s, m), f"job {j} (list of {L}, start {s})")


def test_batched_patches_inside_a_poisoned_arena(R, arena):
    """both kinds of patch, three tiers, odd patch size: every output element written, nothing outside the outputs"""
    patch = 131
    pts = room(3001, seed=12)
    g0 = torch.Generator().manual_seed(5)
    lengths = [1, 57, patch - 1, patch, 1027, 0, 4101]
    idx = torch.cat([torch.randperm(3001, generator=g0)[:L] for L in lengths[:-1]] + [torch.randint(0, 3001, (4101,), generator=g0)]).int()
    off = torch.zeros(len(lengths) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.tensor(lengths), 0)
    g_ref, g = torch.Generator().manual_seed(2), torch.Generator().manual_seed(2)
    ref_xyz, ref_idx, ref_cuts = cpu_ops.room_create_patches(pts, idx, off, patch, g_ref)
    dp, di, do = arena.put(pts), arena.put(idx), arena.put(off)
    n0 = arena.n_allocations
    got = R.create_patches_batched(dp, di, do, patch, g)
    assert arena.n_allocations >= n0 + 3  # picks, bounds, xyz, idx
    arena.check_guards()
    arena.assert_written(got["xyz"], "xyz")
    eq(got["xyz"], ref_xyz, "xyz"), eq(got["idx"], ref_idx, "idx"), eq(got["cuts"], ref_cuts, "cuts")
    assert torch.equal(g.get_state(), g_ref.get_state())


@pytest.mark.parametrize("centres", [6, 48])
def test_library_calls_are_bounded(R, monkeypatch, centres):
    pts, idx_flat, offsets = room_lists(20000, 4, centres, 0.45)
    calls = []
    real = R.call

    def counting(name, *a):
        calls.append(name)
        return real(name, *a)

    monkeypatch.setattr(R, "call", counting)
    got = R.create_patches_batched(pts.cuda(), idx_flat.cuda(), offsets.cuda(), 128, torch.Generator().manual_seed(1))
    assert got["xyz"].shape[0] >= centres
    assert 1 <= len(calls) <= R.BATCHED_MAX_LIBRARY_CALLS, calls
    assert calls.count("p2pb_room_assemble_patches") == 1 and "p2pb_furthest_point_sampling" not in calls
    print(f"\n{centres} centres, {got['xyz'].shape[0]} patches: {len(calls)} library calls {calls}")


_PIPE = {}


def pipe_case(R):
    """room(12000, seed 5), patches of 128, k = 1, r = 0.5 (94 centres, lists of 17 .. 372 points: both kinds of patch), stub sampler:
    loop mode's trace and output, the oracle's output"""
    if not _PIPE:
        pts = room(12000, seed=5)
        kw = dict(k=1, radius=0.5, batch_size=7, steps=3)
        out = R.denoise_room(_Stub(), pts.cuda(), 128, generator=torch.Generator().manual_seed(11), trace=(tr := {}), **kw)
        ref, num, _ = cpu_ops.denoise_room(lambda x: 0.9 * x, pts, 128, 1, 0.5, torch.Generator().manual_seed(11))
        _PIPE.update(pts=pts, kw=kw, out=out, trace=tr, ref=ref, num=num)
    return _PIPE


def test_denoise_room_batched_with_stub_sampler(R):
    c = pipe_case(R)
    out = R.denoise_room(_Stub(), c["pts"].cuda(), 128, generator=torch.Generator().manual_seed(11), trace=(tr := {}),
                         batched_patches=True, **c["kw"])
    assert sorted(tr) == sorted(c["trace"]) and sorted(tr["patches"]) == sorted(c["trace"]["patches"])
    for key in ("xyz", "idx", "cuts"):
        eq(tr["patches"][key], c["trace"]["patches"][key], f"patches[{key}]")
    cuts = tr["patches"]["cuts"]
    assert (cuts < 128).any() and (cuts == 128).any()
    assert torch.equal(tr["counts"].cpu().long(), c["num"].long())
    assert (out.cpu() - c["ref"]).abs().max().item() < 1e-5
    out2 = R.denoise_room(_Stub(), c["pts"].cuda(), 128, generator=torch.Generator().manual_seed(11),
                          average_predictions=False, batched_patches=True, **c["kw"])
    assert out2.shape == c["pts"].shape and torch.isfinite(out2).all()


def test_denoise_room_batched_feeds_the_same_conditioning(R):
    """colours reach the sampler through the per-batch gather: the output equals loop mode's to the merge tolerance
    (tests/test_room_gpu.py: 1e-6), and differs from the run without colours"""
    c = pipe_case(R)
    colors = torch.rand(c["pts"].shape[0], 3, generator=torch.Generator().manual_seed(3)).cuda()
    kw = dict(k=1, radius=0.5, batch_size=7, steps=3, colors=colors, use_rgb_features=True)
    loop = R.denoise_room(_Stand(), c["pts"].cuda(), 128, generator=torch.Generator().manual_seed(11), **kw)
    got = R.denoise_room(_Stand(), c["pts"].cuda(), 128, generator=torch.Generator().manual_seed(11), batched_patches=True, **kw)
    assert (got - loop).abs().max().item() < 1e-6
    kw.update(colors=None)
    plain = R.denoise_room(_Stand(), c["pts"].cuda(), 128, generator=torch.Generator().manual_seed(11), batched_patches=True, **kw)
    assert (got - plain).abs().max().item() > 1e-4


def test_denoise_room_batched_with_real_sampler(R):
    """the tiny golden network, 2 bridge steps, graph replay, on room(12000, seed 8): the tolerance of loop mode's test"""
    from p2p_bridge_amd import p2pb as product

    cfg = json.load(open(os.path.join(GOLDEN, "tiny_cfg.json")))
    w = np.load(os.path.join(GOLDEN, "tiny_weights.npz"))
    sd = {k: torch.from_numpy(w[k]).float() for k in w.files}
    model = product.build_model(cfg, sd, device="cuda")
    orc = net_ref.RefNet(cfg, sd, vox_mode="tree")
    pts = room(12000, seed=8)
    out = R.denoise_room(model, pts.cuda(), 1024, k=2, radius=0.5, batch_size=16, steps=2,
                         generator=torch.Generator().manual_seed(2), graph=True, batched_patches=True)
    ref, _, _ = cpu_ops.denoise_room(lambda x: net_ref.sample(orc, cfg, x, steps=2, log_count=2)["x_pred"], pts, 1024, 2,
                                     0.5, torch.Generator().manual_seed(2))
    err = (out.cpu() - ref).abs().max().item()
    print(f"\nroom pipeline, batched patches, real sampler: max|hip - oracle| = {err:.3e}")
    assert err < 1e-4
