"""The host half of the batched room patch builder (p2p_bridge_amd/denoise_room.py plan_patches; csrc/room_patches.hip): the
planner takes every random draw of create_patches in its order, so patch count, cuts and the generator's final state equal the
oracle loop's (oracle/cpu_ops.py room_create_patches) on the same lists and seed; and the new entry points are declared, bound
and exported. No GPU."""
import ctypes
import re

import pytest
import torch

from oracle import cpu_ops
from test_abi import HDR, header_symbols

NEW = ["p2pb_room_fps_tier_capacity", "p2pb_room_fps_jobs_ws_bytes", "p2pb_room_fps_jobs", "p2pb_room_list_bounds",
       "p2pb_room_assemble_patches"]
PATCH = 32


def lists(lengths, n=400, seed=0):
    """hand-made radius lists of the given lengths over a random cloud: idx_flat i32, offsets i64"""
    g = torch.Generator().manual_seed(seed)
    pts = torch.rand(n, 3, generator=g)
    idx = torch.cat([torch.randperm(n, generator=g)[:L] for L in lengths] + [torch.zeros(0, dtype=torch.int64)]).int()
    off = torch.zeros(len(lengths) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.tensor(lengths, dtype=torch.int64), 0)
    return pts, idx, off


CASES = {
    "short": [5, 17, PATCH - 1],
    "long": [PATCH + 1, 3 * PATCH + 5, 2 * PATCH - 1],
    "exactly_patch": [PATCH, PATCH, 2 * PATCH],
    "single_point": [1, 1, PATCH + 3, 1],
    "empty_in_the_middle": [9, 0, PATCH + 9, 0, 0, 3],
    "mixed": [1, PATCH - 1, PATCH, PATCH + 1, 0, 5 * PATCH + 7, 2],
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_takes_the_loops_draws(name):
    from p2p_bridge_amd import denoise_room as R

    pts, idx, off = lists(CASES[name], seed=len(name))
    g_ref, g_plan = torch.Generator().manual_seed(7), torch.Generator().manual_seed(7)
    ref_xyz, ref_idx, ref_cuts = cpu_ops.room_create_patches(pts, idx, off, PATCH, g_ref)
    plan = R.plan_patches(off, PATCH, g_plan)
    assert plan["centre"].numel() == ref_xyz.shape[0] == plan["kind"].numel()
    assert torch.equal(plan["cuts"], ref_cuts) and plan["cuts"].dtype == torch.int64
    assert torch.equal(g_plan.get_state(), g_ref.get_state())
    # the tables agree with each other and with the lists
    L = (off[1:] - off[:-1])[plan["centre"]]
    assert (L > 0).all() and torch.equal(plan["kind"] == 1, L >= PATCH)
    assert torch.equal(plan["job_patch"], (plan["kind"] == 1).nonzero()[:, 0])
    assert torch.equal(plan["pad_patch"], (plan["kind"] == 0).nonzero()[:, 0])
    assert ((plan["job_start"] >= 0) & (plan["job_start"] < L[plan["job_patch"]])).all()
    assert torch.equal(plan["pad_ptr"][1:] - plan["pad_ptr"][:-1], PATCH - L[plan["pad_patch"]])
    assert plan["pad_r"].numel() == int(plan["pad_ptr"][-1]) and plan["pad_normals"].shape == (plan["pad_r"].numel(), 3)
    # ... and the draws are the loop's: the duplicates it appended are the lists' entries at pad_r
    for q, p in enumerate(plan["pad_patch"].tolist()):
        c, r = int(plan["centre"][p]), plan["pad_r"][plan["pad_ptr"][q]:plan["pad_ptr"][q + 1]]
        assert torch.equal(ref_idx[p, int(L[p]):], idx[off[c]:off[c + 1]].long()[r])
    # the FPS subsets start at the drawn position
    for j, p in enumerate(plan["job_patch"].tolist()):
        c = int(plan["centre"][p])
        assert int(ref_idx[p, 0]) == int(idx[off[c] + plan["job_start"][j]])


def test_plan_of_no_centres():
    from p2p_bridge_amd import denoise_room as R

    g = torch.Generator().manual_seed(3)
    before = g.get_state()
    for off in (torch.zeros(1, dtype=torch.int64), torch.zeros(4, dtype=torch.int64)):  # s == 0; three empty lists
        plan = R.plan_patches(off, PATCH, g)
        assert all(plan[key].numel() == 0 for key in ("centre", "kind", "cuts", "job_patch", "job_start", "pad_patch", "pad_r"))
        assert plan["pad_ptr"].tolist() == [0] and plan["pad_normals"].shape == (0, 3)
    assert torch.equal(g.get_state(), before)


def test_new_entry_points_are_declared_bound_and_exported():
    from p2p_bridge_amd import _lib, build
    from p2p_bridge_amd import denoise_room as R

    build.build()
    so = ctypes.CDLL(_lib.LIB_PATH)
    syms = header_symbols()
    for s in NEW:
        assert s in syms and s in _lib.SYMBOLS and hasattr(so, s), s
    assert int(re.search(r"#define\s+P2PB_ABI_VERSION\s+(\d+)", open(HDR).read()).group(1)) == 13 == _lib.ABI_VERSION
    # the tier edges of the binding are the library's; the form behind them streams
    n = len(R.FPS_JOB_TIERS)
    assert tuple(so.p2pb_room_fps_tier_capacity(t) for t in range(n)) == R.FPS_JOB_TIERS
    assert so.p2pb_room_fps_tier_capacity(n) >= 1 << 28 and so.p2pb_room_fps_tier_capacity(n + 1) == 0
    assert R.BATCHED_MAX_LIBRARY_CALLS == n + 3
    so.p2pb_room_fps_jobs_ws_bytes.restype = ctypes.c_size_t
    assert so.p2pb_room_fps_jobs_ws_bytes(ctypes.c_longlong(20001)) >= 4 * 20001 and so.p2pb_room_fps_jobs_ws_bytes(ctypes.c_longlong(0)) == 0


def test_bad_sizes_are_refused_before_any_launch():
    """P2PB_EINVAL (-22) for sizes and pointers no launch could serve"""
    from p2p_bridge_amd import _lib

    so = _lib.lib()
    i, ll, p = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p
    buf = (ctypes.c_longlong * 64)()
    ok = p(ctypes.addressof(buf))
    fps = lambda tier, jobs, m, n, pts, ws, wsf: so.p2pb_room_fps_jobs(  # noqa: E731
        i(tier), i(jobs), i(m), i(n), pts, ok, ll(8), ok, i(1), ws, ll(wsf), ok, p(0))
    for args in [(-1, 1, 4, 8, ok, p(0), 0), (5, 1, 4, 8, ok, p(0), 0), (0, 0, 4, 8, ok, p(0), 0), (0, 1, 0, 8, ok, p(0), 0),
                 (0, 1, 4, 0, ok, p(0), 0), (0, 1, 4, 8, p(0), p(0), 0), (4, 1, 4, 8, ok, p(0), 0), (4, 1, 4, 8, ok, ok, 0)]:
        assert fps(*args) == -22, args
    assert so.p2pb_room_list_bounds(i(0), i(8), ok, ok, ll(8), ok, ok, p(0)) == -22
    assert so.p2pb_room_list_bounds(i(1), i(8), ok, ok, ll(8), p(0), ok, p(0)) == -22
    asm = lambda npatch, k, rows, picks, pad_total, pad_r: so.p2pb_room_assemble_patches(  # noqa: E731
        i(npatch), i(k), i(8), ok, ok, ll(8), ok, picks, i(rows), pad_r, ok, ll(pad_total), ok, ok, p(0))
    for args in [(0, 4, 1, ok, 0, ok), (1, 0, 1, ok, 0, ok), (1, 4, 1, p(0), 0, ok), (1, 4, 0, ok, 3, p(0)), (1, 4, -1, ok, 0, ok)]:
        assert asm(*args) == -22, args
