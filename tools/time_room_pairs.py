"""Times the room-pairs stage (p2p_bridge_amd/room_pairs.py, csrc/pairs.hip) on the GPU and writes
profiles/room_pairs_timing.txt. At the production shape s = 4096, K = 128, m = 50 000 clean points per patch, P = 8 patches:
    * patch_knn (one launch) against p2pb_knn_points called once per patch -- the only way to get these lists without it --
      after checking that the two give the same bits;
    * unique_assign against the numpy restatement of the sequential rule (tests/pairs_ref.py), same result checked;
    * finish;
and one synthetic scene of 10^6 noisy and 5 * 10^6 clean points end to end (create_spherical_batches, npoints 4096, r 0.3).
Device work is timed per call over windows of about 0.25 s of back-to-back calls between device events, after a warm-up; median
(min) of 7 windows, the windows of the two k-NN paths alternating. Host work and the scene are timed with a wall clock.

    python tools/time_room_pairs.py [--out profiles/room_pairs_timing.txt] [--small]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pairs_ref  # noqa: E402
from p2p_bridge_amd import denoise  # noqa: E402
from p2p_bridge_amd import room_pairs as RP  # noqa: E402


WINDOW_S, REPEATS = 0.25, 7


def timed(*fns):
    """per-call time of each fn: after a warm-up, each is given as many calls as fill a window of about WINDOW_S between device
    events, and the windows of the fns ALTERNATE, REPEATS of each -> [(median ms, min ms, calls per window)]"""
    iters = []
    for fn in fns:
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        iters.append(max(1, int(WINDOW_S / max(time.perf_counter() - t0, 1e-6))))
    out = [[] for _ in fns]
    for _ in range(REPEATS):
        for j, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters[j]):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[j].append(a.elapsed_time(b) / iters[j])
    return [(statistics.median(o), min(o), n) for o, n in zip(out, iters)]


def box_scene(n_noisy, seed=0):
    """a 4 x 3 x 2.5 m room: the box mesh, a jittered scan of it and colours"""
    x, y, z = 4.0, 3.0, 2.5
    verts = np.array([[0, 0, 0], [x, 0, 0], [x, y, 0], [0, y, 0], [0, 0, z], [x, 0, z], [x, y, z], [0, y, z]], dtype=np.float32)
    quads = [(0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 5, 4), (1, 2, 6, 5), (2, 3, 7, 6), (3, 0, 4, 7)]
    faces = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], dtype=np.int32)
    g = torch.Generator().manual_seed(seed)
    dv, df = torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda()
    vcol = torch.rand(8, 3, generator=g).cuda()
    _, noisy, rgb_noisy = RP.sample_mesh(dv, df, torch.rand(n_noisy, 3, dtype=torch.float64, generator=g).cuda(), vcol)
    noisy = (noisy + 0.01 * torch.randn(n_noisy, 3, generator=g).cuda()).contiguous()
    _, clean, rgb_clean = RP.sample_mesh(dv, df, torch.rand(5 * n_noisy, 3, dtype=torch.float64, generator=g).cuda(), vcol)
    return clean, noisy, rgb_clean, rgb_noisy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "room_pairs_timing.txt"))
    ap.add_argument("--small", action="store_true", help="a rehearsal at toy sizes (overheads, not a measurement)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_room_pairs: no GPU visible; nothing is measured without one")
    p, s, k, m, scene_n = (2, 256, 128, 2000, 20000) if a.small else (8, 4096, 128, 50000, 1000000)
    rng = np.random.default_rng(0)
    ref = rng.uniform(0, 1, (p * m, 3)).astype(np.float32)
    ref[:, 2] *= 0.05
    query = (ref.reshape(p, m, 3)[:, rng.integers(0, m, s)] + rng.normal(0, 0.005, (p, s, 3))).astype(np.float32)
    dq, dr = torch.from_numpy(query).cuda(), torch.from_numpy(ref).cuda()
    off = torch.arange(p + 1, dtype=torch.int64).cuda() * m
    rows, lines = [], []

    def row(what, ms, ms_min, calls=1, **extra):
        rows.append(dict(what=what, ms_median=ms, ms_min=ms_min, calls_per_window=calls, **extra))
        lines.append(f"{what} [{calls} calls per window]: {ms:.3f} ms ({ms_min:.3f})")
        print(lines[-1], flush=True)

    # k-NN: the same bits first, then the times
    idx, d2 = RP.patch_knn(dq, dr, off, k)
    per_patch = lambda: [denoise.knn_points(dq[j][None], dr[j * m:(j + 1) * m][None], K=k) for j in range(p)]  # noqa: E731
    old = per_patch()
    assert all(torch.equal(idx[j].long(), old[j].idx[0]) and torch.equal(d2[j], old[j].dists[0]) for j in range(p))
    del old
    shape = f"P {p}, s {s}, K {k}, m {m}"
    (ms, lo, n), (ms2, lo2, n2) = timed(lambda: RP.patch_knn(dq, dr, off, k), per_patch)  # (alternating windows)
    row(f"patch_knn, one launch ({shape})", ms, lo, n, pairs_per_s=p * s * m / (ms * 1e-3))
    row(f"p2pb_knn_points, one call per patch ({shape})", ms2, lo2, n2, pairs_per_s=p * s * m / (ms2 * 1e-3))
    # assignment
    assign, unique = RP.unique_assign(idx, off, total=p * m)
    t0 = time.perf_counter()
    want = np.stack([pairs_ref.sequential_assign(x) for x in idx.cpu().numpy()])
    host_ms = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(assign.cpu().numpy(), want)
    (ms, lo, n), = timed(lambda: RP.unique_assign(idx, off, total=p * m))
    row(f"unique_assign ({shape}; {float((assign == idx[:, :, 0]).float().mean()):.4f} of the points keep their first choice, "
        f"unique fraction {float(unique.float().mean()) / s:.4f})", ms, lo, n)
    row("sequential rule in numpy / Python, same lists, one run (same result)", host_ms, host_ms)
    # the same with contention: s noisy points on 1.5 s clean ones, so that many first choices collide
    mc = s + s // 2
    off_c = torch.arange(p + 1, dtype=torch.int64).cuda() * mc
    ref_c = dr.reshape(p, m, 3)[:, :mc].reshape(-1, 3).contiguous()
    idx_c, _ = RP.patch_knn(dq, ref_c, off_c, k, return_dist=False)
    assign_c, unique_c = RP.unique_assign(idx_c, off_c, total=p * mc)
    t0 = time.perf_counter()
    want = np.stack([pairs_ref.sequential_assign(x) for x in idx_c.cpu().numpy()])
    host_ms = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(assign_c.cpu().numpy(), want)
    (ms, lo, n), = timed(lambda: RP.unique_assign(idx_c, off_c, total=p * mc))
    row(f"unique_assign, contended (P {p}, s {s}, K {k}, m {mc}; {float((assign_c == idx_c[:, :, 0]).float().mean()):.4f} of the "
        f"points keep their first choice, unique fraction {float(unique_c.float().mean()) / s:.4f})", ms, lo, n)
    row("sequential rule in numpy / Python, the contended lists, one run (same result)", host_ms, host_ms)
    rgb_q, rgb_r = torch.rand(p, s, 3).cuda(), torch.rand(p * m, 3).cuda()
    (ms, lo, n), = timed(lambda: RP.finish(dq, rgb_q, dr, rgb_r, off, assign))
    row(f"finish ({shape})", ms, lo, n)
    # one scene end to end (host clock around work that ends in device-to-host copies)
    clean, noisy, rgb_clean, rgb_noisy = box_scene(scene_n)
    args = {"npoints": 4096 if not a.small else 256, "r": 0.3}
    walls, kept = [], 0
    for rep in range(1 + (1 if a.small else 3)):
        np.random.seed(42)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        data, stats = RP.create_spherical_batches(clean, noisy, rgb_clean, rgb_noisy, None, args)
        torch.cuda.synchronize()
        if rep:
            walls.append((time.perf_counter() - t0) * 1e3)
        kept = len(data)
    row(f"create_spherical_batches, {noisy.shape[0]} noisy + {clean.shape[0]} clean points, npoints {args['npoints']}, r 0.3: "
        f"{kept} patches kept, {stats[0]} skipped, unique fraction {stats[1]:.4f}, wall clock after one warm-up run",
        statistics.median(walls), min(walls))
    head = [f"box: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, HIP {torch.version.hip}",
            f"per call, median (min) over {REPEATS} windows of about {WINDOW_S} s between device events after a warm-up (the two "
            "k-NN paths in alternating windows); host work and the scene: wall clock"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(head + lines) + "\n" + json.dumps({"small": a.small, "rows": rows}) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
