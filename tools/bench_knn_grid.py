"""Times the grid k-NN (p2p_bridge_amd/knn_grid.py, csrc/knn_grid.hip) against the exhaustive search it restates (csrc/knn.hip)
on the same GPU and the same seeded room. Not part of bench.py.

      knn     k = 10 for 100 000 queries drawn from a 300 000-point room: denoise.knn_points(method="brute") against
              method="grid" (grid build included), and PointGrid's build and search on their own with the per-stage stats.
              The brute force needs 4 n bytes of scratch per query (120 GB in one call here): its queries are taken in
              chunks of 1 GiB of scratch, as the fill stage takes them
      fill    image_features.interpolate_missing_features end to end, neighbours="brute" against "grid", 30 % of the room
              unobserved (scattered points and one occluded corner)

    python tools/bench_knn_grid.py [--points 300000] [--queries 100000] [--k 10] [--channels 64] [--repeats 3] [--small]
                                   [--step-timeout 420] [--out profiles/knn_grid_timing.txt]

The parent process never touches the GPU: every step is a fresh child process under its own `timeout`, and the first step that
fails, faults or runs out of time ends the run (nothing more is started on the GPU after it). Inside a step both methods are
warmed up once, compared for equal bits once, and then ALTERNATED inside every repeat; a timed call ends in a device
synchronise, so the host clock around it is the time to the finished result. Median, minimum and maximum per call; the brute
force's own spread (max - min) is the yardstick a gain has to exceed. The room is seeded and synthetic: a floor, two walls
and clutter in 4 x 3 x 2.5 m. --small: a 20 000-point room that finishes in seconds (nothing is written). Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = ("knn", "fill")
BRUTE_WS_BYTES = 1 << 30  # scratch of one brute-force call (4 n bytes per query), the fill stage's KNN_WS_BYTES


def room(n, seed=0):
    """a synthetic room: floor + two walls + clutter, metres"""
    import torch

    g = torch.Generator().manual_seed(seed)
    u = torch.rand(n, 3, generator=g)
    which = torch.randint(0, 4, (n,), generator=g)
    p = torch.stack([u[:, 0] * 4.0, u[:, 1] * 3.0, u[:, 2] * 2.5], 1)
    p[which == 0, 2] = 0.0
    p[which == 1, 0] = 0.0
    p[which == 2, 1] = 3.0
    return (p + 0.005 * torch.randn(n, 3, generator=g)).contiguous()


def emit(d):
    print(json.dumps(d), flush=True)


def alternate(fns, repeats):
    """{name: [ms per call]} of the callables, alternated inside every repeat; each ends in a device synchronise itself"""
    times = {name: [] for name, _ in fns}
    for _ in range(repeats):
        for name, fn in fns:
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    return times


def summary(what, ms):
    return {"what": what, "repeats": len(ms), "ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms),
            "ms_spread": max(ms) - min(ms)}


def verdict(what, times, old, new):
    gain = statistics.median(times[old]) - statistics.median(times[new])
    spread = max(times[old]) - min(times[old])
    return {"what": what, f"{old}_over_{new}_at_median": statistics.median(times[old]) / statistics.median(times[new]),
            "ms_saved_at_median": gain, f"{old}_ms_spread": spread, "gain_exceeds_spread": gain > spread}


def step_knn(a):
    import torch

    from p2p_bridge_amd import denoise
    from p2p_bridge_amd.knn_grid import PointGrid

    pts = room(a.points, a.seed).cuda()
    pick = torch.randperm(a.points, generator=torch.Generator().manual_seed(a.seed + 1))[:a.queries]
    query = pts[pick.cuda()].contiguous()
    emit({"what": "setup", "step": "knn", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
          "points": a.points, "queries": a.queries, "k": a.k})

    chunk = max(1, BRUTE_WS_BYTES // (4 * a.points))

    def brute():
        parts = [denoise.knn_points(query[None, q0:q0 + chunk], pts[None], K=a.k, method="brute")
                 for q0 in range(0, a.queries, chunk)]
        out = torch.cat([p.dists for p in parts], 1), torch.cat([p.idx for p in parts], 1)
        torch.cuda.synchronize()
        return out

    def grid():
        out = denoise.knn_points(query[None], pts[None], K=a.k, method="grid")
        torch.cuda.synchronize()
        return out.dists, out.idx

    def build():
        g = PointGrid(pts, a.k)
        torch.cuda.synchronize()
        return g

    built = build()

    def search():
        out = built.knn(query, a.k, return_stats=True)
        torch.cuda.synchronize()
        return out

    want, got = brute(), grid()  # warm-up of both, and the agreement
    stats = search()[2]
    emit({"what": "agreement", "step": "knn", "idx_equal": bool(torch.equal(want[1], got[1])),
          "dist2_bits_equal": bool(torch.equal(want[0].view(torch.int32), got[0].view(torch.int32)))})
    emit({"what": "grid", "cell": built.cell, "stats": stats})
    del want, got
    times = alternate((("brute", brute), ("grid", grid), ("grid_build", build), ("grid_search", search)), a.repeats)
    emit(summary(f'knn_points(method="brute"), {chunk} queries per call', times["brute"]))
    emit(summary('knn_points(method="grid"), grid build included', times["grid"]))
    emit(summary("PointGrid(ref, k): the build alone", times["grid_build"]))
    emit(summary("PointGrid.knn on a built grid", times["grid_search"]))
    emit(verdict("verdict, k-NN", times, "brute", "grid"))


def step_fill(a):
    import torch

    from p2p_bridge_amd import image_features as IF

    pts = room(a.points, a.seed).cuda()
    g = torch.Generator().manual_seed(a.seed + 2)
    corner = (pts[:, 0] > 3.0) & (pts[:, 1] < 0.8)  # one occluded corner: whole neighbourhoods are unobserved (several rounds)
    scattered = (torch.rand(a.points, generator=g) < 0.3 - float(corner.float().mean())).cuda()
    seen = ~(corner | scattered)
    count = seen.to(torch.int32)
    feats = (torch.rand(a.points, a.channels, generator=g).cuda() * 0.9 + 0.1) * seen[:, None]
    feats = feats.to(torch.float16).contiguous()
    emit({"what": "setup", "step": "fill", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
          "points": a.points, "channels": a.channels, "k": a.k, "unobserved": int((~seen).sum()),
          "unobserved_in_the_corner": int(corner.sum())})
    rounds = {}

    def fill(neighbours):
        def fn():
            out, rounds[neighbours] = IF.interpolate_missing_features(feats.clone(), count, pts, k=a.k, return_rounds=True,
                                                                      neighbours=neighbours)
            torch.cuda.synchronize()
            return out
        return fn

    brute, grid = fill("brute"), fill("grid")
    want, got = brute(), grid()  # warm-up of both, and the agreement
    emit({"what": "agreement", "step": "fill", "feats_bits_equal": bool(torch.equal(want.view(torch.int16), got.view(torch.int16))),
          "rounds_brute": rounds["brute"], "rounds_grid": rounds["grid"]})
    del want, got
    times = alternate((("brute", brute), ("grid", grid)), a.repeats)
    emit(summary('interpolate_missing_features(neighbours="brute")', times["brute"]))
    emit(summary('interpolate_missing_features(neighbours="grid")', times["grid"]))
    emit(verdict("verdict, fill stage end to end", times, "brute", "grid"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=300000)
    ap.add_argument("--queries", type=int, default=100000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--small", action="store_true", help="20 000 points, 5 000 queries: finishes in seconds")
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds each GPU step may take")
    ap.add_argument("--out", default=None, help="default: profiles/knn_grid_timing.txt (nothing is written with --small)")
    ap.add_argument("--step", choices=STEPS, default=None, help="run one step in this process (what the parent starts)")
    a = ap.parse_args()
    if a.small:
        a.points, a.queries = 20000, 5000
    elif a.out is None:
        a.out = os.path.join(ROOT, "profiles", "knn_grid_timing.txt")
    if a.step is not None:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("bench_knn_grid needs a GPU: nothing is timed on the CPU")
        {"knn": step_knn, "fill": step_fill}[a.step](a)
        return
    lines = []
    for step in STEPS:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step,
               "--points", str(a.points), "--queries", str(a.queries), "--k", str(a.k), "--channels", str(a.channels),
               "--repeats", str(a.repeats), "--seed", str(a.seed)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, cwd=ROOT)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0:  # a failure, a fault or the time limit: nothing more is started on the GPU
            raise SystemExit(f"bench_knn_grid: step {step!r} ended with status {r.returncode}; stopping")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
