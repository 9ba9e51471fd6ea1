"""Times the room-size Chamfer distance on the grid (metrics.chamfer_grid: PointGrid.nearest, csrc/nn_grid.hip) against the
exhaustive kernel it restates (metrics.chamfer_3DDist, csrc/chamfer.hip) and against the same Chamfer composed from the wave-
per-query search that was there before (PointGrid.knn(., 1), csrc/knn_grid.hip), on the same GPU and the same seeded rooms.
Not part of bench.py.

      room    a prediction of 300 000 points against a ground truth of 300 000 points from another seed
      scan    1 500 000 against 6 000 000 points: the shape of an ARKitScenes prediction against its laser scan

    python tools/bench_nn_grid.py [--repeats 5] [--small] [--step-timeout 420] [--brute-budget 20]
                                  [--out profiles/nn_grid_timing.txt]

Forms, per step: (a) chamfer_3DDist; (b) knn(., 1) in both directions on prebuilt grids; (c) chamfer_grid with the two grid
builds included, and on prebuilt grids; and (c) with the queries in their file order instead of the order of their own grid's
sorted rows, which shows what `order` is worth; and the two first-level p2pb_nn_grid launches of (c) alone, which shows how
much of (c) is the ring search. All four outputs of every form are compared with (a) for equal bits first.
The exhaustive kernel is timed once in that comparison; when that one call takes longer than --brute-budget seconds it is left
out of the repeats (the line "brute_in_repeats": false says so).

The parent process never touches the GPU: every step is a fresh child process under its own `timeout`, and the first step that
fails, faults or runs out of time ends the run (nothing more is started on the GPU after it). Inside a step the forms are
ALTERNATED inside every repeat; a timed call ends in a device synchronise, so the host clock around it is the time to the
finished result. Median, minimum and maximum per call. The verdict the kernel has to pass: (c) on prebuilt grids beats (b) by
more than (b)'s own spread (max - min), at both sizes. --small: 20 000 against 30 000 points, finishes in seconds (nothing is
written). Needs a GPU."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_knn_grid import alternate, emit, room, summary, verdict  # noqa: E402  (the seeded room and the timing idiom)

STEPS = {"room": (300000, 300000), "scan": (1500000, 6000000)}
SMALL = {"room": (20000, 30000)}


def step(a):
    import torch

    from p2p_bridge_amd import metrics
    from p2p_bridge_amd._lib import call, ptr, stream_ptr
    from p2p_bridge_amd.knn_grid import PointGrid
    from p2p_bridge_amd.scan_fusion import KNN_RINGS

    n, m = (SMALL if a.small else STEPS)[a.step]
    pred, gt = room(n, a.seed).cuda(), room(m, a.seed + 1).cuda()
    x1, x2 = pred[None], gt[None]
    emit({"what": "setup", "step": a.step, "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
          "prediction_points": n, "ground_truth_points": m, "k_hint": metrics.CHAMFER_GRID_K_HINT})
    sync = torch.cuda.synchronize

    def brute():
        out = metrics.chamfer_3DDist()(x1, x2)
        sync()
        return out

    def build():
        g = PointGrid(pred, metrics.CHAMFER_GRID_K_HINT), PointGrid(gt, metrics.CHAMFER_GRID_K_HINT)
        sync()
        return g

    g1, g2 = build()

    def knn1():
        (d1, i1), (d2, i2) = g2.knn(pred, 1), g1.knn(gt, 1)
        sync()
        return d1[None, :, 0], d2[None, :, 0], i1[None, :, 0].int(), i2[None, :, 0].int()

    def grid():
        out = metrics.chamfer_grid(x1, x2)
        sync()
        return out

    def grid_prebuilt():
        out = metrics.chamfer_grid(x1, x2, grid1=g1, grid2=g2)
        sync()
        return out

    ident1 = torch.arange(n, dtype=torch.int32, device="cuda")
    ident2 = torch.arange(m, dtype=torch.int32, device="cuda")

    def grid_file_order():
        (d1, i1, s1), (d2, i2, s2) = g2._nearest(pred, ident1), g1._nearest(gt, ident2)
        sync()
        return d1[None], d2[None], i1[None], i2[None]

    scratch = {q: (torch.empty(q, device="cuda"), torch.empty(q, dtype=torch.int32, device="cuda"),
                   torch.empty(q, dtype=torch.uint8, device="cuda")) for q in {n, m}}

    def rings_level0():
        # the two p2pb_nn_grid launches of (c)'s first stage alone: no later stage, no torch between them
        for g, own, query in ((g2, g1, pred), (g1, g2, gt)):
            pts, skeys, rows, cell = g.level(0)
            d, i, u = scratch[query.shape[0]]
            call("p2pb_nn_grid", query.shape[0], pts.shape[0], KNN_RINGS, ptr(own.level(0)[2]), ptr(query), ptr(pts), ptr(skeys),
                 ptr(rows), cell, ptr(d), ptr(i), ptr(u), stream_ptr())
        sync()

    def equal(got, want):
        return all(g.dtype == w.dtype and g.shape == w.shape and bool(torch.equal(g.view(torch.int32), w.view(torch.int32)))
                   for g, w in zip(got, want))

    t0 = time.perf_counter()
    want = brute()
    brute_s = time.perf_counter() - t0  # (first call: start-up cost included; only compared with the budget)
    emit({"what": "agreement, all four outputs bit for bit with chamfer_3DDist", "step": a.step,
          "knn1": equal(knn1(), want), "chamfer_grid": equal(grid(), want), "chamfer_grid_prebuilt": equal(grid_prebuilt(), want),
          "chamfer_grid_file_order": equal(grid_file_order(), want)})
    del want
    emit({"what": "stages", "step": a.step, "cell_prediction_grid": g1.cell, "cell_ground_truth_grid": g2.cell,
          "nearest_prediction_to_ground_truth": g2.nearest(pred, return_stats=True)[2],
          "nearest_ground_truth_to_prediction": g1.nearest(gt, return_stats=True)[2],
          "knn1_prediction_to_ground_truth": g2.knn(pred, 1, return_stats=True)[2],
          "knn1_ground_truth_to_prediction": g1.knn(gt, 1, return_stats=True)[2]})
    with_brute = brute_s <= a.brute_budget
    emit({"what": "first chamfer_3DDist call", "seconds": brute_s, "brute_budget_s": a.brute_budget, "brute_in_repeats": with_brute})
    fns = (("brute", brute),) if with_brute else ()
    fns += (("knn1", knn1), ("grid", grid), ("grid_build", build), ("grid_prebuilt", grid_prebuilt),
            ("grid_file_order", grid_file_order), ("rings_level0", rings_level0))
    times = alternate(fns, a.repeats)
    if with_brute:
        emit(summary("(a) chamfer_3DDist, every pair", times["brute"]))
    emit(summary("(b) PointGrid.knn(., 1) both ways, prebuilt grids", times["knn1"]))
    emit(summary("(c) chamfer_grid, both grid builds included", times["grid"]))
    emit(summary("    the two PointGrid builds alone", times["grid_build"]))
    emit(summary("(c) chamfer_grid, prebuilt grids", times["grid_prebuilt"]))
    emit(summary("    nearest both ways with the queries in file order, prebuilt grids", times["grid_file_order"]))
    emit(summary("    the two first-level p2pb_nn_grid launches of (c) alone", times["rings_level0"]))
    emit(verdict(f"verdict, {a.step}: (c) prebuilt against (b)", times, "knn1", "grid_prebuilt"))
    emit(verdict(f"what the order is worth, {a.step}", times, "grid_file_order", "grid_prebuilt"))
    if with_brute:
        emit(verdict(f"against every pair, {a.step}, builds included", times, "brute", "grid"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--small", action="store_true", help="20 000 against 30 000 points: finishes in seconds")
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds each GPU step may take")
    ap.add_argument("--brute-budget", type=float, default=20.0,
                    help="seconds one chamfer_3DDist call may take and still be repeated")
    ap.add_argument("--out", default=None, help="default: profiles/nn_grid_timing.txt (nothing is written with --small)")
    ap.add_argument("--step", choices=list(STEPS), default=None, help="run one step in this process (what the parent starts)")
    a = ap.parse_args()
    if not a.small and a.out is None:
        a.out = os.path.join(ROOT, "profiles", "nn_grid_timing.txt")
    if a.step is not None:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("bench_nn_grid needs a GPU: nothing is timed on the CPU")
        step(a)
        return
    lines = []
    for name in (SMALL if a.small else STEPS):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name,
               "--repeats", str(a.repeats), "--seed", str(a.seed), "--brute-budget", str(a.brute_budget)]
        p = subprocess.Popen(cmd + (["--small"] if a.small else []), stdout=subprocess.PIPE, text=True, cwd=ROOT)
        for ln in p.stdout:  # (passed on line by line: a long step is seen to be alive)
            sys.stdout.write(ln)
            sys.stdout.flush()
            if ln.startswith("{"):
                lines.append(ln.rstrip("\n"))
        if p.wait() != 0:  # a failure, a fault or the time limit: nothing more is started on the GPU
            raise SystemExit(f"bench_nn_grid: step {name!r} ended with status {p.returncode}; stopping")
    if a.out and not a.small:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
