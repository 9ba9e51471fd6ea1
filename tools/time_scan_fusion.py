"""Times the final stages of scan fusion (p2p_bridge_amd/scan_fusion.py, csrc/scan.hip) at the size of a fused room: the synthetic
room of tests/scan_ref.py with 2 * 10^6 points in an 8 x 6 x 3 m box,
  voxel_down_sample at 0.01        the whole-room down-sampling
  outlier_removal, std_thresh=2    the k = 20 self-query of every point (grid search) and the statistical band
  filter_iphone_scan               the 1-NN query against a second cloud of half the size (the laser scan's stand-in)
against two baselines on the same machine:
  scipy.spatial.cKDTree, workers=16   build + query, the CPU stand-in for cuML (the reference's own libraries cannot run here);
  denoise.knn_points                  the package's brute-force search, at 2 * 10^5 points only (it is O(n^2): past
                                      --brute-budget seconds the rest is extrapolated from the chunks that ran, and said so).
The masks of the grid path are compared with the cKDTree ones under the margin rule of tests/scan_ref.py before anything is
quoted. Not part of bench.py.

    python tools/time_scan_fusion.py [--points 2000000] [--brute-points 200000] [--repeats 5] [--brute-budget 60] [--out FILE]

One process, seeded inputs, every GPU stage warmed up before it is timed; a stage's time is the host clock around the call with
a device synchronise on both sides (the calls synchronise themselves: they read counts back), median and minimum over the
repeats. The cKDTree stages run `--cpu-repeats` times. Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scan_ref  # noqa: E402
from p2p_bridge_amd import denoise  # noqa: E402
from p2p_bridge_amd import scan_fusion as SF  # noqa: E402

EXT = (8.0, 6.0, 3.0)


def gpu_ms(fn, repeats):
    fn()  # warm-up: code objects, allocator
    out, t = None, []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return out, {"ms_median": statistics.median(t), "ms_min": min(t), "repeats": repeats}


def cpu_ms(fn, repeats):
    out, t = None, []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return out, {"ms_median": statistics.median(t), "ms_min": min(t), "repeats": repeats}


def brute_kth(pts, k, budget):
    """k-th distance of every point through knn_points, the queries in chunks of 1 GiB of scratch -> (seconds, extrapolated?)"""
    n = pts.shape[0]
    cloud = pts.reshape(1, n, 3)
    step = max(1, (1 << 30) // (4 * n))
    denoise.knn_points(cloud[:, :step].contiguous(), cloud, K=k)
    torch.cuda.synchronize()
    t0, done = time.perf_counter(), 0
    for q0 in range(0, n, step):
        denoise.knn_points(cloud[:, q0:q0 + step].contiguous(), cloud, K=k)
        torch.cuda.synchronize()
        done = min(n, q0 + step)
        if time.perf_counter() - t0 > budget:
            break
    spent = time.perf_counter() - t0
    return spent * n / done, done < n, done


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2000000)
    ap.add_argument("--brute-points", type=int, default=200000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-repeats", type=int, default=3)
    ap.add_argument("--brute-budget", type=float, default=60.0)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_scan_fusion needs a GPU: nothing is timed on the CPU alone")
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    def stages(n, brute):
        raw = torch.from_numpy(scan_ref.room(n, 0, ext=EXT)).cuda()
        faro_np = scan_ref.room(n // 2, 100, ext=EXT)
        faro = torch.from_numpy(faro_np).cuda()
        rgb = torch.rand(n, 3, device="cuda") * 255
        (xyz, _), t_vox = gpu_ms(lambda: SF.voxel_down_sample(raw, 0.01, rgb), a.repeats)
        emit({"what": "voxel_down_sample 0.01 (xyz + rgb)", "points_in": n, "voxels": xyz.shape[0], **t_vox})
        keep, t_out = gpu_ms(lambda: SF.outlier_removal(xyz, 10, 0.05, std_thresh=2.0), a.repeats)
        emit({"what": "outlier_removal k=20 std_thresh=2 (grid)", "points": xyz.shape[0], "kept": int(keep.sum()), **t_out})
        _, t_kth = gpu_ms(lambda: SF.knn_kth_distance(xyz, xyz, 20), a.repeats)
        emit({"what": "  of which knn_kth_distance k=20", "points": xyz.shape[0], **t_kth})
        kept = xyz[keep].contiguous()
        keep2, t_far = gpu_ms(lambda: SF.filter_iphone_scan(kept, faro), a.repeats)
        emit({"what": "filter_iphone_scan 1-NN (grid)", "queries": kept.shape[0], "ref": faro.shape[0], "kept": int(keep2.sum()), **t_far})

        pts = xyz.cpu().numpy()
        kth, c_out = cpu_ms(lambda: scan_ref.kth_distance(pts, pts, 20, workers=a.workers), a.cpu_repeats)
        emit({"what": f"cKDTree build + k=20 self-query, workers={a.workers}", "points": len(pts), **c_out})
        want = scan_ref.threshold_decisions(kth, *scan_ref.std_band(kth, 2.0, 2.0))
        left_out = scan_ref.compare_masks(keep.cpu().numpy(), *want)
        kept_np = kept.cpu().numpy()
        nn, c_far = cpu_ms(lambda: scan_ref.kth_distance(kept_np, faro_np, 1, workers=a.workers), a.cpu_repeats)
        emit({"what": f"cKDTree build + 1-NN query, workers={a.workers}", "queries": len(kept_np), "ref": len(faro_np), **c_far})
        left_out += scan_ref.compare_masks(keep2.cpu().numpy(),
                                           *scan_ref.threshold_decisions(nn, None, scan_ref.std_band(nn, None, 1.0)[1]))
        summary = {"what": "summary", "points": n, "masks_agree_with_cKDTree": True, "points_in_margin": left_out,
                   "grid_ms": t_vox["ms_median"] + t_out["ms_median"] + t_far["ms_median"],
                   "grid_knn_stages_ms": t_out["ms_median"] + t_far["ms_median"],
                   "ckdtree_knn_stages_ms": c_out["ms_median"] + c_far["ms_median"]}
        if brute:
            seconds, extrapolated, done = brute_kth(xyz, 20, a.brute_budget)
            emit({"what": "knn_points brute force, k=20 self-query", "points": xyz.shape[0], "ms": seconds * 1e3,
                  "extrapolated": extrapolated, "queries_run": done})
            summary["brute_k20_ms"], summary["grid_k20_ms"] = seconds * 1e3, t_kth["ms_median"]
        emit(summary)

    emit({"what": "setup", "device": torch.cuda.get_device_name(0), "room": EXT, "cpu_threads": a.workers})
    stages(a.brute_points, brute=True)
    stages(a.points, brute=False)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
