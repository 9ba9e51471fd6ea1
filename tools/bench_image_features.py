"""Times the image-feature stage (p2p_bridge_amd/image_features.py, csrc/imgfeat.hip) at the size of a ScanNet++ room: a synthetic
cloud of 10^6 points, 192 x 256 occlusion mask and feature maps, C = 384 (DINOv2 ViT-S), 20 frames in batches of 2.
  visible_points          per batch: projection, per-pixel lists, records of the running minimum
  update_features         per batch, HIP: one launch
  update_features_torch   the same inputs through this package's torch-operator path on the same device (the yardstick: the
                          reference's own stage needs numba / cuML / open3d and cannot run on this hardware)
  interpolate_missing_features   once, after all 20 frames: neighbour search (csrc/knn.hip, exhaustive) and the fill rounds,
                          timed apart. The neighbour search is O(missing x points): its first chunk is timed, and if the whole
                          would exceed --fill-budget seconds only as many unobserved points as fit are filled (the rest are
                          marked observed); the output says how many.
The fuse kernel's achieved bytes/s is quoted against its algorithmic traffic: c * 2 bytes per (frame, valid point) gathered, one
read of `mean`, one write of the rows that changed, plus valid / xy / count. Not part of bench.py.

    python tools/bench_image_features.py [--points 1000000] [--frames 20] [--batch 2] [--channels 384] [--repeats 7]
                                         [--window 0.25] [--fill-budget 120] [--out FILE]

One process, seeded inputs, every call warmed up before it is timed, device events around back-to-back calls (as many as fill
`window` seconds); median and minimum per call over the repeats. Needs a GPU."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from p2p_bridge_amd import image_features as IF  # noqa: E402

F16, F64, I32 = torch.float16, torch.float64, torch.int32
H, W = 192, 256


def per_call_ms(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def measure(name, fn, repeats, window):
    for _ in range(3):  # warm-up: code objects, allocator, clocks
        fn()
    torch.cuda.synchronize()
    iters = max(3, min(2000, int(window * 1e3 / per_call_ms(fn, 3)) + 1))
    t = [per_call_ms(fn, iters) for _ in range(repeats)]
    return {"what": name, "iters": iters, "ms_median": statistics.median(t), "ms_min": min(t)}


def rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]]) @ np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]])
            @ np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--channels", type=int, default=384)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--fill-budget", type=float, default=120.0, help="seconds the neighbour search of the fill may take")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_features needs a GPU: nothing is timed on the CPU")
    n, c, bs = a.points, a.channels, a.batch
    rng = np.random.default_rng(0)
    # a room seen from inside: points on the walls of a 6 x 4 x 3 m box plus clutter, cameras near the middle looking around
    pts = rng.uniform([-3, -2, -1.5], [3, 2, 1.5], (n, 3))
    wall = rng.integers(0, 3, n)
    on_wall = rng.random(n) < 0.7
    side = np.where(rng.random(n) < 0.5, -1.0, 1.0) * np.array([3, 2, 1.5])[wall]
    pts[np.arange(n)[on_wall], wall[on_wall]] = side[on_wall]
    points = torch.from_numpy(pts.astype(np.float32).astype(np.float64)).cuda()
    cam = np.array([[200.0, 0, 128.0], [0, 200.0, 96.0], [0, 0, 1.0]])
    rots = np.stack([rotation(0.3 * math.sin(f), 2 * math.pi * f / a.frames, 0.05 * f) for f in range(a.frames)])
    trs = rng.uniform(-0.5, 0.5, (a.frames, 3))
    gen = torch.Generator(device="cuda").manual_seed(0)
    maps = torch.randn(bs, H, W, c, generator=gen, device="cuda", dtype=torch.float32).to(F16)
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    emit({"what": "setup", "points": n, "frames": a.frames, "batch": bs, "channels": c, "mask": [H, W],
          "device": torch.cuda.get_device_name(0)})
    mean, count = torch.zeros(n, c, dtype=F16, device="cuda"), torch.zeros(n, dtype=I32, device="cuda")
    batches = []
    for b0 in range(0, a.frames, bs):
        r, t = torch.from_numpy(rots[b0:b0 + bs]).cuda(), torch.from_numpy(trs[b0:b0 + bs]).cuda()
        k = torch.from_numpy(np.repeat(cam[None], r.shape[0], 0)).cuda()
        valid, xy = IF.visible_points(points, r, t, k, W, H)
        IF.update_features(mean, count, maps[:r.shape[0]], valid, xy)
        batches.append((r, t, k, valid, xy))
    torch.cuda.synchronize()
    seen = [int(b[3].sum()) for b in batches]
    emit({"what": "scene", "valid_per_batch": seen, "unobserved": int((count == 0).sum()), "max_count": int(count.max())})

    r, t, k, valid, xy = batches[0]
    emit(measure("visible_points (B=%d)" % bs, lambda: IF.visible_points(points, r, t, k, W, H), a.repeats, a.window))
    nvalid, touched = int(valid.sum()), int(valid.any(0).sum())
    traffic = nvalid * c * 2 + n * c * 2 + touched * c * 2 + valid.numel() + nvalid * 8 + n * 4 + touched * 4
    m1, c1 = mean.clone(), count.clone()
    res = measure("update_features HIP (B=%d)" % bs, lambda: IF.update_features(m1, c1, maps, valid, xy), a.repeats, a.window)
    res.update({"valid_points": nvalid, "rows_changed": touched, "algorithmic_bytes": traffic,
                "GBps_at_median": traffic / res["ms_median"] / 1e6})
    emit(res)
    m2, c2 = mean.clone(), count.clone()
    res_t = measure("update_features_torch (B=%d)" % bs, lambda: IF.update_features_torch(m2, c2, maps, valid, xy), a.repeats,
                    a.window)
    res_t["hip_speedup_at_median"] = res_t["ms_median"] / res["ms_median"]
    emit(res_t)
    del m1, c1, m2, c2

    # ---- the fill, once ---------------------------------------------------------------------------------------------
    missing = torch.nonzero(count == 0).flatten()
    m = missing.numel()
    probe = min(m, 256)
    cloud = points.float().reshape(1, n, 3).contiguous()
    if probe:
        q = cloud[:, missing[:probe]].contiguous()
        from p2p_bridge_amd import denoise

        denoise.knn_points(q, cloud, K=10)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        denoise.knn_points(q, cloud, K=10)
        torch.cuda.synchronize()
        per_query = (time.perf_counter() - t0) / probe
        fit = int(a.fill_budget / per_query)
        if fit < m:
            count[missing[fit:]] = 1  # (marked observed: their zero rows drop out of every median)
        emit({"what": "fill neighbour search probe", "queries": probe, "us_per_query": per_query * 1e6, "unobserved": m,
              "filled_in_this_run": min(m, fit)})
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, rounds = IF.interpolate_missing_features(mean, count, cloud[0], return_rounds=True)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        emit({"what": "interpolate_missing_features (whole call, once)", "seconds": total, "rounds": rounds,
              "points_filled": min(m, fit), "estimated_neighbour_search_seconds": per_query * min(m, fit)})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
