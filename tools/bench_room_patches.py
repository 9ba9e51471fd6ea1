"""Times the two patch builders of the room pipeline (p2p_bridge_amd/denoise_room.py) against each other on the same GPU, same room,
same radius lists, same generator seed. Not part of bench.py.

      loop       create_patches: one batch-1 FPS launch per subset, one host synchronisation per padded patch
      batched    create_patches_batched: the draws on the host first, then every FPS subset of the room as a ragged job, one workgroup
                 each, one launch per size tier (csrc/room_patches.hip), one bounding-box launch, one assembly launch

    python tools/bench_room_patches.py [--points 1800000] [--patch-size 4096] [--k 3] [--radius 0.3] [--repeats 3] [--small]
                                       [--out profiles/room_patches_timing.txt]

The room is seeded and synthetic: a floor, two walls and clutter in 4 x 3 x 2.5 m (the generator of tests/test_room_gpu.py). FPS
centres and the radius query run once; then each builder is warmed up once (code objects, allocator), and the two are ALTERNATED
inside every repeat. A timed call ends in a device synchronise, so the host clock around it is the time to finished patches; median and minimum per call over the repeats, and the loop's own spread (max - min) as the yardstick a gain has
to exceed. Per-tier kernel times of the batched builder come from device events around each tier's launch. The two results are
compared for equality once. --small: a 60 000-point room with patches of 512 that finishes in seconds. Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from p2p_bridge_amd import denoise_room as R  # noqa: E402
from p2p_bridge_amd import pointnet2_batch_cuda as ext  # noqa: E402


def room(n, seed=0):
    """a synthetic room: floor + two walls + clutter, metres"""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(n, 3, generator=g)
    which = torch.randint(0, 4, (n,), generator=g)
    p = torch.stack([u[:, 0] * 4.0, u[:, 1] * 3.0, u[:, 2] * 2.5], 1)
    p[which == 0, 2] = 0.0
    p[which == 1, 0] = 0.0
    p[which == 2, 1] = 3.0
    return (p + 0.005 * torch.randn(n, 3, generator=g)).contiguous()


class Calls:
    """counts the library calls of both builders; with `events`, device events around every FPS-jobs launch, by tier"""

    def __init__(self):
        self.names, self.events, self.timed = [], [], False
        self._real = (R.call, ext.call)

    def __enter__(self):
        real = self._real[0]

        def counting(name, *a):
            self.names.append(name)
            if self.timed and name == "p2pb_room_fps_jobs":
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                real(name, *a)
                e1.record()
                self.events.append((a[0].value, a[1].value, e0, e1))
                return None
            return real(name, *a)

        R.call = ext.call = counting
        return self

    def __exit__(self, *exc):
        R.call, ext.call = self._real
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1800000)
    ap.add_argument("--patch-size", type=int, default=4096)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--radius", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--small", action="store_true", help="60 000 points, patches of 512: finishes in seconds")
    ap.add_argument("--out", default=None, help="default: profiles/room_patches_timing.txt (nothing is written with --small)")
    a = ap.parse_args()
    if a.small:
        a.points, a.patch_size = 60000, 512
    elif a.out is None:
        a.out = os.path.join(ROOT, "profiles", "room_patches_timing.txt")
    if not torch.cuda.is_available():
        raise SystemExit("bench_room_patches needs a GPU: nothing is timed on the CPU")
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    pts = room(a.points, a.seed).cuda()
    n_centres = int(-(-a.points // a.patch_size) * a.k)
    cidx = ext.furthest_point_sampling_forward(pts.t().contiguous()[None], n_centres)[0].long()
    idx_flat, offsets = R.radius_query(pts[cidx].contiguous(), pts, a.radius)
    L = (offsets[1:] - offsets[:-1]).cpu()
    plan = R.plan_patches(offsets, a.patch_size, torch.Generator().manual_seed(1))
    jl = L[plan["centre"][plan["job_patch"]]]
    tiers = torch.bucketize(jl, torch.tensor(R.FPS_JOB_TIERS)).bincount(minlength=len(R.FPS_JOB_TIERS) + 1).tolist()
    emit({"what": "setup", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "points": a.points,
          "patch_size": a.patch_size, "k": a.k, "radius": a.radius, "centres": n_centres, "list_points_total": int(idx_flat.numel()),
          "list_len_min": int(L.min()), "list_len_median": int(L.median()), "list_len_max": int(L.max()),
          "patches": int(plan["centre"].numel()), "fps_jobs": int(jl.numel()), "padded_patches": int(plan["pad_patch"].numel()),
          "fps_job_tiers": list(R.FPS_JOB_TIERS) + ["streaming"], "fps_jobs_per_tier": tiers})

    def loop():
        out = R.create_patches(pts, idx_flat, offsets, a.patch_size, torch.Generator().manual_seed(1))
        torch.cuda.synchronize()
        return out

    def batched():
        out = R.create_patches_batched(pts, idx_flat, offsets, a.patch_size, torch.Generator().manual_seed(1))
        torch.cuda.synchronize()
        return out

    with Calls() as calls:  # warm-up of both, the call counts, the per-tier event times, and the agreement
        ref = loop()
        n_loop = len(calls.names)
        calls.names.clear()
        got = batched()
        n_batched, names = len(calls.names), list(calls.names)
        calls.timed = True
        batched()
        torch.cuda.synchronize()
        per_tier = [{"tier": t, "jobs": j, "ms": e0.elapsed_time(e1)} for t, j, e0, e1 in calls.events]
    same = all(torch.equal(ref[key].cpu(), got[key].cpu()) for key in ("xyz", "idx", "cuts"))
    emit({"what": "library calls per builder call", "loop": n_loop, "batched": n_batched, "batched_bound": R.BATCHED_MAX_LIBRARY_CALLS,
          "batched_calls": names})
    emit({"what": "batched builder, kernel time per tier (device events)", "tiers": per_tier,
          "ms_all_tiers": sum(p["ms"] for p in per_tier)})
    emit({"what": "agreement", "xyz_idx_cuts_equal": same})
    del ref, got

    times = {"loop": [], "batched": []}
    for _ in range(a.repeats):
        for name, fn in (("loop", loop), ("batched", batched)):
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    for name in ("loop", "batched"):
        emit({"what": f"create_patches{'_batched' if name == 'batched' else ''}", "repeats": a.repeats,
              "ms_median": statistics.median(times[name]), "ms_min": min(times[name]), "ms_max": max(times[name]),
              "ms_spread": max(times[name]) - min(times[name])})
    gain = statistics.median(times["loop"]) - statistics.median(times["batched"])
    emit({"what": "verdict", "loop_over_batched_at_median": statistics.median(times["loop"]) / statistics.median(times["batched"]),
          "ms_saved_at_median": gain, "loop_ms_spread": max(times["loop"]) - min(times["loop"]),
          "gain_exceeds_loop_spread": gain > max(times["loop"]) - min(times["loop"])})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
