"""Times the three search operators of the pointops extension (csrc/pointops.hip; furthestsampling: csrc/fps_ref.hip) at a
Point-Transformer-like shape through the `*_cuda` functions of p2p_bridge_amd/pointops_cuda.py: b = 4 equal segments, uniform fp32 clouds in [-1, 1]^3,
  knnquery           n = m = 40960 (the cloud queries itself), nsample 16
  ballquery          the same shape, radius 0.1
  furthestsampling   40960 -> 10240
There is no earlier implementation on this hardware to compare with; the figures are absolute. Not part of bench.py.

    python tools/bench_pointops.py [--segments 4] [--points 40960] [--samples 10240] [--nsample 16] [--radius 0.1]
                                   [--repeats 7] [--window 0.25] [--commit TEXT] [--out FILE]

One process, seeded inputs, every call warmed up before it is timed, device events around back-to-back calls -- as many as fill
`window` seconds, counted after the warm-up; median and minimum of the per-call time over the repeats. Each figure includes the
output initialisation its caller has to do (idx / dist2 zero fill, tmp fill). Needs a GPU."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from p2p_bridge_amd import pointops_cuda as ext  # noqa: E402

F32, I32 = torch.float32, torch.int32


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
    iters = max(3, min(5000, int(window * 1e3 / per_call_ms(fn, 3)) + 1))
    t = [per_call_ms(fn, iters) for _ in range(repeats)]
    return {"what": name, "iters": iters, "ms_median": statistics.median(t), "ms_min": min(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=4)
    ap.add_argument("--points", type=int, default=40960)
    ap.add_argument("--samples", type=int, default=10240)
    ap.add_argument("--nsample", type=int, default=16)
    ap.add_argument("--radius", type=float, default=0.1)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pointops needs a GPU: nothing is timed on the CPU")
    b, n, ms, u = a.segments, a.points, a.samples, a.nsample
    seg, sseg = n // b, ms // b
    g = torch.Generator().manual_seed(0)
    xyz = (torch.rand(n, 3, generator=g) * 2 - 1).cuda()
    offset = torch.arange(1, b + 1, dtype=I32, device="cuda") * seg
    new_offset = torch.arange(1, b + 1, dtype=I32, device="cuda") * sseg

    def knn():
        idx = torch.zeros(n, u, dtype=I32, device="cuda")
        dist2 = torch.zeros(n, u, dtype=F32, device="cuda")
        ext.knnquery_cuda(n, u, xyz, xyz, offset, offset, idx, dist2)
        return idx

    def ball():
        idx = torch.zeros(n, u, dtype=I32, device="cuda")
        ext.ballquery_cuda(n, a.radius, u, xyz, xyz, offset, offset, idx)
        return idx

    def fps():
        tmp = torch.full((n,), 1e10, dtype=F32, device="cuda")
        idx = torch.zeros(b * sseg, dtype=I32, device="cuda")
        ext.furthestsampling_cuda(b, seg, xyz, offset, new_offset, tmp, idx)
        return idx

    shape = f"b {b}, n = m = {n}"
    rows = [measure(f"knnquery ({shape}, nsample {u})", knn, a.repeats, a.window),
            measure(f"ballquery ({shape}, radius {a.radius}, nsample {u})", ball, a.repeats, a.window),
            measure(f"furthestsampling (b {b}, {n} -> {b * sseg})", fps, a.repeats, a.window)]
    pairs = float(b) * seg * seg  # query-point pairs a search visits (ballquery stops early where its rows fill)
    rows[0]["pairs_per_s"] = pairs / (rows[0]["ms_median"] * 1e-3)
    hits = (ball() != 0).any(1).float().mean().item()
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip, "commit": a.commit,
              "repeats": a.repeats, "window_s": a.window, "rows": rows}
    lines = [f"box: {result['device']}, torch {result['torch']}, HIP {result['hip']}; commit: {a.commit}",
             f"per call, median (min) over {a.repeats} repeats of windows of about {a.window} s"]
    for r in rows:
        lines.append(f"{r['what']} [{r['iters']} calls per window]: {r['ms_median']:.3f} ms ({r['ms_min']:.3f})")
    lines.append(f"knnquery: {pairs:.3g} query-point pairs per call, {rows[0]['pairs_per_s']:.3g} pairs/s; "
                 f"ballquery rows with a neighbour besides point 0: {hits:.3f}")
    text = "\n".join(lines) + "\n" + json.dumps(result) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
