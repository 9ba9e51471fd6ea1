"""Times the five classic PointNet++ operators (csrc/ball_query.hip, csrc/three_nn.hip; FPS: csrc/fps_ref.hip) at a set-abstraction
shape (B = 16, N = 8192 -> M = 2048, nsample = 32, C = 64) through the `*_wrapper` functions of p2p_bridge_amd/pointnet2_batch_cuda.py, each next to a comparator
in the same run: what a user of the package could do before these operators existed -- transpose the point-major tensors to
channel-major, call the existing PVCNN operator, transpose the result back. The comparator is a yardstick for TIME only: its
FPS breaks ties like a 512-thread block, its ball query zero-fills the rows without a neighbour, its 3-NN returns weights
instead of distances. Not part of bench.py.

    python tools/bench_pointnet2_legacy.py [--batch 16] [--points 8192] [--centres 2048] [--nsample 32] [--channels 64]
                                           [--radius 0.2] [--repeats 7] [--window 0.25] [--commit TEXT] [--out FILE]

One process, seeded inputs, every call warmed up before it is timed, new and comparator alternated inside each repeat, device
events around back-to-back calls -- as many as fill `window` seconds for the slower of the two, counted after the warm-up;
median and minimum of the per-call time over the repeats. Both columns include the
output allocation / initialisation their callers have to do (temp fill, idx zero fill, gradient zero fill). Needs a GPU."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from p2p_bridge_amd import pointnet2_batch_cuda as ext  # noqa: E402

F32, I32 = torch.float32, torch.int32


def per_call_ms(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def compare(name, new, old, repeats, window):
    for _ in range(3):  # warm-up: code objects, allocator, clocks
        new(), old()
    torch.cuda.synchronize()
    iters = max(5, min(5000, int(window * 1e3 / max(per_call_ms(new, 5), per_call_ms(old, 5))) + 1))
    tn, to = [], []
    for _ in range(repeats):
        tn.append(per_call_ms(new, iters))
        to.append(per_call_ms(old, iters))
    return {"what": name, "iters": iters, "new_ms_median": statistics.median(tn), "new_ms_min": min(tn),
            "comparator_ms_median": statistics.median(to), "comparator_ms_min": min(to),
            "comparator_over_new": statistics.median(to) / statistics.median(tn)}


def cm(t):
    """[B, N, K] -> channel-major [B, K, N], contiguous (a launch of its own: part of the comparator's price)"""
    return t.transpose(1, 2).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--centres", type=int, default=2048)
    ap.add_argument("--nsample", type=int, default=32)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--radius", type=float, default=0.2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pointnet2_legacy needs a GPU: nothing is timed on the CPU")
    B, N, M, U, C = a.batch, a.points, a.centres, a.nsample, a.channels
    g = torch.Generator().manual_seed(0)
    xyz = (torch.rand(B, N, 3, generator=g) * 2 - 1).cuda()
    feat_m = torch.randn(B, C, M, generator=g).cuda()
    grad_n = torch.randn(B, C, N, generator=g).cuda()

    def fps_new():
        temp = torch.empty(B, N, dtype=F32, device="cuda").fill_(1e10)
        idx = torch.empty(B, M, dtype=I32, device="cuda")
        ext.furthest_point_sampling_wrapper(B, N, M, xyz, temp, idx)
        return idx

    def fps_old():
        return ext.furthest_point_sampling_forward(cm(xyz), M)

    centres_idx = fps_new()
    new_xyz = torch.gather(xyz, 1, centres_idx.long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()

    def bq_new():
        idx = torch.zeros(B, M, U, dtype=I32, device="cuda")
        ext.ball_query_wrapper(B, N, M, a.radius, U, new_xyz, xyz, idx)
        return idx

    def bq_old():
        return ext.ball_query(cm(new_xyz), cm(xyz), a.radius, U)

    def nn_new():
        dist2 = torch.empty(B, N, 3, dtype=F32, device="cuda")
        idx = torch.empty(B, N, 3, dtype=I32, device="cuda")
        ext.three_nn_wrapper(B, N, M, xyz, new_xyz, dist2, idx)
        return dist2, idx

    def nn_old():
        idx, w = ext.three_nn(cm(xyz), cm(new_xyz))
        return cm(w), cm(idx)

    dist2, idx3 = nn_new()
    recip = 1.0 / (dist2.sqrt() + 1e-8)
    w3 = (recip / recip.sum(dim=2, keepdim=True)).contiguous()

    def ti_new():
        out = torch.empty(B, C, N, dtype=F32, device="cuda")
        ext.three_interpolate_wrapper(B, C, M, N, feat_m, idx3, w3, out)
        return out

    def ti_old():
        return ext.three_interpolate(feat_m, cm(idx3), cm(w3))

    def tig_new():
        grad = torch.zeros(B, C, M, dtype=F32, device="cuda")
        ext.three_interpolate_grad_wrapper(B, C, N, M, grad_n, idx3, w3, grad)
        return grad

    def tig_old():
        return ext.three_nearest_neighbors_interpolate_backward(grad_n, cm(idx3), cm(w3), M)

    # what the two columns compute: equal where the contracts coincide (random fp32 clouds: no ties, every ball has its centre)
    agree = {
        "fps_idx_equal": bool(torch.equal(fps_new(), fps_old())),
        "ball_query_idx_equal": bool(torch.equal(bq_new(), bq_old())),
        "three_nn_idx_equal": bool(torch.equal(nn_new()[1], nn_old()[1])),
        "three_interpolate_max_abs_diff": (ti_new() - ti_old()).abs().max().item(),
        "three_interpolate_grad_max_abs_diff": (tig_new() - tig_old()).abs().max().item(),
    }
    shape = f"B {B}, N {N}, M {M}"
    rows = [
        compare(f"furthest point sampling ({shape})", fps_new, fps_old, a.repeats, a.window),
        compare(f"ball query ({shape}, radius {a.radius}, nsample {U})", bq_new, bq_old, a.repeats, a.window),
        compare(f"three_nn ({shape})", nn_new, nn_old, a.repeats, a.window),
        compare(f"three_interpolate ({shape}, C {C})", ti_new, ti_old, a.repeats, a.window),
        compare(f"three_interpolate_grad ({shape}, C {C})", tig_new, tig_old, a.repeats, a.window),
    ]
    # the interpolation columns differ by the order of fp32 atomic adds at most
    mismatch = [k for k, v in agree.items() if (v is False) or (not isinstance(v, bool) and v > 1e-3)]
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip, "commit": a.commit,
              "repeats": a.repeats, "window_s": a.window, "rows": rows, "agreement": agree, "mismatch": mismatch}
    lines = [f"box: {result['device']}, torch {result['torch']}, HIP {result['hip']}; commit: {a.commit}",
             f"per call, median (min) over {a.repeats} repeats of windows of about {a.window} s; comparator = transpose to "
             "channel-major + the existing PVCNN operator + transpose back"]
    for r in rows:
        verdict = "new is faster" if r["comparator_over_new"] > 1.0 else "NEW KERNEL LOSES to the comparator"
        lines.append(f"{r['what']} [{r['iters']} calls per window]: new {r['new_ms_median']:.3f} ms ({r['new_ms_min']:.3f}), comparator "
                     f"{r['comparator_ms_median']:.3f} ms ({r['comparator_ms_min']:.3f}), comparator / new = "
                     f"{r['comparator_over_new']:.2f} -- {verdict}")
    lines.append("agreement of the two columns on this data: " + ", ".join(f"{k} {v}" for k, v in agree.items()))
    if mismatch:
        lines.append("MISMATCH between the two columns at the timed size (they should agree on this data): " + ", ".join(mismatch))
    text = "\n".join(lines) + "\n" + json.dumps(result) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
