"""Times the set-level metrics (p2p_bridge_amd/evaluation_metrics_fast.py, csrc/setmetrics.hip) against the reference's algorithm
run through the package's existing drop-in ops -- one expand().contiguous() of a cloud and one batched chamfer / approxmatch
call per (cloud, batch of the other set), four matrix passes per metric (metrics/evaluation_metrics_fast.py:209-231, :423-464):
what a user of the drop-in got before the pairwise kernels existed. Not part of bench.py.

    python tools/bench_set_metrics.py [--cd-clouds 256] [--emd-clouds 64] [--points 2048] [--repeats 5] [--out FILE]

One process, seeded inputs, every shape warmed up before it is timed, the two paths alternated inside each repeat, host clock
around a device synchronise; the minimum and the median over the repeats are reported. The Chamfer rate is point-pair distances
EVALUATED per second (a symmetric matrix evaluates each directional sum once, so half the pairs of the general case) and its
share of the packed-fp32 VALU peak (157.3 TFLOP/s) at 8 FLOP per pair (3 subtractions, 1 multiplication, 2 fused multiply-adds);
the minimum is not counted. Needs a GPU: there is no CPU timing."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from p2p_bridge_amd import evaluation_metrics_fast as E  # noqa: E402
from p2p_bridge_amd import metrics  # noqa: E402

VALU_PEAK_FLOPS = 157.3e12  # packed fp32, MI355X
FLOP_PER_PAIR = 8


def clouds(count, points, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(count, points, 3, generator=g)
    x = x / x.norm(dim=2, keepdim=True) * torch.rand(count, points, 1, generator=g) ** (1 / 3) * 0.5
    return (x * (0.6 + 0.4 * torch.rand(count, 1, 3, generator=g))).cuda().contiguous()


def baseline_matrix(metric, A, B, batch):
    rows = []
    for i in range(A.shape[0]):
        row = []
        for lo in range(0, B.shape[0], batch):
            b = B[lo:lo + batch]
            a = A[i].view(1, -1, 3).expand(b.shape[0], -1, -1).contiguous()
            if metric == "CD":
                d1, d2, _, _ = metrics.chamfer_3DDist_nograd()(a, b)
                row.append((d1.mean(dim=1) + d2.mean(dim=1)).view(1, -1))
            else:
                row.append(metrics.earth_mover_distance_nograd(a, b, transpose=False).view(1, -1))
        rows.append(torch.cat(row, dim=1))
    return torch.cat(rows, dim=0)


def baseline_all(metric, smp, ref):
    """the reference's compute_all_metrics for one metric: rs twice, rr, ss, then the statistics"""
    batch = ref.shape[0] // 2
    baseline_matrix(metric, ref, smp, batch)
    M_rs = baseline_matrix(metric, ref, smp, batch)
    out = {k: v.item() for k, v in E.lgan_mmd_cov(M_rs.t()).items()}
    M_rr, M_ss = baseline_matrix(metric, ref, ref, batch), baseline_matrix(metric, smp, smp, batch)
    out.update({k: v.item() for k, v in E.knn(M_rr, M_rs, M_ss, 1).items() if "acc" in k})
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def compare(name, new, old, repeats, work=None):
    new(), old()  # warm-up: code objects, allocator, clocks
    tn, to = [], []
    for _ in range(repeats):
        tn.append(timed(new)[0])
        to.append(timed(old)[0])
    row = {"what": name, "new_s_min": min(tn), "new_s_median": statistics.median(tn), "baseline_s_min": min(to),
           "baseline_s_median": statistics.median(to), "speedup_median": statistics.median(to) / statistics.median(tn)}
    if work:
        row["pairs_evaluated"] = work
        row["new_pairs_per_s"] = work / min(tn)
        row["new_share_of_valu_peak"] = work * FLOP_PER_PAIR / min(tn) / VALU_PEAK_FLOPS
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cd-clouds", type=int, default=256)
    ap.add_argument("--emd-clouds", type=int, default=64)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_set_metrics needs a GPU: nothing is timed on the CPU")
    n = args.points
    rows = []
    # ---- Chamfer
    c = args.cd_clouds
    smp, ref = clouds(c, n, 1), clouds(c, n, 2)
    new_rs, old_rs = E.pairwise_chamfer(ref, smp), baseline_matrix("CD", ref, smp, c // 2)
    agree_cd = ((new_rs - old_rs).abs() / old_rs).max().item()
    rows.append(compare(f"CD matrix {c}x{c}x{n} (general)", lambda: E.pairwise_chamfer(ref, smp),
                        lambda: baseline_matrix("CD", ref, smp, c // 2), args.repeats, work=2.0 * c * c * n * n))
    rows.append(compare(f"CD matrix {c}x{c}x{n} (symmetric)", lambda: E.pairwise_chamfer(ref, ref),
                        lambda: baseline_matrix("CD", ref, ref, c // 2), args.repeats, work=1.0 * c * c * n * n))
    rows.append(compare(f"compute_all_metrics CD only {c}x{c}x{n}",
                        lambda: E.compute_all_metrics(smp, ref, c, verbose=False, accelerated_cd=True, metric2=None),
                        lambda: baseline_all("CD", smp, ref), max(2, args.repeats // 2)))
    # ---- EMD
    e = args.emd_clouds
    smp, ref = clouds(e, n, 3), clouds(e, n, 4)
    new_rs, old_rs = E.pairwise_emd(ref, smp), baseline_matrix("EMD", ref, smp, e // 2)
    agree_emd = ((new_rs - old_rs).abs() / old_rs).max().item()
    rows.append(compare(f"EMD matrix {e}x{e}x{n}", lambda: E.pairwise_emd(ref, smp),
                        lambda: baseline_matrix("EMD", ref, smp, e // 2), max(2, args.repeats // 2)))
    rows.append(compare(f"compute_all_metrics EMD only {e}x{e}x{n}",
                        lambda: E.compute_all_metrics(smp, ref, e, verbose=False, accelerated_cd=True, metric1="EMD", metric2=None),
                        lambda: baseline_all("EMD", smp, ref), 2))
    # ---- JSD counters (no baseline on the device: the reference runs sklearn on the host)
    t_occ = min(timed(lambda: E.occupancy_counts(smp, 28, True))[0] for _ in range(3))
    result = {"device": torch.cuda.get_device_name(0), "rows": rows, "cd_new_vs_baseline_max_rel": agree_cd,
              "emd_new_vs_baseline_max_rel": agree_emd, "occupancy_counts_s": t_occ,
              "occupancy_shape": [e, n, 28], "valu_peak_flops": VALU_PEAK_FLOPS, "flop_per_pair": FLOP_PER_PAIR}
    lines = [f"{r['what']}: new {r['new_s_median'] * 1e3:.2f} ms (min {r['new_s_min'] * 1e3:.2f}), baseline "
             f"{r['baseline_s_median'] * 1e3:.2f} ms (min {r['baseline_s_min'] * 1e3:.2f}), x{r['speedup_median']:.2f}"
             + (f", {r['new_pairs_per_s'] / 1e12:.2f} T pairs/s = {100 * r['new_share_of_valu_peak']:.1f} % of the packed-fp32 VALU peak"
                if "new_pairs_per_s" in r else "") for r in rows]
    lines.append(f"new vs baseline, max relative difference: CD {agree_cd:.2e}, EMD {agree_emd:.2e}")
    lines.append(f"occupancy_counts {e} x {n} points, resolution 28, sphere: {t_occ * 1e3:.2f} ms (with the copy of the counters to the host)")
    text = "\n".join(lines) + "\n" + json.dumps(result) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
