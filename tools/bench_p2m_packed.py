"""Timing of the packed point <-> mesh loss operators (p2p_bridge_amd/p2m.py, csrc/p2m_packed.hip): forward + backward of the four
kinds at 8 examples x 2048 points, each against its own 20 000-face mesh (a tessellated sphere; edges: every face's first side),
default and deterministic mode, beside an fp32 torch-autograd evaluation of the CHOSEN pairs alone on the same GPU (the
restatement of tests/p2m_ref.py: what a loss written in eager torch would pay for the gradient once it had the indices).
    python tools/bench_p2m_packed.py [--out report.txt]"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

N, POINTS, NLAT, NLON = 8, 2048, 101, 100  # 2 * 101 * 100 - 200 collapsed pole triangles = 20 000 faces


def scene():
    from bench_p2m_grid import uv_sphere

    g = torch.Generator().manual_seed(0)
    tris, pts = [], []
    for b in range(N):
        t = uv_sphere((0.0, 0.0, 0.0), 0.8 + 0.02 * b, NLAT, NLON)
        pick = torch.randint(0, t.shape[0], (POINTS,), generator=g)
        w = torch.rand(POINTS, 3, generator=g)
        w = w / w.sum(1, keepdim=True)
        pts.append((t[pick] * w[:, :, None]).sum(1) + 0.01 * torch.randn(POINTS, 3, generator=g))
        tris.append(t)
    first = lambda xs: torch.tensor([sum(x.shape[0] for x in xs[:i]) for i in range(len(xs))], dtype=torch.int64)
    return torch.cat(pts).contiguous(), first(pts), torch.cat(tris).contiguous(), first(tris), max(t.shape[0] for t in tris)


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    import p2m_ref as R

    import p2p_bridge_amd
    from p2p_bridge_amd import p2m as P

    pts, pfirst, tris, tfirst, max_tris = scene()
    pts, pfirst, tris, tfirst = pts.cuda(), pfirst.cuda(), tris.cuda(), tfirst.cuda()
    lines = [f"{N} examples x {POINTS} points, {tris.shape[0] // N} faces per example ({tris.shape[0]} packed), min_triangle_area 5e-3; "
             "host clock around forward + backward with a device synchronise, best of 5 after a warm-up, ms",
             f"{'kind':<12} {'forward':>9} {'fwd+bwd':>9} {'fwd+bwd det':>12} {'torch fp32 autograd, chosen pairs':>34}"]
    for kind in R.KINDS:
        qp = kind.startswith("point")
        prims = tris if "face" in kind else tris[:, :2].contiguous()
        extra = (5e-3,) if "face" in kind else ()
        fn = getattr(P, kind + "_distance")
        maxq = POINTS if qp else max_tris

        def both(det=False):
            a, b = pts.detach().requires_grad_(), prims.detach().requires_grad_()
            d = fn(a, pfirst, b, tfirst, maxq, *extra)
            with p2p_bridge_amd.deterministic(det):
                d.sum().backward()
            return d

        with torch.no_grad():
            t_f = timed(lambda: fn(pts, pfirst, prims, tfirst, maxq, *extra))
        t_fb, t_det = timed(both), timed(lambda: both(True))
        d = fn(pts.detach().requires_grad_(), pfirst, prims, tfirst, maxq, *extra)
        idx = d.grad_fn.saved_tensors[2]

        def eager():
            a, b = pts.detach().requires_grad_(), prims.detach().requires_grad_()
            p, pr = (a, b[idx]) if qp else (a[idx], b)
            R.pair_d2(p, pr, 5e-3)[0].sum().backward()

        lines.append(f"{kind:<12} {t_f:9.3f} {t_fb:9.3f} {t_det:12.3f} {timed(eager):34.3f}")
        print(lines[-1], flush=True)
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
