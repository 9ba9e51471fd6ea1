"""Timing of the point-to-mesh metric at room shape: brute force (csrc/p2m.hip) vs grid (csrc/p2m_grid.hip), equal outputs.
A synthetic room: a box of two triangles per wall and eight finely tessellated spheres (198 924 faces), 300 000 points near
its surfaces, on the mesh's unit sphere; min_triangle_area 5e-3 (evaluate_rooms) and 0. Two processes, one after the other:
  --stage brute : times the two brute-force entry points, stores their outputs
  --stage grid  : times index build + the two grid queries, asserts torch.equal with the stored outputs, writes the report"""
import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def uv_sphere(center, radius, nlat, nlon):
    th = torch.linspace(0, math.pi, nlat + 1)
    ph = torch.linspace(0, 2 * math.pi, nlon + 1)[:-1]
    v = torch.stack([torch.sin(th)[:, None] * torch.cos(ph)[None], torch.sin(th)[:, None] * torch.sin(ph)[None],
                     torch.cos(th)[:, None].expand(-1, nlon)], -1) * radius + torch.tensor(center)
    a, b = v[:-1], v[1:]
    a2, b2 = torch.roll(a, -1, 1), torch.roll(b, -1, 1)
    t = torch.cat([torch.stack([a, b, b2], 2).reshape(-1, 3, 3), torch.stack([a, b2, a2], 2).reshape(-1, 3, 3)], 0)
    area = torch.linalg.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]).norm(dim=1)
    return t[area > 1e-9]  # (the collapsed triangles at the poles are dropped)


def scene():
    g = torch.Generator().manual_seed(0)
    c = torch.tensor([[x, y, z] for z in (-1.0, 1.0) for y in (-1.0, 1.0) for x in (-1.0, 1.0)])
    f = torch.tensor([[0, 1, 3], [0, 3, 2], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                      [1, 3, 7], [1, 7, 5]])
    centers = [(-0.5, -0.5, -0.5), (0.5, -0.5, -0.5), (-0.5, 0.5, -0.5), (0.5, 0.5, -0.5), (-0.5, -0.5, 0.5), (0.5, -0.5, 0.5),
               (-0.5, 0.5, 0.5), (0.5, 0.5, 0.5)]
    tris = torch.cat([c[f]] + [uv_sphere(ct, 0.3, 112, 112) for ct in centers], 0)
    # 2e5 points near the spheres (jittered barycentric samples), 1e5 near the walls
    pick = torch.randint(12, tris.shape[0], (200_000,), generator=g)
    w = torch.rand(200_000, 3, generator=g)
    w = w / w.sum(1, keepdim=True)
    on = (tris[pick] * w[:, :, None]).sum(1) + 0.004 * torch.randn(200_000, 3, generator=g)
    wall = torch.rand(100_000, 3, generator=g) * 2 - 1
    ax, side = torch.randint(0, 3, (100_000,), generator=g), torch.randint(0, 2, (100_000,), generator=g) * 2.0 - 1
    wall[torch.arange(100_000), ax] = side * (1 - 0.004 * torch.rand(100_000, generator=g))
    pts = torch.cat([on, wall], 0)
    scale = tris.reshape(-1, 3).norm(dim=1).max()  # the mesh's unit sphere, as metrics.point_face_dist normalises
    return (pts / scale).contiguous(), (tris / scale).contiguous()


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stage", required=True, choices=["brute", "grid"])
    ap.add_argument("--out", default=os.path.join(ROOT, "prof_out"), help="directory for the stored outputs and the report")
    args = ap.parse_args()
    OUT = args.out
    from p2p_bridge_amd import metrics as M

    os.makedirs(OUT, exist_ok=True)
    pts, tris = scene()
    dp, dt = pts.cuda(), tris.cuda()
    report = {"points": pts.shape[0], "faces": tris.shape[0]}
    for area in (5e-3, 0.0):
        tag = f"area{area:g}"
        if args.stage == "brute":
            t_pf, pf = timed(lambda: M.point_face_distance(dp, dt, area), 1)
            print(tag, "brute point_face", t_pf, flush=True)
            t_fp, fp = timed(lambda: M.face_point_distance(dp, dt, area), 1)
            print(tag, "brute face_point", t_fp, flush=True)
            torch.save({"pf": [t.cpu() for t in pf], "fp": [t.cpu() for t in fp], "t_pf": t_pf, "t_fp": t_fp},
                       os.path.join(OUT, f"p2m_brute_{tag}.pt"))
        else:
            ref = torch.load(os.path.join(OUT, f"p2m_brute_{tag}.pt"))
            t_build, grid = timed(lambda: M.TriangleGrid(dt, area), 3)
            t_pf, pf = timed(lambda: grid.point_face(dp, return_stats=True), 3)
            t_fp, fp = timed(lambda: grid.face_point(dp, return_stats=True), 3)
            for got, want, name in ((pf, ref["pf"], "point_face"), (fp, ref["fp"], "face_point")):
                assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1]), f"{tag} {name}: grid != brute"
            report[tag] = {"brute_point_face_s": ref["t_pf"], "brute_face_point_s": ref["t_fp"], "grid_build_s": t_build,
                           "grid_point_face_s": t_pf, "grid_face_point_s": t_fp, "point_face_stats": pf[2],
                           "face_point_stats": fp[2], "outputs_equal": True}
            print(tag, json.dumps(report[tag]), flush=True)
    if args.stage == "grid":
        with open(os.path.join(OUT, "p2m_room_timing.json"), "w") as f:
            json.dump(report, f, indent=1)
        for area in (5e-3, 0.0):
            os.remove(os.path.join(OUT, f"p2m_brute_area{area:g}.pt"))


if __name__ == "__main__":
    main()
