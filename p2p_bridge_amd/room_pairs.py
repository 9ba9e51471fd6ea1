"""Room training pairs: a laser mesh and an iPhone scan -> the `points_{i}.npz` patch files that `room_data.ScanNetPP` reads.
The GPU port of the reference's data/preprocess_batches.py and data/processing/utils.py:create_spherical_batches, which run
through Open3D (mesh sampling), fpsample (centres), scikit-learn (radius patches), pytorch3d (FPS), cuML (128 nearest clean
points) and a Python double loop (`optimize_assignments`).

    mesh_cdf, sample_mesh       TriangleMesh.sample_points_uniformly                       csrc/pairs.hip (fp64, searchsorted)
    centres                     fpsample.bucket_fps_kdline_sampling                        csrc/sampling.hip (exact FPS, drawn start)
    radius patches              KDTree.query_radius on both clouds                         denoise_room.radius_query (csrc/room.hip)
    pad / reduce to npoints     numpy global RNG draws / pytorch3d sample_farthest_points  host draws / csrc/sampling.hip from index 0
    patch_knn                   cuml NearestNeighbors(128).kneighbors                      csrc/pairs.hip, one launch per chunk
    unique_assign               optimize_assignments (utils.py:12-40)                      csrc/pairs.hip, deferred acceptance
    finish                      centre, max-norm scale, concatenation (:157-178)           csrc/pairs.hip
    python -m p2p_bridge_amd.room_pairs   preprocess_batches.py:main (scenes one after another; --nprocs is ignored)

Every function takes CUDA tensors and runs kernels; a CPU tensor raises RuntimeError (there is no fallback). No float atomics:
the same inputs and the same numpy seed give the same bytes. Contract of the kernels: include/p2pb_hip.h, "room training pairs";
which edges are pinned to the reference by tests/golden/room_pairs.npz and which are restated: INTEGRATION.md.
"""
import argparse
import math
import os
import zlib

import numpy as np
import torch

from . import pointnet2_batch_cuda as _ext
from ._lib import call, ptr, stream_ptr
from .denoise_room import _fps_from, radius_query
from .evaluate_rooms import _ns, read_ply
from .scan_fusion import _cuda

F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64
KNN_K = 128  # clean candidates per noisy point (utils.py:149)
MAX_K = 128
MAX_PATCHES = 65535  # patches of one p2pb_pairs_knn launch
IDX_BYTES = 256 << 20  # budget of one chunk's neighbour lists idx i32[P,npoints,128]: patches are taken in chunks below it
OVERSAMPLE = 5  # mesh samples per iPhone point (preprocess_batches.py:60)


# ---- mesh ------------------------------------------------------------------------------------------------------------
def mesh_cdf(verts, faces):
    """verts f32[V,3], faces i32[F,3] -> cdf f64[F]: the inclusive prefix sum of the fp64 triangle areas"""
    _cuda(verts, F32, (None, 3), "verts"), _cuda(faces, I32, (None, 3), "faces")
    if verts.shape[0] == 0 or faces.shape[0] == 0:
        raise ValueError("mesh_cdf: empty mesh")
    area = torch.empty(faces.shape[0], dtype=F64, device=verts.device)
    bad = torch.zeros(1, dtype=I32, device=verts.device)
    call("p2pb_pairs_tri_areas", verts.shape[0], faces.shape[0], ptr(verts), ptr(faces), ptr(area), ptr(bad), stream_ptr())
    if int(bad.item()):
        raise ValueError(f"mesh_cdf: a face names a vertex outside [0, {verts.shape[0]})")
    return torch.cumsum(area, 0)


def sample_mesh(verts, faces, u, vcol=None, cdf=None):
    """Uniform points on a triangle mesh (Open3D's sample_points_uniformly, restated): u f64[n,3] in [0,1) from the caller;
    face = searchsorted(cdf, u0 * cdf[-1], side="right"), barycentric weights (1 - s, s (1 - u2), s u2) with s = sqrt(u1), the
    weighted sums in fp64, rounded once. -> (face i32[n], xyz f32[n,3], rgb f32[n,3] | None)"""
    _cuda(verts, F32, (None, 3), "verts"), _cuda(faces, I32, (None, 3), "faces"), _cuda(u, F64, (None, 3), "u")
    if vcol is not None:
        _cuda(vcol, F32, (verts.shape[0], 3), "vcol")
    cdf = mesh_cdf(verts, faces) if cdf is None else cdf
    _cuda(cdf, F64, (faces.shape[0],), "cdf")
    if not float(cdf[-1].item()) > 0.0:
        raise ValueError("sample_mesh: the mesh has no area")
    n, dev = u.shape[0], verts.device
    if n == 0:
        raise ValueError("sample_mesh: no samples asked for")
    face = torch.empty(n, dtype=I32, device=dev)
    xyz = torch.empty(n, 3, dtype=F32, device=dev)
    rgb = torch.empty(n, 3, dtype=F32, device=dev) if vcol is not None else None
    call("p2pb_pairs_sample_mesh", verts.shape[0], faces.shape[0], n, ptr(verts), ptr(vcol), ptr(faces), ptr(cdf),
         ptr(u), ptr(face), ptr(xyz), ptr(rgb), stream_ptr())
    return face, xyz, rgb


# ---- the three patch kernels -----------------------------------------------------------------------------------------
def _offsets(ref_off, npatch, total):
    _cuda(ref_off, I64, (npatch + 1,), "ref_off")
    return int(ref_off[-1].item()) if total is None else int(total)


def patch_knn(query, ref, ref_off, K=KNN_K, return_dist=True):
    """query f32[P,s,3]; ref f32[total,3] = the clean patches one after another, patch p rows ref_off[p]..ref_off[p+1] (i64[P+1])
    -> (idx i32[P,s,K] inside the patch, dist2 f32[P,s,K] | None): the contract and the bits of denoise.knn_points per patch
    (ascending squared distance, ties by ascending index), in one launch and without scratch. 1 <= K <= 128 <= every patch."""
    _cuda(query, F32, (None, None, 3), "query"), _cuda(ref, F32, (None, 3), "ref")
    p, s, k = query.shape[0], query.shape[1], int(K)
    _cuda(ref_off, I64, (p + 1,), "ref_off")
    if not 1 <= k <= MAX_K:
        raise ValueError(f"patch_knn: K={k} must be in [1, {MAX_K}]")
    if p == 0 or s == 0 or ref.shape[0] == 0:
        raise ValueError("patch_knn: empty batch")
    idx = torch.empty(p, s, k, dtype=I32, device=query.device)
    dist2 = torch.empty(p, s, k, dtype=F32, device=query.device) if return_dist else None
    call("p2pb_pairs_knn", p, s, k, ref.shape[0], ptr(query), ptr(ref), ptr(ref_off), ptr(idx), ptr(dist2), stream_ptr())
    return idx, dist2


def unique_assign(nn, ref_off, total=None):
    """optimize_assignments for a batch of patches: nn i32[P,s,K] -> (assign i32[P,s], unique i32[P]). Point i (ascending)
    takes the first entry of nn[p,i] no earlier point took, else nn[p,i,0]; unique = distinct values per patch."""
    _cuda(nn, I32, (None, None, None), "nn")
    p, s, k = nn.shape
    if not 1 <= k <= MAX_K or p == 0 or s == 0:
        raise ValueError(f"unique_assign: nn {list(nn.shape)} must be [P >= 1, s >= 1, 1 <= K <= {MAX_K}]")
    total = _offsets(ref_off, p, total)
    if total <= 0:
        raise ValueError("unique_assign: empty clean patches")
    owner = torch.empty(total, dtype=I32, device=nn.device)
    assign = torch.empty(p, s, dtype=I32, device=nn.device)
    unique = torch.empty(p, dtype=I32, device=nn.device)
    call("p2pb_pairs_unique_assign", p, s, k, total, ptr(nn), ptr(ref_off), ptr(owner), ptr(assign), ptr(unique),
         stream_ptr())
    return assign, unique


def finish(noisy, noisy_rgb, ref, ref_rgb, ref_off, assign):
    """centre (fp64 sum in index order / s, rounded), scale (largest fp32 norm of the centred noisy points), and the output
    rows: -> (clean f32[P,s,6] = ((ref[assign] - centre) / scale, ref_rgb[assign]), noisy f32[P,s,6], center f32[P,3],
    scale f32[P])"""
    _cuda(noisy, F32, (None, None, 3), "noisy")
    p, s = noisy.shape[:2]
    _cuda(noisy_rgb, F32, (p, s, 3), "noisy_rgb"), _cuda(ref, F32, (None, 3), "ref")
    _cuda(ref_rgb, F32, (ref.shape[0], 3), "ref_rgb"), _cuda(ref_off, I64, (p + 1,), "ref_off"), _cuda(assign, I32, (p, s), "assign")
    if p == 0 or s == 0 or ref.shape[0] == 0:
        raise ValueError("finish: empty batch")
    dev = noisy.device
    clean_out = torch.empty(p, s, 6, dtype=F32, device=dev)
    noisy_out = torch.empty(p, s, 6, dtype=F32, device=dev)
    center = torch.empty(p, 3, dtype=F32, device=dev)
    scale = torch.empty(p, dtype=F32, device=dev)
    call("p2pb_pairs_finish", p, s, ref.shape[0], ptr(noisy), ptr(noisy_rgb), ptr(ref), ptr(ref_rgb), ptr(ref_off),
         ptr(assign), ptr(clean_out), ptr(noisy_out), ptr(center), ptr(scale), stream_ptr())
    return clean_out, noisy_out, center, scale


# ---- host logic (no device: tests/test_room_pairs.py) ----------------------------------------------------------------
def plan_patches(clean_counts, noisy_counts, npoints):
    """the skip rules of utils.py:117-125 -> (kept centre numbers, skipped): a patch needs npoints clean points and
    npoints // 8 noisy ones"""
    kept = [c for c in range(len(noisy_counts)) if clean_counts[c] >= npoints and noisy_counts[c] >= npoints // 8]
    return kept, len(noisy_counts) - len(kept)


def pad_draws(patch_xyz, npoints):
    """utils.py:131-140 for a noisy patch of L < npoints points (f32[L,3], host): the reference's two draws in its order from
    numpy's GLOBAL generator -- randint(0, L, diff), then normal(0, 1e-2 * diagonal, (diff, 3)) with the bounding-box diagonal
    in fp64 -- and the duplicates + jitter added in fp64, rounded to fp32 once. -> (rand_idx i64[diff], extra f32[diff,3])"""
    patch_xyz = np.asarray(patch_xyz)
    L = patch_xyz.shape[0]
    diff = npoints - L
    rand_idx = np.random.randint(0, L, diff)
    p64 = patch_xyz.astype(np.float64)
    diagonal = np.linalg.norm(np.max(p64, axis=0) - np.min(p64, axis=0))
    jitter = np.random.normal(0, 1e-2 * diagonal, (diff, 3))
    return rand_idx.astype(np.int64), (p64[rand_idx] + jitter).astype(np.float32)


def chunk_patches(npatch, npoints, k, budget):
    """[lo, hi) runs of patches whose neighbour lists idx i32[hi - lo, npoints, k] stay under `budget` bytes, and which one
    p2pb_pairs_knn launch takes (at most MAX_PATCHES)"""
    step = min(MAX_PATCHES, max(1, budget // (npoints * k * 4)))
    return [(lo, min(npatch, lo + step)) for lo in range(0, npatch, step)]


# ---- the scene -------------------------------------------------------------------------------------------------------
@torch.no_grad()
def create_spherical_batches(pcd_clean, pcd_noisy, rgb_clean, rgb_noisy, features, args, centers_idx=None, trace=None):
    """utils.py:64-226. pcd_clean f32[Nc,3], pcd_noisy f32[Nn,3], rgb_* f32[*,3] (CUDA), features [Nn,C] (tensor or numpy) or
    None; args.npoints, args.r. centers_idx (i64[n_batches]) overrides the FPS centres, which otherwise start at an index drawn
    with np.random.randint. Random draws come from numpy's global generator in the reference's order (seed it: the reference
    runs np.random.seed(42)). trace is a hook of the tests, not part of the reference's signature: a dict that receives the
    intermediate results of every stage (device tensors of every chunk, which stay alive as long as the dict does).
    -> (list of dicts {clean f32[npoints,6], noisy f32[npoints,6], idxs i64[npoints], features f16 (if given), center f32[3],
    scale f32 scalar}, (skipped, mean unique fraction, mean noisy count))"""
    _cuda(pcd_clean, F32, (None, 3), "pcd_clean"), _cuda(pcd_noisy, F32, (None, 3), "pcd_noisy")
    _cuda(rgb_clean, F32, (pcd_clean.shape[0], 3), "rgb_clean"), _cuda(rgb_noisy, F32, (pcd_noisy.shape[0], 3), "rgb_noisy")
    npoints, r = int(_ns(args, "npoints")), float(_ns(args, "r"))
    if npoints < 8:
        raise ValueError(f"create_spherical_batches: npoints={npoints} must be at least 8")
    dev, nn_pts = pcd_noisy.device, pcd_noisy.shape[0]
    if features is not None and features.shape[0] != nn_pts:
        raise ValueError(f"create_spherical_batches: {nn_pts} points but {features.shape[0]} features")
    k = min(KNN_K, npoints)  # (a kept patch has at least npoints clean points)
    n_batches = int(math.ceil(nn_pts / npoints))
    if centers_idx is None:
        centers_idx = _fps_from(pcd_noisy, n_batches, int(np.random.randint(0, nn_pts)))
    else:
        centers_idx = torch.as_tensor(centers_idx).long().to(dev)
        n_batches = centers_idx.numel()
    centres = pcd_noisy[centers_idx].contiguous()
    idx_clean, off_clean = radius_query(centres, pcd_clean, r)
    idx_noisy, off_noisy = radius_query(centres, pcd_noisy, r)
    oc, on = off_clean.cpu().numpy(), off_noisy.cpu().numpy()
    kept, skipped = plan_patches(np.diff(oc), np.diff(on), npoints)
    stats_noisy = float(sum(int(on[c + 1] - on[c]) for c in kept))
    if trace is not None:
        trace.update(centers_idx=centers_idx, off_clean=oc, off_noisy=on, idx_clean=idx_clean, idx_noisy=idx_noisy, kept=kept,
                     branch=[], chunks=[])
    if not kept:
        return [], (skipped, float("nan"), stats_noisy / max(n_batches, 1))

    # the noisy patches, brought to npoints: padded (host draws, in patch order) or reduced by exact FPS from index 0
    host_xyz, host_idx = pcd_noisy.cpu().numpy(), idx_noisy.cpu().numpy()
    rows, sels = [], []
    for c in kept:
        m_host = host_idx[on[c]:on[c + 1]].astype(np.int64)
        m = idx_noisy[on[c]:on[c + 1]].long()
        p = pcd_noisy[m]
        if len(m_host) < npoints:
            rand_idx, extra = pad_draws(host_xyz[m_host], npoints)
            rows.append(torch.cat([p, torch.from_numpy(extra).to(dev)], 0))
            sels.append(torch.cat([m, m[torch.from_numpy(rand_idx).to(dev)]]))
        else:  # (at equality too, like the reference)
            f = _ext.furthest_point_sampling_forward(p.t().contiguous()[None], npoints)[0].long()
            rows.append(p[f])
            sels.append(m[f])
        if trace is not None:
            trace["branch"].append("pad" if len(m_host) < npoints else "fps")
    query = torch.stack(rows).contiguous()
    sel = torch.stack(sels)
    query_rgb = rgb_noisy[sel].contiguous()

    outs = []
    for lo, hi in chunk_patches(len(kept), npoints, k, IDX_BYTES):
        counts = [int(oc[c + 1] - oc[c]) for c in kept[lo:hi]]
        ref_idx = torch.cat([idx_clean[oc[c]:oc[c + 1]] for c in kept[lo:hi]]).long()
        ref, ref_rgb = pcd_clean[ref_idx].contiguous(), rgb_clean[ref_idx].contiguous()
        ref_off = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)).to(dev)
        nn, _ = patch_knn(query[lo:hi], ref, ref_off, k, return_dist=False)
        assign, unique = unique_assign(nn, ref_off, total=ref.shape[0])
        clean_out, noisy_out, center, scale = finish(query[lo:hi], query_rgb[lo:hi], ref, ref_rgb, ref_off, assign)
        outs.append((clean_out.cpu(), noisy_out.cpu(), center.cpu(), scale.cpu(), unique.cpu()))
        if trace is not None:
            trace["chunks"].append(dict(lo=lo, hi=hi, ref=ref, ref_rgb=ref_rgb, ref_idx=ref_idx, ref_off=ref_off, nn=nn,
                                        assign=assign, unique=unique, query=query[lo:hi], query_rgb=query_rgb[lo:hi],
                                        clean=clean_out, noisy=noisy_out, center=center, scale=scale))
    clean_all, noisy_all, center_all, scale_all, unique_all = (torch.cat([o[j] for o in outs]).numpy() for j in range(5))
    sel_host = sel.cpu().numpy()
    data = []
    for j in range(len(kept)):
        d = {"clean": clean_all[j], "noisy": noisy_all[j], "idxs": sel_host[j]}
        if features is not None:
            f = features[sel[j].to(features.device)] if isinstance(features, torch.Tensor) else np.asarray(features)[sel_host[j]]
            d["features"] = (f.cpu().numpy() if isinstance(f, torch.Tensor) else f).astype(np.float16)
        d["center"], d["scale"] = center_all[j], scale_all[j]
        data.append(d)
    return data, (skipped, float(np.mean(unique_all / float(npoints))), stats_noisy / n_batches)


def handle_scene(scene, args, log=print):
    """preprocess_batches.py:26-91 for one scene folder: scans/mesh_aligned_0.05.ply (vertex colours needed) and
    scans/iphone{suffix}.ply -> output_root/scene/points_{i}.npz. The 5 N mesh samples take their uniforms from a torch CPU
    generator seeded with the CRC-32 of the scene's name. -> number of files written, None when the scene is skipped."""
    root, suffix = _ns(args, "data_root"), _ns(args, "name_suffix", "") or ""
    mesh_path = os.path.join(root, scene, "scans", "mesh_aligned_0.05.ply")
    scan_path = os.path.join(root, scene, "scans", f"iphone{suffix}.ply")
    if not os.path.exists(mesh_path) or not os.path.exists(scan_path):
        log(f"Skipping {scene} because of missing scans")
        return None
    features, ftype = None, _ns(args, "feature_type")
    if ftype is not None:
        fpath = os.path.join(root, scene, "features", f"{ftype}_iphone{suffix}.npy")
        if not os.path.exists(fpath):
            log(f"Skipping {scene} because of missing features")
            return None
        features = np.load(fpath).T
    scan, mesh = read_ply(scan_path, colors=True), read_ply(mesh_path, colors=True)
    for what, d in (("iphone scan", scan), ("mesh", mesh)):
        if d["colors"] is None:
            raise ValueError(f"{scene}: the {what} has no vertex colours")
    if mesh["faces"] is None or len(mesh["faces"]) == 0:
        raise ValueError(f"{scene}: {mesh_path} has no faces")
    n = scan["points"].shape[0]
    if features is not None and features.shape[0] != n:
        log(f"Scene {scene} has {n} points but {features.shape[0]} features")
        return None
    dev = "cuda"
    xyz_noisy = torch.from_numpy(scan["points"]).float().to(dev)
    rgb_noisy = torch.from_numpy(scan["colors"]).float().to(dev)
    verts = torch.from_numpy(mesh["points"]).float().to(dev)
    vcol = torch.from_numpy(mesh["colors"]).float().to(dev)
    faces = torch.from_numpy(mesh["faces"]).int().to(dev)
    gen = torch.Generator().manual_seed(zlib.crc32(scene.encode()))
    u = torch.rand(OVERSAMPLE * n, 3, dtype=F64, generator=gen).to(dev)
    _, xyz_clean, rgb_clean = sample_mesh(verts, faces, u, vcol)
    batches, (skipped, uniq, avg) = create_spherical_batches(xyz_clean, xyz_noisy, rgb_clean, rgb_noisy, features, args)
    log(f"{scene}: skipped {skipped} batches, unique assignments {uniq:.4f}, average noisy points {avg:.1f}")
    target = os.path.join(_ns(args, "output_root"), scene)
    os.makedirs(target, exist_ok=True)
    for j, b in enumerate(batches):
        np.savez(os.path.join(target, f"points_{j}.npz"), **b)
    return len(batches)


def build_parser():
    ap = argparse.ArgumentParser(description="ScanNet++ scenes -> (noisy, clean) training patches")
    ap.add_argument("--data_root", type=str, required=True, help="Path to the data directory.")
    ap.add_argument("--name_suffix", type=str, default="", help="Suffix to append to the name of the points and features.")
    ap.add_argument("--output_root", type=str, required=True, help="Path to the target directory.")
    ap.add_argument("--npoints", type=int, default=4096, help="Number of points per patch.")
    ap.add_argument("--r", type=float, default=0.3, help="Radius for the spherical batches.")
    ap.add_argument("--feature_type", type=str, default="dino", help="Features to use.")
    ap.add_argument("--nprocs", type=int, default=4, help="Accepted and ignored: scenes run one after another.")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    torch.manual_seed(42)
    np.random.seed(42)
    scenes = sorted(f for f in os.listdir(args.data_root) if os.path.isdir(os.path.join(args.data_root, f)))
    for scene in scenes:
        handle_scene(scene, args)


if __name__ == "__main__":
    main()
