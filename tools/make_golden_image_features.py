"""tests/golden/image_features.npz: the reference's OWN five functions of data/processing/image_features.py run in the build
container -- `project_point_cloud_batch` (:114-143), `filter_points_batch_with_occlusion` (:146-190),
`map_image_features_to_filtered_ptc_batch_torch` (:223-250), `update_features_batched_torch` (:253-279) and
`interpolate_missing_features` (:282-326) -- on a small synthetic scene; inputs and results only. Environment stand-ins only:
numba's @njit is an identity decorator (the body is plain Python), open3d / torchvision.transforms / loguru / scannetpp are import
stubs (none is called by these five functions), and PYTORCH_JIT=0 makes @torch.jit.script an identity too (scripting the
`ArrayLike` annotations fails; the bodies are plain torch).

The fusion is fed ONE FRAME AT A TIME with features shaped [1, n_valid, C]: that is the per-frame pairing the function's docstring
and the RGB path describe ("Image features", deviations).

The tool asserts the conditions under which an independent fp64 / fp32 implementation has to agree with these results exactly;
with them holding, nothing is excluded from the comparison. If one fails, choose another SEED.
Never run on the GPU box.    python tools/make_golden_image_features.py"""
import os

os.environ["PYTORCH_JIT"] = "0"  # before torch is imported
import importlib  # noqa: E402
import sys  # noqa: E402
import types  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_import  # noqa: E402

SEED = int(sys.argv[1]) if len(sys.argv) > 1 else 5  # (an argument tries another seed; commit the one that passes)
N, FRAMES, BATCH, C = 6000, 6, 2, 8
W, H = 32, 24
K = np.array([[20.0, 0.0, 16.0], [0.0, 20.0, 12.0], [0.0, 0.0, 1.0]])


def stub(name, **kw):
    m = sys.modules.get(name) or types.ModuleType(name)
    m.__dict__.update(kw)
    sys.modules[name] = m
    return m


def njit(*a, **k):
    return a[0] if (len(a) == 1 and callable(a[0]) and not k) else (lambda f: f)


class _Logger:
    def __getattr__(self, k):
        return lambda *a, **kw: None


def load_reference():
    if not ref_import.available():
        raise RuntimeError("reference tree not present at %s" % ref_import.REF)
    sys.dont_write_bytecode = True
    sys.path.insert(1, os.path.join(ref_import.REF, "data"))
    stub("numba", njit=njit)
    stub("open3d")
    stub("torchvision")
    sys.modules["torchvision"].transforms = stub("torchvision.transforms", Compose=object)
    stub("loguru", logger=_Logger())
    stub("scannetpp")
    stub("scannetpp.common")
    stub("scannetpp.common.scene_release", ScannetppScene_Release=object)
    stub("scannetpp.common.utils")
    stub("scannetpp.common.utils.colmap", read_model=None)
    return importlib.import_module("processing.image_features")


def rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]]) @ np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]])
            @ np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def save_npz(path, arrays):
    """np.savez_compressed with a fixed member timestamp: the same arrays give the same bytes on every run"""
    import zipfile

    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as f:
                np.lib.format.write_array(f, np.asanyarray(v), allow_pickle=False)


def main():
    R = load_reference()
    rng = np.random.default_rng(SEED)
    pts32 = np.stack([rng.uniform(-2, 2, N), rng.uniform(-2, 2, N), rng.uniform(0.5, 4, N)], 1).astype(np.float32)
    pts = pts32.astype(np.float64)  # (both sides see identical coordinates)
    rot = np.stack([rotation(*rng.uniform(-0.15, 0.15, 3)) for _ in range(FRAMES)])
    trans = rng.uniform(-0.3, 0.3, (FRAMES, 3))
    cam = np.repeat(K[None], FRAMES, 0)
    maps = rng.standard_normal((FRAMES, H, W, C)).astype(np.float16)

    feats = torch.zeros((N, C), dtype=torch.float16)
    count = torch.zeros((N, 1), dtype=torch.long)
    valid_all = np.zeros((FRAMES, N), dtype=bool)
    proj_all = np.zeros((FRAMES, N, 3))
    for b0 in range(0, FRAMES, BATCH):
        sl = slice(b0, b0 + BATCH)
        B = BATCH
        proj = R.project_point_cloud_batch(np.repeat(pts[None], B, 0), trans[sl][:, :, None], rot[sl], cam[sl].copy())
        valid = R.filter_points_batch_with_occlusion(np.full((B, H, W), np.inf), np.zeros((B, N), dtype=bool), B, N, proj, W, H)
        proj_all[sl], valid_all[sl] = proj, valid
        proj_t, valid_t, maps_t = torch.from_numpy(proj), torch.from_numpy(valid), torch.from_numpy(maps[sl])
        for j in range(B):  # one frame at a time: frame j's rows go to frame j's points
            rows = R.map_image_features_to_filtered_ptc_batch_torch(torch.tensor([], dtype=torch.float16), maps_t[j:j + 1],
                                                                    proj_t[j:j + 1], valid_t[j:j + 1])
            feats, count = R.update_features_batched_torch(feats, count, rows[None], valid_t[j:j + 1])
    mean = feats.numpy().copy()
    cnt = count.numpy()[:, 0].astype(np.int32)
    filled = R.interpolate_missing_features(feats.numpy().copy(), count.numpy(), pts, C)
    np.nan_to_num(filled, copy=False)
    final = filled.astype(np.float16).T  # (what process_scene saves: :511-514)

    # ---- the conditions for exact agreement -----------------------------------------------------------------------------
    xy = proj_all[..., :2]
    near = np.abs(xy - np.round(xy))
    near = near[np.isfinite(near)].min()
    print(f"closest projected coordinate to an integer: {near:.3g} px")
    assert near > 1e-7, "a projected coordinate within 1e-7 px of an integer: choose another SEED"
    gap = np.inf
    for b in range(FRAMES):
        x, y, d = proj_all[b].T
        inb = (x > -1) & (x < W) & (y > -1) & (y < H) & (d > 0.1) & (d < 1000)
        pix = (np.trunc(y[inb]) * W + np.trunc(x[inb])).astype(np.int64)
        o = np.lexsort((d[inb], pix))
        ps, ds = pix[o], d[inb][o]
        same = ps[1:] == ps[:-1]
        if same.any():
            gap = min(gap, ((ds[1:] - ds[:-1])[same] / ds[1:][same]).min())
    print(f"smallest relative gap of two in-range depths of one pixel: {gap:.3g}")
    assert gap > 1e-9, "two depths of one pixel within 1e-9 relative: choose another SEED"
    miss = np.where(cnt == 0)[0]
    kgap = np.inf
    for m0 in range(0, len(miss), 500):
        d2 = ((pts[miss[m0:m0 + 500], None, :] - pts[None, :, :]) ** 2).sum(-1)
        part = np.partition(d2, (9, 10), axis=1)
        kgap = min(kgap, ((part[:, 10] - part[:, 9]) / part[:, 10]).min())
    print(f"smallest relative gap of the 10th and 11th neighbour's squared distance: {kgap:.3g}")
    assert kgap > 1e-5, "10th and 11th neighbour of a missing point within 1e-5 relative: choose another SEED"
    print(f"unobserved: {len(miss)} of {N} ({100.0 * len(miss) / N:.0f} %), counts up to {cnt.max()}, "
          f"rows still zero after the fill: {int((~filled.any(1)).sum())}")

    out = {"points": pts32, "rotation": rot, "translation": trans, "camera": cam, "size": np.array([W, H], dtype=np.int32),
           "maps": maps, "batch": np.array(BATCH, dtype=np.int32), "proj0": proj_all[0], "valid": np.packbits(valid_all, axis=1),
           "mean": mean, "count": cnt, "filled": filled.astype(np.float16), "final": final}
    path = os.path.join(ref_import.ROOT, "tests", "golden", "image_features.npz")
    save_npz(path, out)
    for k, v in out.items():
        print(k, v.shape, v.dtype)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
