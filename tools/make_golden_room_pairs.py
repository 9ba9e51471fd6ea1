"""Writes tests/golden/room_pairs.npz and tests/golden/room_pairs_options.json from the REFERENCE's own code
(data/processing/utils.py, data/preprocess_batches.py). Runs only where the reference tree is present (tools/ref_import.py).

Third-party modules the reference imports that are not installed where the fixture is made are stubbed, each with the behaviour
the port restates:
    fpsample.bucket_fps_kdline_sampling   returns the centre indices supplied by this tool (its start point is random)
    cuml.neighbors.NearestNeighbors       scikit-learn's class of the same name (exact, fp64)
    pytorch3d.ops.sample_farthest_points  raises: the FPS branch calls .cuda() and cannot run here
    sklearn.neighbors.KDTree              wrapped: query_radius returns every list in ASCENDING index order (the tree's own
                                          order is pinned as a SET by tests/golden/room_radius.npz)
Recorded:
    optimize_assignments on the list sets of tests/pairs_ref.assign_lists (outputs + a CRC-32 of each list set);
    one create_spherical_batches run after np.random.seed(SEED) on a small scene in which every kept patch is padded.
Input condition, asserted before writing: for every query of every kept patch, consecutive neighbour distances up to rank 129
differ by more than 1e-5 relative in fp64 -- so fp32 and fp64 arithmetic agree on the lists. (Clean points that break it are
moved by about a millimetre and the reference is run again; trying seed after seed cannot get there.)
"""
import argparse
import json
import os
import sys
import types
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tools import ref_import  # noqa: E402

import pairs_ref  # noqa: E402

SEED = 42  # the reference's np.random.seed
NPOINTS, RADIUS = 256, 0.55
ASSIGN_SETS = [("random", 256, 8, 300), ("identical", 256, 8, 8), ("identical", 1024, 128, 128), ("shifted", 512, 16, 520),
               ("geometric", 512, 16, 520), ("random", 100, 8, 120), ("random", 4096, 128, 6000)]


def import_reference():
    ref_import.install()
    import sklearn.neighbors as skn

    state = {"centres": None}

    def bucket_fps(points, n, h=5):
        assert len(state["centres"]) == n, (len(state["centres"]), n)
        return np.asarray(state["centres"])

    def no_fps(*a, **kw):
        raise RuntimeError("the FPS branch needs a GPU: the fixture scene must not take it")

    class SortedKDTree(skn.KDTree):
        def query_radius(self, X, r, return_distance=False, **kw):
            out = super().query_radius(X, r=r, return_distance=False)
            return np.array([np.sort(o) for o in out], dtype=object)

    sys.modules["fpsample"] = types.SimpleNamespace(bucket_fps_kdline_sampling=bucket_fps)
    sys.modules["cuml"] = types.ModuleType("cuml")
    sys.modules["cuml.neighbors"] = types.SimpleNamespace(NearestNeighbors=skn.NearestNeighbors)
    sys.modules["pytorch3d"] = types.ModuleType("pytorch3d")
    sys.modules["pytorch3d.ops"] = types.SimpleNamespace(sample_farthest_points=no_fps)
    sys.path.insert(0, os.path.join(ref_import.REF, "data"))
    import processing.utils as utils

    utils.neighbors = types.SimpleNamespace(KDTree=SortedKDTree)
    return utils, state


def parser_defaults():
    """the defaults of the reference parser, read by running its main() up to parse_args"""
    import argparse as ap

    seen = {}
    real = ap.ArgumentParser.parse_args

    class Stop(Exception):
        pass

    def grab(self, *a, **kw):
        seen.update({x.dest: x.default for x in self._actions if x.dest != "help"})
        seen["required"] = sorted(x.dest for x in self._actions if x.required)
        raise Stop

    for name in ("open3d", "tqdm"):
        sys.modules.setdefault(name, types.SimpleNamespace(tqdm=lambda x, **kw: x))
    import preprocess_batches as pb

    ap.ArgumentParser.parse_args = grab
    try:
        pb.main()
    except Stop:
        pass
    finally:
        ap.ArgumentParser.parse_args = real
    return seen


def make_scene(seed):
    """a 2 x 2 x 1 m box shell around the origin: ~7500 clean points, 1536 noisy ones (1500 jittered surface points, a sparse
    cluster whose centre fails the noisy rule, and a cluster away from the mesh whose centre fails the clean rule)"""
    rng = np.random.default_rng(seed)

    def shell(n):
        p = rng.uniform(-1, 1, (n, 3)) * [1.0, 1.0, 0.5]
        ax = rng.integers(0, 3, n)
        p[np.arange(n), ax] = np.sign(p[np.arange(n), ax]) * np.array([1.0, 1.0, 0.5])[ax]
        return p

    clean = shell(7500)
    noisy = shell(1480) + rng.normal(0, 0.01, (1480, 3))
    lonely = np.array([3.0, 0.0, 0.0]) + rng.normal(0, 0.05, (10, 3))  # fewer than npoints // 8 noisy points around
    off_mesh = np.array([0.0, 3.0, 0.0]) + rng.normal(0, 0.1, (46, 3))  # enough noisy points, hardly any clean ones
    clean = np.concatenate([clean, np.array([3.0, 0.0, 0.0]) + rng.normal(0, 0.05, (300, 3))])
    noisy = np.concatenate([noisy, lonely, off_mesh])
    clean, noisy = clean.astype(np.float32), noisy.astype(np.float32)
    rgb_clean = (rng.integers(0, 256, clean.shape) / 255.0).astype(np.float32)
    rgb_noisy = (rng.integers(0, 256, noisy.shape) / 255.0).astype(np.float32)
    feats = rng.normal(0, 1, (len(noisy), 4)).astype(np.float16)
    # centres: exact FPS of the surface part from point 0, then one point of each special cluster
    n_centres = int(np.ceil(len(noisy) / NPOINTS))
    d = np.full(1480, np.inf)
    cen = [0]
    for _ in range(n_centres - 3):
        d = np.minimum(d, ((noisy[:1480].astype(np.float64) - noisy[cen[-1]]) ** 2).sum(1))
        cen.append(int(np.argmax(d)))
    cen += [1480, 1490]
    return clean, noisy, rgb_clean, rgb_noisy, feats, np.array(cen, dtype=np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    utils, state = import_reference()
    out = {}
    for n, (kind, s, k, m) in enumerate(ASSIGN_SETS):
        nn = pairs_ref.assign_lists(kind, s, k, m, seed=n)
        got = utils.optimize_assignments(np.zeros((s, 3)), np.zeros((m, 3)), nn)
        out[f"assign_{n}"] = got.astype(np.int32)
        out[f"assign_{n}_crc"] = np.array(zlib.crc32(np.ascontiguousarray(nn).tobytes()), dtype=np.int64)
    out["assign_sets"] = np.array(json.dumps(ASSIGN_SETS))

    # A random scene never meets the gap condition outright (some 10^5 gaps, each too small with probability ~10^-3), so the
    # offending clean points are nudged by about a millimetre and the reference is run again, until the condition holds.
    clean, noisy, rgb_clean, rgb_noisy, feats, centres = make_scene(0)
    state["centres"] = centres
    rng = np.random.default_rng(1)
    import sklearn.neighbors as skn

    for attempt in range(200):
        np.random.seed(SEED)
        ref_args = ref_import.AttrDict(npoints=NPOINTS, r=RADIUS)
        data = utils.create_spherical_batches(clean.astype(np.float64), noisy.astype(np.float64), rgb_clean.astype(np.float64),
                                              rgb_noisy.astype(np.float64), feats, ref_args)
        assert 3 <= len(data) < len(centres)  # (the scene keeps most patches and skips one by each rule)
        # the lists of every kept patch: the centre's ascending radius lists
        lists = [np.sort(o) for o in skn.KDTree(clean.astype(np.float64)).query_radius(noisy[centres].astype(np.float64), r=RADIUS)]
        lists_n = [np.sort(o) for o in skn.KDTree(noisy.astype(np.float64)).query_radius(noisy[centres].astype(np.float64), r=RADIUS)]
        kept = [c for c in range(len(centres)) if len(lists[c]) >= NPOINTS and len(lists_n[c]) >= NPOINTS // 8]
        assert len(kept) == len(data)
        close = set()
        for c, d in zip(kept, data):
            assert len(lists_n[c]) < NPOINTS, "a kept patch of the fixture must be padded"
            assert np.array_equal(d["idxs"][:len(lists_n[c])], lists_n[c])
            q64 = d["noisy"][:, :3] * d["scale"] + d["center"]
            ref = clean[lists[c]]
            for q in (q64, q64.astype(np.float32)):
                idx, d2 = pairs_ref.knn_brute(q, ref, 129)
                dist = np.sqrt(d2)
                bad = np.diff(dist, axis=1) <= 1e-5 * dist[:, 1:]
                close.update(lists[c][idx[:, 1:][bad]].tolist())
            if not np.array_equal(pairs_ref.knn_brute(q64, ref, 128)[0], pairs_ref.knn_brute(q64.astype(np.float32), ref, 128)[0]):
                close.add(-1)
        if not close:
            break
        print(f"attempt {attempt}: {len(close)} clean points with a neighbour distance too close to the next, nudged")
        close.discard(-1)
        pick = np.array(sorted(close), dtype=np.int64)
        clean[pick] = (clean[pick] + rng.normal(0, 1e-3, (len(pick), 3))).astype(np.float32)
    else:
        raise SystemExit("the distance-gap condition was not reached")
    for c, d in zip(kept, data):  # the condition itself, asserted on what is written
        q64 = d["noisy"][:, :3] * d["scale"] + d["center"]
        assert pairs_ref.knn_gaps_ok(q64, clean[lists[c]], 128), "neighbour distances up to rank 129 must differ by > 1e-5 relative"
    for cloud in (clean, noisy):  # nothing so close to a patch's radius that fp32 and fp64 could disagree on the radius lists
        dist = np.linalg.norm(cloud.astype(np.float64)[None] - noisy[centres].astype(np.float64)[:, None], axis=2)
        assert np.all(np.abs(dist - RADIUS) > 1e-5 * RADIUS), "a point lies on a patch's radius"
    scene_seed = 0
    print(f"{len(data)} of {len(centres)} patches kept after {attempt} rounds of nudging")
    out.update(scene_seed=np.array(scene_seed), seed=np.array(SEED), npoints=np.array(NPOINTS), r=np.array(RADIUS),
               pcd_clean=clean, pcd_noisy=noisy, rgb_clean=rgb_clean, rgb_noisy=rgb_noisy, features=feats, centers_idx=centres,
               n_kept=np.array(len(data)), keys=np.array(json.dumps(sorted(data[0].keys()))))
    for j, d in enumerate(data):
        for key, v in d.items():
            out[f"patch{j}_{key}"] = np.asarray(v)
    os.makedirs(args.out, exist_ok=True)
    np.savez_compressed(os.path.join(args.out, "room_pairs.npz"), **out)
    with open(os.path.join(args.out, "room_pairs_options.json"), "w") as f:
        json.dump(parser_defaults(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", os.path.join(args.out, "room_pairs.npz"), os.path.getsize(os.path.join(args.out, "room_pairs.npz")), "bytes")


if __name__ == "__main__":
    main()
