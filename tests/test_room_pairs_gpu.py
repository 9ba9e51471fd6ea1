"""Room training pairs on the GPU (csrc/pairs.hip, p2p_bridge_amd/room_pairs.py) against the numpy restatements of
tests/pairs_ref.py, the existing p2pb_knn_points, and the reference's recorded run (tests/golden/room_pairs.npz).
Integer results (assignment, neighbour indices, faces, idxs) are held exactly; floating-point bounds are derived where used."""
import json
import os

import numpy as np
import pytest
import torch

import pairs_ref
from oracle.poison_arena import PoisonArena
from p2p_bridge_amd import denoise, room_data, scan_fusion
from p2p_bridge_amd import room_pairs as RP

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -23


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: shared arrays stay untouched)


def host(t):
    return t.cpu().numpy()


def offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


# ---- assignment ------------------------------------------------------------------------------------------------------
ASSIGN_CASES = [("random", 256, 8, 300), ("identical", 256, 8, 8), ("identical", 1024, 128, 128), ("shifted", 512, 16, 520),
                ("geometric", 512, 16, 520), ("random", 100, 8, 120), ("random", 4096, 128, 6000)]


@pytest.mark.parametrize("n", range(len(ASSIGN_CASES)))
def test_unique_assign_equals_the_sequential_rule(n):
    kind, s, k, m = ASSIGN_CASES[n]
    nn = pairs_ref.assign_lists(kind, s, k, m, seed=n)
    assign, unique = RP.unique_assign(dev(nn[None]), dev(offsets([m])))
    want = pairs_ref.sequential_assign(nn)
    assert assign.dtype == torch.int32 and assign.shape == (1, s)
    assert np.array_equal(host(assign)[0], want)
    assert int(unique[0]) == len(np.unique(want))
    if kind == "identical":  # K points take the K entries, everybody else falls back to entry 0
        assert int((want == 0).sum()) == 1 + s - k and int(unique[0]) == k


def test_unique_assign_ragged_batch():
    """three patches of different sizes in one launch, one of exactly K points: wrong if ref_off is ignored"""
    rng = np.random.default_rng(5)
    s, k, ms = 64, 8, (8, 50, 20)
    nn = np.stack([np.stack([rng.permutation(m)[:k] for _ in range(s)]) for m in ms]).astype(np.int32)
    assign, unique = RP.unique_assign(dev(nn), dev(offsets(ms)))
    for p in range(3):
        want = pairs_ref.sequential_assign(nn[p])
        assert np.array_equal(host(assign)[p], want), p
        assert int(unique[p]) == len(np.unique(want))
    # entries outside the patch count as taken; offsets beyond the workspace are refused
    bad = nn.copy()
    bad[1, ::2, 0] = 50
    taken, want, holders = {50}, [], 0
    for row in bad[1]:
        free = [int(t) for t in row if int(t) not in taken]
        want.append(free[0] if free else int(row[0]))
        taken.update(free[:1])
        holders += bool(free)
    assign, unique = RP.unique_assign(dev(bad), dev(offsets(ms)))
    assert np.array_equal(host(assign)[1], want)
    # unique counts the points that took an entry; the fall-backs to entry 50, which nobody can take, add a value it leaves out
    assert 50 in want and int(unique[1]) == holders == len(np.unique(want)) - 1
    with pytest.raises(RuntimeError):
        RP.unique_assign(dev(nn), dev(offsets(ms)), total=70)


# ---- k-NN ------------------------------------------------------------------------------------------------------------
def _knn_per_patch(query, refs, k):
    """p2pb_knn_points, one call per patch -> (idx i64[P,s,k], dist2 f32[P,s,k])"""
    out = [denoise.knn_points(dev(query[p][None]), dev(refs[p][None]), K=k) for p in range(len(refs))]
    return np.concatenate([host(o.idx) for o in out]), np.concatenate([host(o.dists) for o in out])


def _check_knn(query, refs, k, restated=True):
    ref_off = offsets([len(r) for r in refs])
    idx, d2 = RP.patch_knn(dev(query), dev(np.concatenate(refs)), dev(ref_off), K=k)
    want_idx, want_d2 = _knn_per_patch(query, refs, k)
    assert idx.dtype == torch.int32 and idx.shape == (len(refs), query.shape[1], k)
    assert np.array_equal(host(idx), want_idx)
    assert np.array_equal(host(d2).view(np.uint32), want_d2.view(np.uint32))  # the same bits
    assert torch.equal(RP.patch_knn(dev(query), dev(np.concatenate(refs)), dev(ref_off), K=k, return_dist=False)[0], idx)
    if restated:  # queries whose fp64 neighbour distances are well apart: fp32 and fp64 give the same list
        for p, r in enumerate(refs):
            kk = min(k + 1, len(r))
            d = np.sqrt(pairs_ref.knn_brute(query[p], r, kk)[1])
            clear = np.all(np.diff(d, axis=1) > 1e-5 * d[:, 1:], axis=1)
            assert clear.sum() > len(clear) // 2
            assert np.array_equal(host(idx)[p][clear], pairs_ref.knn_brute(query[p], r, k)[0][clear])


@pytest.fixture(scope="module")
def clouds():
    rng = np.random.default_rng(11)
    refs = [rng.uniform(-1, 1, (m, 3)).astype(np.float32) for m in (128, 1000, 5000)]  # K itself, one tile, five tiles
    query = rng.uniform(-1, 1, (3, 256, 3)).astype(np.float32)
    for a in refs + [query]:
        a.setflags(write=False)
    return query, refs


@pytest.mark.parametrize("k", [1, 16, 128])
def test_patch_knn_equals_knn_points_per_patch(clouds, k):
    _check_knn(clouds[0], clouds[1], k)


def test_patch_knn_ties_and_offsets(clouds):
    rng = np.random.default_rng(12)
    g = np.arange(8, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)  # many exactly equal distances
    q = np.concatenate([lattice[rng.integers(0, 512, 100)], rng.integers(0, 8, (30, 3)).astype(np.float32) + 0.5])
    _check_knn(q[None], [lattice], 33, restated=False)
    base = clouds[1][1]
    dup = np.concatenate([base[:700], base[:700][rng.integers(0, 700, 600)]])  # duplicated reference points
    _check_knn(clouds[0][:1], [dup], 64, restated=False)
    _check_knn(base[None, :259], [base], 16, restated=False)  # queries that are reference points; s % 4 == 3
    _check_knn(clouds[0] + np.float32(50), [r + np.float32(50) for r in clouds[1]], 128, restated=False)  # the scene shifted


@pytest.mark.parametrize("k", [64, 65])
def test_patch_knn_at_the_second_register_of_the_list(k):
    """K = 65 is the first list whose last rank, and with it tau, lives in the second register of a lane; K = 64 on the same
    input is the last that does not. Patches of 70 points (barely above K) and 1100 (one crossing of the 1024-point LDS
    tile); 5 queries: the second workgroup has three idle waves."""
    rng = np.random.default_rng(13)
    refs = [rng.uniform(-1, 1, (m, 3)).astype(np.float32) for m in (70, 1100)]
    _check_knn(rng.uniform(-1, 1, (2, 5, 3)).astype(np.float32), refs, k, restated=False)


def test_patch_knn_refuses_a_patch_smaller_than_k(clouds):
    query, refs = clouds
    with pytest.raises(ValueError):
        RP.patch_knn(dev(query), dev(np.concatenate(refs)), dev(offsets([128, 1000, 5000])), K=129)
    with pytest.raises(RuntimeError):
        RP.patch_knn(dev(query), dev(np.concatenate(refs)), dev(offsets([100, 1028, 5000])), K=128)
    with pytest.raises(RuntimeError):  # offsets beyond the cloud
        RP.patch_knn(dev(query), dev(np.concatenate(refs)), dev(offsets([128, 1000, 5001])), K=16)


# ---- mesh ------------------------------------------------------------------------------------------------------------
def _square_mesh():
    verts = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [2, 0, 0], [2.002, 0, 0], [2, 0.001, 0]], dtype=np.float32)
    faces = np.array([[0, 1, 2], [0, 1, 1], [0, 2, 3], [4, 5, 6]], dtype=np.int32)  # unit square, a zero-area one between, 1e-6
    vcol = np.random.default_rng(3).uniform(0, 1, (7, 3)).astype(np.float32)
    return verts, faces, vcol


def test_sample_mesh():
    verts, faces, vcol = _square_mesh()
    cdf_dev = RP.mesh_cdf(dev(verts), dev(faces))
    cdf = host(cdf_dev)
    want_cdf = np.cumsum(pairs_ref.tri_areas(verts, faces))
    assert cdf[0] == 0.5 and cdf[1] == 0.5 and cdf[2] == 1.0 and abs(cdf[3] - 1.0 - 1e-6) < 1e-9
    assert np.allclose(cdf, want_cdf, rtol=1e-15, atol=0)
    n, total = 4096, cdf[-1]
    u = np.random.default_rng(4).uniform(0, 1, (n, 3))
    u[0, 0], u[1, 0] = 0.0, np.nextafter(1.0, 0.0)
    row = 2
    for b in (cdf[0], cdf[2]):  # u0 with u0 * total exactly on a boundary of the cdf
        cand = b / total
        hits = [x for x in (np.nextafter(cand, 0), cand, np.nextafter(cand, 1)) if x * total == b]
        assert hits, "no uniform lands exactly on this boundary"
        for x in hits:
            u[row, 0] = x
            row += 1
    u[row:row + 3, 1] = (0.0, 1.0, np.nextafter(1.0, 0.0))  # the corners of the weights
    face, xyz, rgb = RP.sample_mesh(dev(verts), dev(faces), dev(u), dev(vcol), cdf=cdf_dev)
    wf, wx, wc = pairs_ref.sample_mesh(verts, faces, cdf, u, vcol)
    face = host(face)
    assert np.array_equal(face, wf)
    assert face[0] == 0 and face[1] == 3 and face[2] == 2 and not np.any(face == 1)  # (row 2: on cdf[0] = cdf[1] -> face 2)
    # one final rounding, plus the freedom the order of the fp64 sum leaves: 2^-23 of the triangle's largest value
    for got, want, values in ((host(xyz), wx, verts), (host(rgb), wc, vcol)):
        bound = EPS * np.abs(values[faces[face]]).max(axis=(1, 2))
        assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float32).astype(np.float64)) <= bound[:, None])
    f2, x2, none = RP.sample_mesh(dev(verts), dev(faces), dev(u))  # the cdf computed inside, no colours
    assert none is None and np.array_equal(host(f2), face) and torch.equal(x2, xyz)
    with pytest.raises(ValueError):
        RP.mesh_cdf(dev(verts), dev(np.array([[0, 1, 7]], dtype=np.int32)))


# ---- finish ----------------------------------------------------------------------------------------------------------
def _check_finish(noisy, noisy_rgb, clean_sel, clean_rgb_sel, got_clean, got_noisy, center, scale, extra=0.0):
    """one patch against the fp64 restatement made from the same selections. Bounds (include/p2pb_hip.h): the centre is the
    fp64 mean rounded once: half an ulp. A normalised coordinate carries the centre's rounding seen through the division,
    ulp32(max |centre|) / scale, plus the subtraction's and the division's own roundings and the scale's, 2^-22 together."""
    wn, wc, c64, s64 = pairs_ref.normalise_fp64(noisy, clean_sel)
    assert np.array_equal(center, c64.astype(np.float32))
    assert np.all(np.abs(center.astype(np.float64) - c64) <= 0.5 * pairs_ref.ulp32(c64))
    bound = pairs_ref.ulp32(np.abs(center).max()) / s64 + 2.0 ** -22 + extra
    # (the scale: the centre's rounding moves every centred point by less than ulp32(max |centre|), then two roundings)
    assert abs(float(scale) - s64) <= pairs_ref.ulp32(np.abs(center).max()) + 2.0 ** -22 * s64
    assert np.abs(got_noisy[:, :3] - wn).max() <= bound and np.abs(got_clean[:, :3] - wc).max() <= bound
    assert np.array_equal(got_noisy[:, 3:], noisy_rgb) and np.array_equal(got_clean[:, 3:], clean_rgb_sel)
    assert abs(np.linalg.norm(got_noisy[:, :3].astype(np.float64), axis=1).max() - 1.0) <= EPS


def test_finish():
    rng = np.random.default_rng(6)
    s, ms = 1000, (1500, 1200)
    mids = np.array([[8.0, -6.0, 1.5], [0.0, 0.0, 0.0]])
    noisy = np.stack([(c + rng.normal(0, 0.15, (s, 3))).astype(np.float32) for c in mids])
    ref = np.concatenate([(c + rng.normal(0, 0.15, (m, 3))).astype(np.float32) for c, m in zip(mids, ms)])
    noisy_rgb, ref_rgb = rng.uniform(0, 1, (2, s, 3)).astype(np.float32), rng.uniform(0, 1, (sum(ms), 3)).astype(np.float32)
    assign = np.stack([rng.integers(0, m, s) for m in ms]).astype(np.int32)
    off = offsets(ms)
    clean, nz, center, scale = RP.finish(dev(noisy), dev(noisy_rgb), dev(ref), dev(ref_rgb), dev(off), dev(assign))
    assert clean.shape == (2, s, 6) and nz.shape == (2, s, 6) and center.shape == (2, 3) and scale.shape == (2,)
    for p in range(2):
        rows = off[p] + assign[p]
        _check_finish(noisy[p], noisy_rgb[p], ref[rows], ref_rgb[rows], host(clean)[p], host(nz)[p], host(center)[p],
                      host(scale)[p])
    assign[1, 5] = ms[1]  # an assignment outside the patch: a loud row, nothing read
    out = host(RP.finish(dev(noisy), dev(noisy_rgb), dev(ref), dev(ref_rgb), dev(off), dev(assign))[0])
    assert np.all(np.isnan(out[1, 5])) and not np.any(np.isnan(np.delete(out[1], 5, axis=0)))


# ---- end to end ------------------------------------------------------------------------------------------------------
E2E_NPOINTS, E2E_R = 1024, 0.6


def _room_mesh():
    """a 4 x 3 x 2.5 m box and a detached 2 x 2 m plate -> verts f32[12,3], faces i32[14,3], vcol f32[12,3]"""
    x, y, z = 4.0, 3.0, 2.5
    box = np.array([[0, 0, 0], [x, 0, 0], [x, y, 0], [0, y, 0], [0, 0, z], [x, 0, z], [x, y, z], [0, y, z]])
    quads = [(0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 5, 4), (1, 2, 6, 5), (2, 3, 7, 6), (3, 0, 4, 7)]
    plate = np.array([[-7, 0, 0], [-5, 0, 0], [-5, 2, 0], [-7, 2, 0]])
    faces = [t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))] + [(8, 9, 10), (8, 10, 11)]
    verts = np.concatenate([box, plate]).astype(np.float32)
    vcol = (np.random.default_rng(20).integers(0, 256, verts.shape) / 255.0).astype(np.float32)
    return verts, np.array(faces, dtype=np.int32), vcol


def _room_scan(n=20000):
    """the noisy scan: a dense floor region (patches of >= npoints: the FPS branch), thin walls (padding), a few points in the
    middle of the plate (clean points enough, noisy too few) and a blob away from the mesh (no clean points)"""
    rng = np.random.default_rng(21)
    verts, faces, _ = _room_mesh()
    cdf = np.cumsum(pairs_ref.tri_areas(verts, faces[:12]))
    _, shell, _ = pairs_ref.sample_mesh(verts, faces[:12], cdf, rng.uniform(0, 1, (n - 9320, 3)))
    dense = np.stack([rng.uniform(0.6, 3.4, 9000), rng.uniform(0.3, 2.7, 9000), np.zeros(9000)], 1)
    plate = np.stack([rng.uniform(-6.2, -5.8, 20), rng.uniform(0.8, 1.2, 20), np.zeros(20)], 1)
    blob = np.array([10.0, 0.0, 1.0]) + rng.normal(0, 0.05, (300, 3))
    pts = np.concatenate([shell + rng.normal(0, 0.01, shell.shape), dense + rng.normal(0, 0.01, dense.shape), plate, blob])
    rgb = rng.integers(0, 256, pts.shape).astype(np.uint8)
    return pts.astype(np.float32), rgb


@pytest.fixture(scope="module")
def room():
    verts, faces, vcol = _room_mesh()
    noisy, rgb8 = _room_scan()
    u = np.random.default_rng(22).uniform(0, 1, (5 * len(noisy), 3))
    _, clean, clean_rgb = RP.sample_mesh(dev(verts), dev(faces), dev(u), dev(vcol))
    feats = np.random.default_rng(23).normal(0, 1, (len(noisy), 8)).astype(np.float32)
    trace = {}
    np.random.seed(42)
    args = {"npoints": E2E_NPOINTS, "r": E2E_R}
    data, stats = RP.create_spherical_batches(clean, dev(noisy), clean_rgb, dev(rgb8 / np.float32(255)), feats, args, trace=trace)
    return dict(noisy=noisy, rgb=(rgb8 / np.float32(255)).astype(np.float32), rgb8=rgb8, clean=host(clean),
                clean_rgb=host(clean_rgb), feats=feats, data=data, stats=stats, trace=trace, args=args)


def test_end_to_end_stages(room):
    tr, data, s = room["trace"], room["data"], E2E_NPOINTS
    oc, on, kept = tr["off_clean"], tr["off_noisy"], tr["kept"]
    nc, nn_ = np.diff(oc), np.diff(on)
    assert len(nc) == -(-len(room["noisy"]) // s)
    # every branch and both skip rules occur
    assert "pad" in tr["branch"] and "fps" in tr["branch"]
    assert np.any(nc < s) and np.any((nc >= s) & (nn_ < s // 8))
    assert kept == [c for c in range(len(nc)) if nc[c] >= s and nn_[c] >= s // 8] and len(data) == len(kept)
    skipped, uniq, avg = room["stats"]
    assert skipped == len(nc) - len(kept) and 0 < uniq <= 1 and avg == sum(nn_[c] for c in kept) / len(nc)
    # the centres: exact FPS from the drawn start
    np.random.seed(42)
    start = np.random.randint(0, len(room["noisy"]))
    cen = host(tr["centers_idx"])
    assert cen[0] == start and len(set(cen.tolist())) == len(cen)
    d = np.full(len(room["noisy"]), np.inf)
    for a, b in zip(cen[:5], cen[1:6]):
        d = np.minimum(d, ((room["noisy"].astype(np.float64) - room["noisy"][a]) ** 2).sum(1))
        assert d[b] >= d.max() * (1 - 1e-6)
    (ch,) = tr["chunks"]
    assert (ch["lo"], ch["hi"]) == (0, len(kept))
    ref, ref_off, query = host(ch["ref"]), host(ch["ref_off"]), host(ch["query"])
    nn, assign, idxs = host(ch["nn"]), host(ch["assign"]), np.stack([d_["idxs"] for d_ in data])
    ref_rows = host(ch["ref_idx"])
    assert np.array_equal(ref, room["clean"][ref_rows]) and np.array_equal(np.diff(ref_off), [nc[c] for c in kept])
    want_idx, _ = _knn_per_patch(query, [ref[ref_off[p]:ref_off[p + 1]] for p in range(len(kept))], 128)
    assert np.array_equal(nn, want_idx)  # stage by stage: each restatement is fed the device output of the stage before
    for p in (tr["branch"].index("pad"), tr["branch"].index("fps")):
        r = ref[ref_off[p]:ref_off[p + 1]]
        dist = np.sqrt(pairs_ref.knn_brute(query[p], r, 129)[1])
        clear = np.all(np.diff(dist, axis=1) > 1e-5 * dist[:, 1:], axis=1)
        assert clear.sum() > s // 2 and np.array_equal(nn[p][clear], pairs_ref.knn_brute(query[p], r, 128)[0][clear])
    for p, c in enumerate(kept):
        want = pairs_ref.sequential_assign(nn[p])
        assert np.array_equal(assign[p], want) and int(ch["unique"][p]) == len(np.unique(want))
        rows = ref_off[p] + assign[p]
        _check_finish(query[p], room["rgb"][idxs[p]], ref[rows], host(ch["ref_rgb"])[rows], data[p]["clean"], data[p]["noisy"],
                      data[p]["center"], data[p]["scale"])
        # idxs maps back to the input cloud: all rows of an FPS patch, the radius list and the duplicates' sources of a padded one
        L = min(nn_[c], s)
        lst = host(tr["idx_noisy"])[on[c]:on[c + 1]]
        assert np.array_equal(query[p][:L], room["noisy"][idxs[p][:L]])
        if tr["branch"][p] == "pad":
            assert np.array_equal(idxs[p][:L], lst) and np.all(np.isin(idxs[p][L:], lst))
            level = 1e-2 * np.linalg.norm(np.ptp(room["noisy"][lst].astype(np.float64), axis=0))
            assert np.abs(query[p][L:] - room["noisy"][idxs[p][L:]]).max() < 6 * level
        else:
            assert idxs[p][0] == lst[0] and len(set(idxs[p].tolist())) == s and np.all(np.isin(idxs[p], lst))
            pts = room["noisy"][lst].astype(np.float64)  # exact FPS from index 0: every pick is a farthest point of the rest
            dmin, pos = np.full(len(lst), np.inf), np.searchsorted(lst, idxs[p][:9])  # (picks as positions in the patch)
            for a, b in zip(pos[:8], pos[1:]):
                dmin = np.minimum(dmin, ((pts - pts[a]) ** 2).sum(1))
                assert dmin[b] >= dmin.max() * (1 - 1e-6)  # (fp32 distances on the device, fp64 here)
        # every clean row is a row of the clean cloud: the same fp32 subtraction and division give the same bits
        src = room["clean"][ref_rows[rows]]
        assert np.array_equal(data[p]["clean"][:, :3], (src - data[p]["center"]) / data[p]["scale"])
        assert np.array_equal(data[p]["clean"][:, 3:], room["clean_rgb"][ref_rows[rows]])
        assert np.array_equal(data[p]["features"], room["feats"][idxs[p]].astype(np.float16))
        assert {k: (v.dtype, v.shape) for k, v in data[p].items()} == {
            "clean": (np.float32, (s, 6)), "noisy": (np.float32, (s, 6)), "idxs": (np.int64, (s,)),
            "features": (np.float16, (s, 8)), "center": (np.float32, (3,)), "scale": (np.float32, ())}


def test_end_to_end_is_deterministic_and_chunked(room, monkeypatch):
    """the same seed gives the same bytes, also when the patches are taken in chunks of three"""
    monkeypatch.setattr(RP, "IDX_BYTES", 3 * E2E_NPOINTS * 128 * 4)
    trace = {}
    np.random.seed(42)
    data, stats = RP.create_spherical_batches(dev(room["clean"]), dev(room["noisy"]), dev(room["clean_rgb"]), dev(room["rgb"]),
                                              room["feats"], room["args"], trace=trace)
    assert len(trace["chunks"]) == -(-len(data) // 3) and stats == room["stats"] and len(data) == len(room["data"])
    for a, b in zip(data, room["data"]):
        assert list(a) == list(b) == ["clean", "noisy", "idxs", "features", "center", "scale"]
        for key in a:
            assert a[key].tobytes() == b[key].tobytes(), key


def test_handle_scene_writes_files_the_loader_reads(room, tmp_path, monkeypatch):
    verts, faces, vcol = _room_mesh()
    scans = tmp_path / "data" / "scene0" / "scans"
    os.makedirs(scans), os.makedirs(tmp_path / "data" / "scene0" / "features"), os.makedirs(tmp_path / "splits")
    with open(scans / "mesh_aligned_0.05.ply", "w") as f:
        f.write(f"ply\nformat ascii 1.0\nelement vertex {len(verts)}\nproperty float x\nproperty float y\nproperty float z\n"
                "property uchar red\nproperty uchar green\nproperty uchar blue\n"
                f"element face {len(faces)}\nproperty list uchar int vertex_indices\nend_header\n")
        for v, c in zip(verts, np.rint(vcol * 255).astype(int)):
            f.write("%r %r %r %d %d %d\n" % (float(v[0]), float(v[1]), float(v[2]), c[0], c[1], c[2]))
        for t in faces:
            f.write("3 %d %d %d\n" % tuple(t))
    scan_fusion.write_ply(str(scans / "iphone.ply"), room["noisy"], room["rgb8"])
    np.save(tmp_path / "data" / "scene0" / "features" / "dino_iphone.npy", room["feats"].T)
    os.makedirs(tmp_path / "data" / "empty_scene")
    (tmp_path / "splits" / "snpp_train.txt").write_text("scene0\n")
    monkeypatch.chdir(tmp_path)
    RP.main(["--data_root", "data", "--output_root", "out", "--npoints", str(E2E_NPOINTS), "--r", str(E2E_R), "--nprocs", "7"])
    files = sorted(os.listdir(tmp_path / "out" / "scene0"))
    assert len(files) >= 10 and files[0] == "points_0.npz" and not os.path.exists(tmp_path / "out" / "empty_scene")
    arrays = np.load(tmp_path / "out" / "scene0" / "points_0.npz")
    assert sorted(arrays.files) == sorted(json.loads('["center", "clean", "features", "idxs", "noisy", "scale"]'))
    ds = room_data.ScanNetPP(str(tmp_path / "out"), "training", additional_features=True)
    assert len(ds) == len(files)
    sample = ds[0]
    for key, shape in (("noisy_points", (E2E_NPOINTS, 3)), ("clean_points", (E2E_NPOINTS, 3)), ("noisy_colors", (E2E_NPOINTS, 3)),
                       ("clean_colors", (E2E_NPOINTS, 3)), ("noisy_features", (E2E_NPOINTS, 8))):
        assert sample[key].shape == shape and sample[key].dtype == torch.float32 and bool(torch.isfinite(sample[key]).all()), key


# ---- the reference's recorded run ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "room_pairs.npz"))


def _golden_run(golden, put=dev):
    np.random.seed(int(golden["seed"]))
    args = {"npoints": int(golden["npoints"]), "r": float(golden["r"])}
    return RP.create_spherical_batches(put(golden["pcd_clean"]), put(golden["pcd_noisy"]), put(golden["rgb_clean"]),
                                       put(golden["rgb_noisy"]), golden["features"], args, centers_idx=golden["centers_idx"])


def test_against_the_reference_fixture(golden):
    data, (skipped, uniq, avg) = _golden_run(golden)
    n_kept = int(golden["n_kept"])
    assert len(data) == n_kept and skipped == len(golden["centers_idx"]) - n_kept  # with equal idxs: the same kept set
    assert sorted(data[0]) == json.loads(str(golden["keys"]))
    clean64 = golden["pcd_clean"].astype(np.float64)

    def rows_of(xyz):  # the clean-cloud row of every de-normalised clean point
        return np.array([np.argmin(((clean64 - p) ** 2).sum(1)) for p in xyz])

    uniq_ref = 0.0
    for j, d in enumerate(data):
        rec = {k: golden[f"patch{j}_{k}"] for k in ("clean", "noisy", "idxs", "features", "center", "scale")}
        assert np.array_equal(d["idxs"], rec["idxs"]) and np.array_equal(d["features"], rec["features"])
        c, sc = rec["center"], float(rec["scale"])
        mine = rows_of(d["clean"][:, :3].astype(np.float64) * float(d["scale"]) + d["center"].astype(np.float64))
        theirs = rows_of(rec["clean"][:, :3] * sc + c)
        assert np.array_equal(mine, theirs)  # the assignment
        uniq_ref += len(np.unique(theirs)) / len(theirs)
        # the Finish bounds, plus the fp32 rounding of the jittered points (one ulp of the coordinate magnitude), which the
        # reference keeps in fp64: it moves the mean, the largest norm and the points themselves by at most that
        jit = pairs_ref.ulp32(np.abs(golden["pcd_noisy"][rec["idxs"]]).max())
        assert np.all(np.abs(d["center"] - c) <= 0.5 * pairs_ref.ulp32(c) + jit)
        assert abs(float(d["scale"]) - sc) <= pairs_ref.ulp32(np.abs(c).max()) + 2.0 ** -22 * sc + jit
        bound = pairs_ref.ulp32(np.abs(c).max()) / sc + 2.0 ** -22 + jit / sc
        assert np.abs(d["noisy"][:, :3] - rec["noisy"][:, :3]).max() <= bound
        assert np.abs(d["clean"][:, :3] - rec["clean"][:, :3]).max() <= bound
        assert np.array_equal(d["noisy"][:, 3:], rec["noisy"][:, 3:].astype(np.float32))
        assert np.array_equal(d["clean"][:, 3:], rec["clean"][:, 3:].astype(np.float32))
    assert abs(uniq - uniq_ref / n_kept) < 1e-12


# ---- memory and CPU tensors ------------------------------------------------------------------------------------------
def test_wrappers_hold_to_their_buffers(golden, clouds):
    verts, faces, vcol = _square_mesh()
    u = np.random.default_rng(8).uniform(0, 1, (999, 3))
    query, refs = clouds
    ref, off = np.concatenate(refs), offsets([len(r) for r in refs])
    rng = np.random.default_rng(9)
    rgb_q, rgb_r = rng.uniform(0, 1, query.shape).astype(np.float32), rng.uniform(0, 1, ref.shape).astype(np.float32)
    want_mesh = RP.sample_mesh(dev(verts), dev(faces), dev(u), dev(vcol))
    want_knn = RP.patch_knn(dev(query), dev(ref), dev(off), K=128)
    want_assign = RP.unique_assign(want_knn[0], dev(off))
    want_fin = RP.finish(dev(query), dev(rgb_q), dev(ref), dev(rgb_r), dev(off), want_assign[0])
    want_data = _golden_run(golden)[0]
    with PoisonArena("cuda", 96 << 20) as arena:
        put = lambda a: arena.put(torch.from_numpy(np.array(a)))  # noqa: E731
        before = arena.n_allocations
        got = RP.sample_mesh(put(verts), put(faces), put(u), put(vcol))
        arena.check_guards()
        assert arena.n_allocations >= before + 9  # four inputs, areas, flag, face, xyz, rgb
        arena.assert_written(got[1], "xyz"), arena.assert_written(got[2], "rgb")
        assert all(torch.equal(a, b) for a, b in zip(got, want_mesh))
        q, r, o = put(query), put(ref), put(off)
        before = arena.n_allocations
        got = RP.patch_knn(q, r, o, K=128)
        arena.check_guards()
        assert arena.n_allocations >= before + 2
        arena.assert_written(got[1], "dist2")
        assert torch.equal(got[0], want_knn[0]) and torch.equal(got[1], want_knn[1])
        before = arena.n_allocations
        got_a = RP.unique_assign(got[0], o)
        arena.check_guards()
        assert arena.n_allocations >= before + 3  # owner, assign, unique
        assert torch.equal(got_a[0], want_assign[0]) and torch.equal(got_a[1], want_assign[1])
        before = arena.n_allocations
        got = RP.finish(q, put(rgb_q), r, put(rgb_r), o, got_a[0])
        arena.check_guards()
        assert arena.n_allocations >= before + 6
        for a, b, name in zip(got, want_fin, ("clean", "noisy", "center", "scale")):
            arena.assert_written(a, name)
            assert torch.equal(a, b), name
        before = arena.n_allocations
        data = _golden_run(golden, put)[0]
        arena.check_guards()
        assert arena.n_allocations >= before + 4 + 4 + 7  # the clouds, two radius queries, the three kernels' outputs
        for a, b in zip(data, want_data):
            assert all(a[k].tobytes() == b[k].tobytes() for k in a)


def test_cpu_tensors_raise():
    x, off = torch.zeros(1, 40, 3), torch.tensor([0, 40])
    nn = torch.zeros(1, 40, 4, dtype=torch.int32)
    verts, faces, _ = _square_mesh()
    for fn in (lambda: RP.patch_knn(x, x[0].cuda(), off.cuda(), K=4), lambda: RP.patch_knn(x.cuda(), x[0], off.cuda(), K=4),
               lambda: RP.patch_knn(x.cuda(), x[0].cuda(), off, K=4), lambda: RP.unique_assign(nn, off.cuda()),
               lambda: RP.unique_assign(nn.cuda(), off), lambda: RP.finish(x, x, x[0], x[0], off, nn[..., 0]),
               lambda: RP.sample_mesh(torch.from_numpy(verts), torch.from_numpy(faces).cuda(), torch.zeros(4, 3).double().cuda()),
               lambda: RP.mesh_cdf(torch.from_numpy(verts).cuda(), torch.from_numpy(faces)),
               lambda: RP.create_spherical_batches(x[0], x[0].cuda(), x[0].cuda(), x[0].cuda(), None, {"npoints": 16, "r": 1.0})):
        with pytest.raises(RuntimeError):
            fn()
