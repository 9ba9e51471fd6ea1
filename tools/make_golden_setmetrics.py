"""tests/golden/set_metrics.npz: the reference's OWN set-level metrics (metrics/evaluation_metrics_fast.py) run on the CPU build
machine on seeded sets of clouds, with the compiled extensions it calls replaced by the CPU oracle (tools/ref_import.py:
chamfer_3D, emd_cuda; loguru stubbed) and Tensor.cuda() / torch.cuda.set_device turned into no-ops (there is no GPU there).

What it holds (data only):
  * inputs: a sample set (24 clouds) and a reference set (20 clouds) of 256 points from a handful of shape families, normalised
    into the sphere of radius 0.5; a second pair with n != m (6 x 256 against 5 x 192 points); an 8 x 512 JSD set with points
    near and beyond the sphere's surface toward the cube corners;
  * the reference's _pairwise_EMD_CD_("CD", ...) matrices M_rs / M_rr / M_ss with accelerated_cd=True (oracle chamfer) and False
    (matmul form), its compute_all_metrics(metric2=None) dictionaries, knn / lgan_mmd_cov on those matrices and on seeded random
    matrices with exact ties, write_results / print_results text;
  * EMD matrices. The reference's EMD wrapper asserts CUDA tensors (PyTorchEMD/emd_nograd.py:12), so it cannot run here (the
    same limitation as tools/make_golden_metrics.py): the matrices are built pair by pair from oracle.cpu_ops.approxmatch_forward
    / matchcost_forward divided by n -- the two calls that wrapper makes -- and the EMD result dictionary comes from the
    reference's own knn / lgan_mmd_cov on them;
  * JSD: the reference's entropy_of_occupancy_grid(..., 28, in_sphere=True) (entropy, counters) and
    jsd_between_point_cloud_sets; the per-cloud "touched" counts are rebuilt from the same sklearn assignment.
Conditions asserted here (change the INPUTS if one fails, not the tests): every grid assignment has a float64 top-2 distance gap
above 1e-5 (offending points are re-drawn); in every CD / EMD matrix each row and column minimum, and in the stacked (S+R)^2
matrix each nearest neighbour, leads its runner-up by more than 1e-4 relative.
Never run on the GPU box.     python tools/make_golden_setmetrics.py"""
import importlib
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_import  # noqa: E402

ref_import.install()
torch.cuda.set_device = lambda *_a, **_k: None
torch.Tensor.cuda = lambda self, *_a, **_k: self
E = importlib.import_module("metrics.evaluation_metrics_fast")
from oracle import cpu_ops  # noqa: E402
from sklearn.neighbors import NearestNeighbors  # noqa: E402

RES = 28
g = torch.Generator().manual_seed(2024)


def rnd(*s):
    return torch.randn(*s, generator=g)


def uni(*s):
    return torch.rand(*s, generator=g)


def shape(family, n):
    """one cloud of a shape family, with per-instance proportions and a little noise"""
    u, v = uni(n) * 2 * np.pi, uni(n) * 2 * np.pi
    k = 0.7 + 0.6 * uni(3)
    if family == "sphere":
        p = torch.nn.functional.normalize(rnd(n, 3), dim=1) * k
    elif family == "box":
        p = (uni(n, 3) - 0.5) * 2 * k
        ax = torch.randint(0, 3, (n,), generator=g)
        p[torch.arange(n), ax] = torch.sign(p[torch.arange(n), ax]) * k[ax]
    elif family == "torus":
        R, r = 1.0, 0.25 + 0.2 * float(uni(1))
        p = torch.stack(((R + r * torch.cos(v)) * torch.cos(u), (R + r * torch.cos(v)) * torch.sin(u), r * torch.sin(v)), 1)
    elif family == "rod":
        p = torch.stack((0.15 * torch.cos(u), 0.15 * torch.sin(u), (uni(n) - 0.5) * 2 * (1.0 + float(uni(1)))), 1)
    elif family == "blobs":
        c = torch.tensor([[0.6, 0.0, 0.0], [-0.6, 0.2, 0.0]])[torch.randint(0, 2, (n,), generator=g)]
        p = c + 0.2 * (0.6 + 0.8 * float(uni(1))) * rnd(n, 3)
    elif family == "disc":
        rad = torch.sqrt(uni(n)) * k[0]
        p = torch.stack((rad * torch.cos(u), rad * torch.sin(u), 0.03 * rnd(n)), 1)
    else:
        raise ValueError(family)
    return p + 0.01 * rnd(n, 3)


def to_sphere(p, radius=0.5):
    """bounding-box centre to the origin, farthest point to `radius` (what metrics.normalize_sphere does)"""
    p = p - (p.max(0)[0] + p.min(0)[0]) / 2
    return p / (p.norm(dim=1).max() / radius)


def cloud_set(families, n):
    return torch.stack([to_sphere(shape(f, n)) for f in families]).float().contiguous()


ref_set = cloud_set(["sphere"] * 4 + ["box"] * 4 + ["torus"] * 4 + ["rod"] * 4 + ["blobs"] * 4, 256)
smp_set = cloud_set(["sphere"] * 7 + ["box"] * 7 + ["torus"] * 6 + ["disc"] * 4, 256)
ref_nm = cloud_set(["sphere", "box", "torus", "rod", "blobs"], 192)
smp_nm = cloud_set(["sphere", "box", "torus", "disc", "rod", "blobs"], 256)

# ---- the JSD set with points whose unclipped nearest cell lies outside the sphere
corner = torch.nn.functional.normalize(torch.sign(rnd(8, 512, 3)) + 0.35 * rnd(8, 512, 3), dim=2)
jsd_set = torch.stack([to_sphere(shape(f, 512)) for f in ["sphere", "box", "torus", "blobs"] * 2])
edge = uni(8, 512) < 0.25
jsd_set = torch.where(edge.unsqueeze(2), corner * (0.47 + 0.08 * uni(8, 512, 1)), jsd_set).float().contiguous()

grid_clip, _ = E.unit_cube_grid_point_cloud(RES, True)
grid_full, _ = E.unit_cube_grid_point_cloud(RES, False)
nn_clip = NearestNeighbors(n_neighbors=2).fit(grid_clip.reshape(-1, 3))


def settle(clouds):
    """re-draw (jitter) every point whose two nearest kept cells are closer than 1e-5 apart in distance"""
    pts = clouds.numpy().copy()
    for _ in range(50):
        flat = pts.reshape(-1, 3)
        dist, _ = nn_clip.kneighbors(flat.astype(np.float64))
        bad = np.nonzero(dist[:, 1] - dist[:, 0] <= 1e-5)[0]
        if len(bad) == 0:
            return torch.from_numpy(pts)
        flat[bad] += (1e-3 * torch.randn(len(bad), 3, generator=g)).numpy()
    raise AssertionError("grid assignment gaps not reached")


ref_set, smp_set, jsd_set = settle(ref_set), settle(smp_set), settle(jsd_set)
out = {"ref": ref_set.numpy(), "smp": smp_set.numpy(), "ref_nm": ref_nm.numpy(), "smp_nm": smp_nm.numpy(),
       "jsd_set": jsd_set.numpy(), "resolution": np.array(RES)}


def lead(M, axis):
    s = np.sort(M, axis=axis)
    a, b = np.take(s, 0, axis), np.take(s, 1, axis)
    return ((b - a) / b).min()


def check_margins(name, M_rs, M_rr, M_ss):
    for k, M in (("rs", M_rs), ("rr", M_rr), ("ss", M_ss)):
        assert lead(M, 0) > 1e-4 and lead(M, 1) > 1e-4, (name, k, lead(M, 0), lead(M, 1))
    full = np.block([[M_rr, M_rs], [M_rs.T, M_ss]]).astype(np.float64)
    np.fill_diagonal(full, np.inf)
    assert lead(full, 0) > 1e-4, (name, "stacked", lead(full, 0))


def put_dict(prefix, d):
    keys = sorted(d)
    out[prefix + "_keys"] = np.array(keys)
    out[prefix + "_vals"] = np.array([float(d[k]) for k in keys], np.float64)


def stats(prefix, M_rs, M_rr, M_ss):
    """the reference's lgan_mmd_cov / knn on three matrices"""
    put_dict(prefix + "_lgan", E.lgan_mmd_cov(M_rs.t()))
    put_dict(prefix + "_knn", E.knn(M_rr, M_rs, M_ss, 1, sqrt=False))


# ---- Chamfer matrices through the reference's own pairwise routine
for acc in (True, False):
    tag = "cd_acc" if acc else "cd_mm"
    kw = dict(accelerated_cd=acc, require_grad=False, verbose=False)
    M_rs = E._pairwise_EMD_CD_("CD", ref_set, smp_set, 10, **kw)[0]
    M_rr = E._pairwise_EMD_CD_("CD", ref_set, ref_set, 10, **kw)[0]
    M_ss = E._pairwise_EMD_CD_("CD", smp_set, smp_set, 10, **kw)[0]
    check_margins(tag, M_rs.numpy(), M_rr.numpy(), M_ss.numpy())
    out[tag + "_rs"], out[tag + "_rr"], out[tag + "_ss"] = M_rs.numpy(), M_rr.numpy(), M_ss.numpy()
    stats(tag, M_rs, M_rr, M_ss)
    put_dict(tag + "_all", E.compute_all_metrics(smp_set, ref_set, 10, verbose=False, accelerated_cd=acc, metric2=None))
kw = dict(accelerated_cd=True, require_grad=False, verbose=False)
out["cd_nm_rs"] = E._pairwise_EMD_CD_("CD", ref_nm, smp_nm, 5, **kw)[0].numpy()
out["cd_nm_sr"] = E._pairwise_EMD_CD_("CD", smp_nm, ref_nm, 5, **kw)[0].numpy()


# ---- EMD matrices from the oracle's approxmatch / matchcost (what earth_mover_distance_nograd calls), / n
def emd_matrix(A, B):
    M = torch.empty(A.shape[0], B.shape[0])
    for i in range(A.shape[0]):
        a = A[i:i + 1].expand(B.shape[0], -1, -1).contiguous()
        match = cpu_ops.emd_cuda.approxmatch_forward(a, B)
        M[i] = cpu_ops.emd_cuda.matchcost_forward(a, B, match) / float(A.shape[1])
    return M


M_rs, M_rr, M_ss = emd_matrix(ref_set, smp_set), emd_matrix(ref_set, ref_set), emd_matrix(smp_set, smp_set)
check_margins("emd", M_rs.numpy(), M_rr.numpy(), M_ss.numpy())
out["emd_rs"], out["emd_rr"], out["emd_ss"] = M_rs.numpy(), M_rr.numpy(), M_ss.numpy()
stats("emd", M_rs, M_rr, M_ss)
emd_all = {"%s-EMD" % k: v.item() for k, v in E.lgan_mmd_cov(M_rs.t()).items()}
emd_all.update({"1-NN-EMD-%s" % k: v.item() for k, v in E.knn(M_rr, M_rs, M_ss, 1, sqrt=False).items() if "acc" in k})
put_dict("emd_all", emd_all)

# ---- knn / lgan_mmd_cov on seeded random matrices, with exact ties
for t in range(3):
    n0, n1 = 7 + t, 9 - t
    Mxx, Mxy, Myy = uni(n0, n0), uni(n0, n1), uni(n1, n1)
    Mxx, Myy = (Mxx + Mxx.t()) / 2, (Myy + Myy.t()) / 2
    Mxy[1, 2] = Mxy[:, 2].min()  # two equal minima in a column of the cross block
    Mxy[3, :] = Mxy[0, :]        # two equal rows
    Mxx[0, 1] = Mxx[1, 0] = Mxy[0].min()
    out[f"tie{t}_xx"], out[f"tie{t}_xy"], out[f"tie{t}_yy"] = Mxx.numpy(), Mxy.numpy(), Myy.numpy()
    for k in (1, 3):
        put_dict(f"tie{t}_knn{k}", E.knn(Mxx, Mxy, Myy, k, sqrt=(t == 1)))
    put_dict(f"tie{t}_lgan", E.lgan_mmd_cov(Mxy))

# ---- JSD
for name, clouds in (("smp", smp_set), ("ref", ref_set), ("set", jsd_set)):
    pts = clouds.numpy()
    ent, counters = E.entropy_of_occupancy_grid(pts, RES, in_sphere=True)
    idx = NearestNeighbors(n_neighbors=1).fit(grid_clip.reshape(-1, 3)).kneighbors(pts.reshape(-1, 3))[1].reshape(pts.shape[:2])
    mine = np.zeros(len(grid_clip), np.int64)
    touched = np.zeros(len(grid_clip), np.int64)
    for row in idx:
        mine += np.bincount(row, minlength=len(grid_clip))
        touched[np.unique(row)] += 1
    assert np.array_equal(mine, counters.astype(np.int64))
    out[f"jsd_{name}_entropy"], out[f"jsd_{name}_counters"], out[f"jsd_{name}_bernoulli"] = np.array(ent), counters, touched
full_nn = NearestNeighbors(n_neighbors=1).fit(grid_full.reshape(-1, 3))
outside = np.linalg.norm(grid_full.reshape(-1, 3)[full_nn.kneighbors(jsd_set.numpy().reshape(-1, 3))[1][:, 0]], axis=1) > 0.5
assert outside.mean() >= 0.05, outside.mean()
out["jsd_set_outside_share"] = np.array(outside.mean())
out["jsd_smp_ref"] = np.array(E.jsd_between_point_cloud_sets(smp_set.numpy(), ref_set.numpy(), RES))
out["jsd_set_ref"] = np.array(E.jsd_between_point_cloud_sets(jsd_set.numpy(), ref_set.numpy(), RES))
out["grid_clip"], out["grid_full_corner"] = grid_clip, grid_full[:2, :2, :2]
out["grid_spacing"] = np.array(E.unit_cube_grid_point_cloud(RES, True)[1])

# ---- the one-line table
results = dict(zip(out["cd_acc_all_keys"].tolist(), out["cd_acc_all_vals"].tolist()))
results.update(emd_all)
results["jsd"] = float(out["jsd_smp_ref"])
texts = []
cases = [dict(), dict(dataset="chair", hash="a1b2", step="100", epoch="7"), dict(dataset="-", hash="-"),
         dict(dataset="shapenet-airplane", hash="-", step="", epoch="12")]
with tempfile.TemporaryDirectory() as tmp:
    for c in cases:
        texts.append(E.write_results(os.path.join(tmp, "r.tsv"), results, **c))
    texts.append(E.write_results(os.path.join(tmp, "r.tsv"), dict(results, url="http://x/y"), dataset="car", hash="m"))
    out["tsv_file"] = np.array(open(os.path.join(tmp, "r.tsv")).read())
out["tsv_texts"] = np.array(texts)
out["plain_text"] = np.array(E.print_results(results, dataset="chair", hash="a1b2", step="3", epoch=""))
head, row = E.formulate_results(results, "chair", "a1b2", "100", "7")
out["formulate_head"], out["formulate_row"] = np.array(head), np.array(row)

path = os.path.join(ref_import.ROOT, "tests", "golden", "set_metrics.npz")
np.savez_compressed(path, **out)
for k, v in out.items():
    print(k, v.shape, v.dtype)
print("COV-CD", results["lgan_cov-CD"], "1-NNA-CD", results["1-NN-CD-acc"], "COV-EMD", results["lgan_cov-EMD"], "1-NNA-EMD",
      results["1-NN-EMD-acc"], "outside share", float(outside.mean()))
assert results["lgan_cov-CD"] < 1 and results["1-NN-CD-acc"] not in (0.5, 1.0)
print("wrote", path, os.path.getsize(path), "bytes")
assert os.path.getsize(path) < 1000000
