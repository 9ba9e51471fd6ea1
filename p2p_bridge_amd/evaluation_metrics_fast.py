"""Set-level generative metrics -- MMD / COV / 1-NNA under Chamfer and approximate EMD, and the occupancy-grid JSD -- with the
names and signatures of the reference's metrics/evaluation_metrics_fast.py, so that the import can be swapped.

What differs from the reference ("Set metrics"):
  * a distance matrix between two SETS of clouds is one library call (csrc/setmetrics.hip: p2pb_pairwise_chamfer,
    p2pb_pairwise_emd) instead of one expand().contiguous() + batched extension call per cloud (:209-231); `batch_size` is
    accepted and no longer bounds memory -- the workspace does (EMD_WS_BYTES);
  * compute_all_metrics computes each of the three matrices once per metric (the reference computes the sample-vs-reference one
    twice, :423-440 and :479-496);
  * the JSD's point-to-cell assignment is p2pb_occupancy_counts for CUDA tensors (the reference: sklearn NearestNeighbors);
  * no tabulate / loguru / scipy / sklearn: the table text and the entropies are restated here.
CUDA tensors run the kernels (a missing library is an error, not a fallback); CPU tensors and numpy arrays take a pure torch /
numpy path with the same arithmetic contract, which is what the host-logic tests run.
"""
import math
import warnings

import numpy as np
import torch

EMD_WS_BYTES = None  # workspace cap of the pairwise-EMD call in bytes (None: the library's suggestion, 4096 pairs in flight)


# ------------------------------------------------------------------------------------------------------------------
# per-batch distances (the reference's building blocks, kept for callers that use them directly)
# ------------------------------------------------------------------------------------------------------------------
def distChamferCUDA(x, y):
    """[B,N,3], [B,M,3] -> (dist1 [B,N], dist2 [B,M]), differentiable (:23-30)"""
    from . import metrics

    d1, d2, _, _ = metrics.chamfer_3DDist()(x.cuda(), y.cuda())
    return d1, d2


def distChamferCUDAnograd(x, y):
    assert x.shape[-1] == 3 and y.shape[-1] == 3, f"get {x.shape} and {y.shape}"
    from . import metrics

    d1, d2, _, _ = metrics.chamfer_3DDist_nograd()(x.cuda(), y.cuda())
    return d1, d2


def emd_approx(sample, ref, require_grad=True):
    """approxmatch cost / N per cloud, [B,N,3] inputs (:42-65)"""
    from . import metrics

    fn = metrics.earth_mover_distance if require_grad else metrics.earth_mover_distance_nograd
    return fn(sample.cuda(), ref.cuda(), transpose=False)


def distChamfer(a, b):
    """the matmul form |x|^2 + |y|^2 - 2 x.y (:89-99): P[b, i, j] between y_i and x_j -> (min over i, min over j)"""
    gram_a = torch.bmm(a, a.transpose(2, 1))
    gram_b = torch.bmm(b, b.transpose(2, 1))
    cross = torch.bmm(a, b.transpose(2, 1))
    sq_a = torch.diagonal(gram_a, dim1=1, dim2=2).unsqueeze(1).expand_as(gram_a)
    sq_b = torch.diagonal(gram_b, dim1=1, dim2=2).unsqueeze(1).expand_as(gram_b)
    P = sq_a.transpose(2, 1) + sq_b - 2 * cross
    return P.min(1)[0], P.min(2)[0]


def _cd_rows_torch(x, y):
    """CPU counterpart of the chamfer kernel: fp32 squared differences, per-point minima, torch's fp32 means"""
    d = ((x.unsqueeze(2) - y.unsqueeze(1)) ** 2).sum(-1)
    return d.min(2)[0], d.min(1)[0]


def _emd_rows_torch(x, y):
    """CPU counterpart of approxmatch + matchcost (PyTorchEMD/cuda/emd_kernel.cu:33,211) / N, vectorised over the batch: the ten
    annealing levels -4^7 .. -4^-1, 0; the match cost is accumulated per level as the pairwise kernel does"""
    n, m = x.shape[1], y.shape[1]
    d = ((x.unsqueeze(2) - y.unsqueeze(1)) ** 2).sum(-1)  # [B, n, m]
    remain_l = torch.full(x.shape[:2], 1.0 if n >= m else float(m // n), dtype=x.dtype)
    remain_r = torch.full(y.shape[:2], float(n // m) if n >= m else 1.0, dtype=x.dtype)
    cost = torch.zeros(x.shape[0], dtype=x.dtype)
    for j in range(7, -3, -1):
        e = torch.exp((0.0 if j == -2 else -(4.0 ** j)) * d)
        ratio_l = remain_l / (1e-9 + (e * remain_r.unsqueeze(1)).sum(2))
        sum_r = (e * ratio_l.unsqueeze(2)).sum(1) * remain_r
        ratio_r = torch.clamp(remain_r / (sum_r + 1e-9), max=1.0) * remain_r
        remain_r = torch.clamp(remain_r - sum_r, min=0.0)
        w = e * ratio_l.unsqueeze(2) * ratio_r.unsqueeze(1)
        remain_l = torch.clamp(remain_l - w.sum(2), min=0.0)
        cost = cost + (w * d).sum((1, 2))
    return cost / float(n)


def EMD_CD(sample_pcs, ref_pcs, batch_size, accelerated_cd=False, reduced=True, require_grad=False):
    """cloud i of one set against cloud i of the other (:102-145) -> {"MMD-CD", "MMD-EMD"}"""
    n_sample, n_ref = sample_pcs.shape[0], ref_pcs.shape[0]
    assert n_sample == n_ref, "REF:%d SMP:%d" % (n_ref, n_sample)
    on_gpu = sample_pcs.is_cuda
    cd, emd = [], []
    for lo in range(0, n_sample, batch_size):
        s, r = sample_pcs[lo:lo + batch_size], ref_pcs[lo:lo + batch_size]
        if not accelerated_cd:
            dl, dr = distChamfer(s, r)
        elif not on_gpu:
            dl, dr = _cd_rows_torch(s, r)
        else:
            dl, dr = distChamferCUDA(s, r) if require_grad else distChamferCUDAnograd(s, r)
        cd.append(dl.mean(dim=1) + dr.mean(dim=1))
        emd.append(emd_approx(s, r, require_grad=require_grad) if on_gpu else _emd_rows_torch(s, r))
    cd, emd = torch.cat(cd), torch.cat(emd)
    if reduced:
        cd, emd = cd.mean(), emd.mean()
    return {"MMD-CD": cd, "MMD-EMD": emd}


# ------------------------------------------------------------------------------------------------------------------
# the one-line result table (:148-187). tabulate is not a dependency: its "tsv" / "plain" layout for ONE data row is
# restated in _table (numeric cells are re-printed with "%g" and right-aligned under their header, text cells are
# left-aligned, every column is at least two characters wider than its header, lines are right-stripped).
# ------------------------------------------------------------------------------------------------------------------
_COLUMNS = (("MMD-CDx0.001↓", "lgan_mmd-CD", 1000.0, 4), ("MMD-EMDx0.01↓", "lgan_mmd-EMD", 100.0, 4),
            ("COV-CD%↑", "lgan_cov-CD", 100.0, 2), ("COV-EMD%↑", "lgan_cov-EMD", 100.0, 2),
            ("1-NNA-CD%↓", "1-NN-CD-acc", 100.0, 2), ("1-NNA-EMD%↓", "1-NN-EMD-acc", 100.0, 2), ("JSD↓", "jsd", 1.0, 2))


def formulate_results(results, dataset, hash, step, epoch):
    """-> (header cells, value cells); "-" drops the dataset / model column, empty step and epoch drop `reported`"""
    head, row = [], []
    if dataset != "-":
        head.append("Dataset"), row.append(f"{dataset}")
    if hash != "-":
        head.append("Model"), row.append(f"{hash}")
    if step != "" or epoch != "":
        head.append("reported"), row.append(f"S{step}E{epoch}")
    for title, key, factor, digits in _COLUMNS:
        head.append(title), row.append("%.*f" % (digits, results.get(key, 0) * factor))
    if results.get("url", None) is not None:
        head.append("url"), row.append(f"{results.get('url', '-')}")
    # (the reference joins with blanks and splits again: a cell that holds a blank becomes several cells)
    return " ".join(head).split(" "), " ".join(row).split(" ")


def _cell_kind(text):
    for kind in (int, float):
        try:
            v = kind(text)
        except ValueError:
            continue
        if kind is float and (math.isinf(v) or math.isnan(v)) and text.lower() not in ("inf", "-inf", "nan"):
            return str
        return kind
    return str


def _table(head, row, sep):
    cells_h, cells_r = [], []
    for h, c in zip(head, row):
        kind = _cell_kind(c)
        text = format(float(c), "g") if kind is float else c
        width = max(len(h) + 2, len(text))
        if kind is str:
            cells_h.append(h.ljust(width)), cells_r.append(text.ljust(width))
        else:
            cells_h.append(h.rjust(width)), cells_r.append(text.rjust(width))
    return sep.join(cells_h).rstrip() + "\n" + sep.join(cells_r).rstrip()


def write_results(out_file, results, dataset="", hash="", step="", epoch=""):
    """appends the table as tab-separated text to out_file and returns it"""
    head, row = formulate_results(results, dataset, hash, step, epoch)
    text = _table(head, row, "\t")
    with open(out_file, "a") as f:
        f.write(text + "\n")
    return text


def print_results(results, dataset="-", hash="-", step="", epoch=""):
    head, row = formulate_results(results, dataset, hash, step, epoch)
    text = _table(head, row, "  ")
    print("\n" + text)
    return text


# ------------------------------------------------------------------------------------------------------------------
# distance matrices between two sets of clouds
# ------------------------------------------------------------------------------------------------------------------
def _set_tensors(a, b):
    from ._lib import check

    a, b = a.detach().float().contiguous(), b.detach().float().contiguous()
    if a.dim() != 3 or b.dim() != 3 or a.shape[-1] != 3 or b.shape[-1] != 3:
        raise RuntimeError(f"sets of clouds must be [S,N,3] and [R,M,3]; get {tuple(a.shape)} and {tuple(b.shape)}")
    check(a, torch.float32, "sample_pcs"), check(b, torch.float32, "ref_pcs")
    if a.device != b.device:
        raise RuntimeError("both sets must be on the same device")
    return a, b


def pairwise_chamfer(a, b):
    """a [S,N,3], b [R,M,3] CUDA tensors -> f32 [S,R] of mean_p min_q + mean_q min_p (p2pb_pairwise_chamfer). Passing the same
    tensor twice takes the symmetric form (each directional sum once; the result equals its transpose bitwise)."""
    from ._lib import ask, call, ptr, stream_ptr

    same = a is b or (a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.is_contiguous() and b.is_contiguous()
                      and a.dtype == b.dtype == torch.float32)
    a, b = _set_tensors(a, b)
    if same:
        b = a
    (s, n, _), (r, m, _) = a.shape, b.shape
    with torch.cuda.device(a.device):
        out = torch.empty(s, r, dtype=torch.float32, device=a.device)
        ws = torch.empty(max(1, ask("p2pb_pairwise_chamfer_ws_bytes", s, r)), dtype=torch.uint8, device=a.device)
        call("p2pb_pairwise_chamfer", s, r, n, m, ptr(a), ptr(b), ptr(out), ptr(ws), stream_ptr())
    return out


def pairwise_emd(a, b, ws_bytes=None):
    """-> f32 [S,R] of earth_mover_distance_nograd(a_i, b_j) (p2pb_pairwise_emd); ws_bytes caps the scratch (pairs run in chunks)"""
    from ._lib import ask, call, ptr, stream_ptr

    a, b = _set_tensors(a, b)
    (s, n, _), (r, m, _) = a.shape, b.shape
    want = ask("p2pb_pairwise_emd_ws_bytes", s, r, n, m)
    cap = ws_bytes if ws_bytes is not None else EMD_WS_BYTES
    nbytes = max(1, want if cap is None else min(want, int(cap)))
    with torch.cuda.device(a.device):
        out = torch.empty(s, r, dtype=torch.float32, device=a.device)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=a.device)
        call("p2pb_pairwise_emd", s, r, n, m, ptr(a), ptr(b), ptr(out), ptr(ws), nbytes, stream_ptr())
    return out


def _pairwise_EMD_CD_sub(metric, sample_batch, ref_pcs, N_ref, batch_size, accelerated_cd, verbose, require_grad):
    """ONE cloud against a set, by the reference's route (:190-242): the cloud expanded to the size of each batch of the set and
    the batched ops called on it -> the same [1, N_ref] row twice. _pairwise_EMD_CD_ only comes here when gradients are wanted
    or for the matmul Chamfer form."""
    if metric not in ("CD", "EMD"):
        raise NotImplementedError
    on_gpu = ref_pcs.is_cuda
    row = []
    for lo in range(0, N_ref, batch_size):
        ref_batch = ref_pcs[lo:min(N_ref, lo + batch_size)]
        rep = sample_batch.reshape(1, -1, ref_batch.size(2)).expand(ref_batch.size(0), -1, -1).contiguous()
        if metric == "EMD":
            row.append((emd_approx(rep, ref_batch, require_grad=require_grad) if on_gpu else _emd_rows_torch(rep, ref_batch)).view(1, -1))
            continue
        if not accelerated_cd:
            dl, dr = distChamfer(rep, ref_batch)
        elif not on_gpu:
            dl, dr = _cd_rows_torch(rep, ref_batch)
        else:
            dl, dr = distChamferCUDA(rep, ref_batch) if require_grad else distChamferCUDAnograd(rep, ref_batch)
        row.append((dl.mean(dim=1) + dr.mean(dim=1)).view(1, -1))
    row = torch.cat(row, dim=1)
    return row, row


def _pairwise_EMD_CD_(metric, sample_pcs, ref_pcs, batch_size, require_grad=True, accelerated_cd=True, verbose=True):
    """[S,N,3] against [R,M,3] -> the [S,R] matrix, twice (:245-281). CUDA tensors that ask for no gradient take the pairwise
    kernels (EMD always, Chamfer with accelerated_cd); everything else goes row by row like the reference."""
    if metric not in ("CD", "EMD"):
        raise NotImplementedError
    wants_grad = require_grad and torch.is_grad_enabled() and (sample_pcs.requires_grad or ref_pcs.requires_grad)
    if sample_pcs.is_cuda and ref_pcs.is_cuda and not wants_grad and (metric == "EMD" or accelerated_cd):
        M = pairwise_chamfer(sample_pcs, ref_pcs) if metric == "CD" else pairwise_emd(sample_pcs, ref_pcs)
        return M, M
    n_ref = ref_pcs.shape[0]
    rows = [_pairwise_EMD_CD_sub(metric, sample_pcs[i], ref_pcs, n_ref, batch_size, accelerated_cd, verbose,
                                 require_grad and wants_grad)[0] for i in range(sample_pcs.shape[0])]
    M = torch.cat(rows, dim=0)
    return M, M


# ------------------------------------------------------------------------------------------------------------------
# statistics of the matrices (torch, on the matrices' device)
# ------------------------------------------------------------------------------------------------------------------
def knn(Mxx, Mxy, Myy, k, sqrt=False):
    """leave-one-out k-NN classifier between the two sets (:334-371): label 1 = the first set"""
    n0, n1 = Mxx.size(0), Myy.size(0)
    label = torch.cat((torch.ones(n0), torch.zeros(n1))).to(Mxx)
    M = torch.cat([torch.cat((Mxx, Mxy), 1), torch.cat((Mxy.transpose(0, 1), Myy), 1)], 0)
    if sqrt:
        M = M.abs().sqrt()
    _, idx = (M + torch.diag(float("inf") * torch.ones(n0 + n1).to(Mxx))).topk(k, 0, False)
    votes = torch.zeros(n0 + n1).to(Mxx)
    for i in range(k):
        votes = votes + label.index_select(0, idx[i])
    pred = torch.ge(votes, (float(k) / 2) * torch.ones(n0 + n1).to(Mxx)).float()
    tp, fp = (pred * label).sum(), (pred * (1 - label)).sum()
    fn, tn = ((1 - pred) * label).sum(), ((1 - pred) * (1 - label)).sum()
    return {"tp": tp, "fp": fp, "fn": fn, "tn": tn,
            "precision": tp / (tp + fp + 1e-10), "recall": tp / (tp + fn + 1e-10),
            "acc_t": tp / (tp + fn + 1e-10), "acc_f": tn / (tn + fp + 1e-10),
            "acc": torch.eq(label, pred).float().mean()}


def lgan_mmd_cov(all_dist):
    """all_dist [N_sample, N_ref] -> MMD (mean over references of the nearest sample), its sample-side counterpart, and COV (the
    share of references that are some sample's nearest) (:374-386)"""
    n_ref = all_dist.size(1)
    from_smp, nearest_ref = torch.min(all_dist, dim=1)
    from_ref, _ = torch.min(all_dist, dim=0)
    cov = float(nearest_ref.unique().view(-1).size(0)) / float(n_ref)
    return {"lgan_mmd": from_ref.mean(), "lgan_cov": torch.tensor(cov).to(all_dist), "lgan_mmd_smp": from_smp.mean()}


def compute_all_metrics(sample_pcs, ref_pcs, batch_size, verbose=True, accelerated_cd=False, metric1="CD", metric2="EMD",
                        **print_kwargs):
    """MMD / COV / 1-NNA under metric1 and (unless None) metric2 (:389-528); [B,N,3] or [B,3,N] inputs. Three matrices per
    metric: reference-vs-sample, reference-vs-reference, sample-vs-sample."""
    if sample_pcs.shape[-1] != 3:
        sample_pcs, ref_pcs = sample_pcs.transpose(-1, -2), ref_pcs.transpose(-1, -2)
    sample_pcs, ref_pcs = sample_pcs.contiguous(), ref_pcs.contiguous()
    batch_size = ref_pcs.shape[0] // 2 if ref_pcs.shape[0] != batch_size else batch_size
    results = {}
    for metric in (metric1, metric2):
        if metric is None:
            continue
        kw = dict(accelerated_cd=accelerated_cd, require_grad=False, verbose=False)
        M_rs, _ = _pairwise_EMD_CD_(metric, ref_pcs, sample_pcs, batch_size, **kw)
        results.update({"%s-%s" % (k, metric): v.item() for k, v in lgan_mmd_cov(M_rs.t()).items()})
        if verbose:
            print_results(results, **print_kwargs)
        M_rr, _ = _pairwise_EMD_CD_(metric, ref_pcs, ref_pcs, batch_size, **kw)
        M_ss, _ = _pairwise_EMD_CD_(metric, sample_pcs, sample_pcs, batch_size, **kw)
        one_nn = knn(M_rr, M_rs, M_ss, 1, sqrt=False)
        results.update({"1-NN-%s-%s" % (metric, k): v.item() for k, v in one_nn.items() if "acc" in k})
        if verbose:
            print_results(results, **print_kwargs)
    return results


# ------------------------------------------------------------------------------------------------------------------
# JSD between the occupancy distributions of two sets (:534-650; Achlioptas et al., latent_3d_points)
# ------------------------------------------------------------------------------------------------------------------
def unit_cube_grid_point_cloud(resolution, clip_sphere=False):
    """-> (centres of the resolution^3 cells of the unit cube, float32 [res,res,res,3] -- or [G,3], the cells with centre norm
    <= 0.5 in row-major order, with clip_sphere -- and the spacing)"""
    spacing = 1.0 / float(resolution - 1)
    axis = (np.arange(resolution) * spacing - 0.5).astype(np.float32)
    grid = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), axis=-1)
    if clip_sphere:
        grid = grid.reshape(-1, 3)
        grid = grid[np.linalg.norm(grid, axis=1) <= 0.5]
    return grid, spacing


def _occupancy_counts_host(pclouds, resolution, in_sphere):
    """numpy counterpart of p2pb_occupancy_counts: nearest centre per axis; where the clip removed that cell, an exact float64
    search over the kept cells (lowest index on a tie)"""
    grid, spacing = unit_cube_grid_point_cloud(resolution, in_sphere)
    grid = grid.reshape(-1, 3).astype(np.float64)
    axis = (np.arange(resolution) * spacing - 0.5).astype(np.float32).astype(np.float64)
    index_of = np.arange(resolution ** 3)
    if in_sphere:
        full = unit_cube_grid_point_cloud(resolution, False)[0].reshape(-1, 3)
        kept = np.linalg.norm(full, axis=1) <= 0.5
        index_of = np.where(kept, np.cumsum(kept) - 1, -1)
    counters, bernoulli = np.zeros(len(grid), np.int64), np.zeros(len(grid), np.int64)
    for pc in np.asarray(pclouds, np.float64):
        ijk = np.abs(pc[:, :, None] - axis[None, None, :]).argmin(-1)
        cell = index_of[(ijk[:, 0] * resolution + ijk[:, 1]) * resolution + ijk[:, 2]]
        for p in np.nonzero(cell < 0)[0]:
            cell[p] = ((grid - pc[p]) ** 2).sum(-1).argmin()
        counters += np.bincount(cell, minlength=len(grid))
        bernoulli[np.unique(cell)] += 1
    return counters, bernoulli


def occupancy_counts(pclouds, resolution, in_sphere=False):
    """pclouds [clouds, npts, 3] -> (counters, bernoulli) as float64 numpy arrays over the grid cells: points per cell and clouds
    per cell. CUDA tensors run p2pb_occupancy_counts; numpy arrays and CPU tensors the host path."""
    if not (torch.is_tensor(pclouds) and pclouds.is_cuda):
        pts = pclouds.detach().numpy() if torch.is_tensor(pclouds) else pclouds
        c, b = _occupancy_counts_host(pts, resolution, in_sphere)
        return c.astype(np.float64), b.astype(np.float64)
    from ._lib import ask, call, check, ptr, stream_ptr

    pts = pclouds.detach().float().contiguous()
    check(pts, torch.float32, "pclouds")
    cells = ask("p2pb_occupancy_grid_cells", int(resolution), int(bool(in_sphere)))
    if cells <= 0:
        raise RuntimeError(f"occupancy grid of resolution {resolution} (in_sphere={in_sphere}) is not supported")
    expect = len(unit_cube_grid_point_cloud(resolution, in_sphere)[0].reshape(-1, 3))
    assert cells == expect, (cells, expect)  # the library's grid is numpy's grid
    with torch.cuda.device(pts.device):
        out = torch.empty(2, cells, dtype=torch.int32, device=pts.device)
        ws = torch.empty(ask("p2pb_occupancy_ws_bytes", int(resolution)), dtype=torch.uint8, device=pts.device)
        call("p2pb_occupancy_counts", pts.shape[0], pts.shape[1], int(resolution), int(bool(in_sphere)), ptr(pts), ptr(out[0]),
             ptr(out[1]), ptr(ws), stream_ptr())
    host = out.cpu().numpy().astype(np.float64)
    return host[0], host[1]


def _entropy(pk, base=None):
    """Shannon entropy of the distribution pk / sum(pk) in nats, or in units of log(base) (scipy.stats.entropy)"""
    pk = np.asarray(pk, np.float64)
    pk = pk / np.sum(pk)
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = np.where(pk > 0, -pk * np.log(pk), 0.0)
    h = np.sum(terms)
    return h / math.log(base) if base is not None else h


def entropy_of_occupancy_grid(pclouds, grid_resolution, in_sphere=False, verbose=False):
    """-> (mean entropy of the per-cell "some point of a cloud falls here" Bernoulli variables, points per cell) (:570-609)"""
    limit = 0.5 + 10e-4
    if verbose:
        pts = pclouds.detach().cpu().numpy() if torch.is_tensor(pclouds) else np.asarray(pclouds)
        if abs(np.max(pts)) > limit or abs(np.min(pts)) > limit:
            warnings.warn("Point-clouds are not in unit cube.")
        if in_sphere and np.max(np.sqrt(np.sum(pts ** 2, axis=2))) > limit:
            warnings.warn("Point-clouds are not in unit sphere.")
    counters, bernoulli = occupancy_counts(pclouds, grid_resolution, in_sphere)
    n = float(len(pclouds))
    acc = 0.0
    for g in bernoulli:
        if g > 0:
            p = float(g) / n
            acc += _entropy([p, 1.0 - p])
    return acc / len(counters), counters


def jsd_between_point_cloud_sets(sample_pcs, ref_pcs, resolution=28):
    """JSD between the occupancy distributions of two sets of clouds normalised into the sphere of radius 0.5 (:555-567)"""
    sample_counts = entropy_of_occupancy_grid(sample_pcs, resolution, True)[1]
    ref_counts = entropy_of_occupancy_grid(ref_pcs, resolution, True)[1]
    return jensen_shannon_divergence(sample_counts, ref_counts)


def jensen_shannon_divergence(P, Q):
    if np.any(P < 0) or np.any(Q < 0):
        raise ValueError("Negative values.")
    if len(P) != len(Q):
        raise ValueError("Non equal size.")
    P_, Q_ = P / np.sum(P), Q / np.sum(Q)
    res = _entropy((P_ + Q_) / 2.0, base=2) - (_entropy(P_, base=2) + _entropy(Q_, base=2)) / 2.0
    if not np.allclose(res, _jsdiv(P_, Q_), atol=10e-5, rtol=0):
        warnings.warn("Numerical values of two JSD methods don't agree.")
    return res


def _jsdiv(P, Q):
    """the same through two Kullback-Leibler divergences to the mixture"""

    def kl(a, b):
        both = np.logical_and(a > 0, b > 0)
        a, b = a[both], b[both]
        return np.sum(a * np.log2(a / b))

    P_, Q_ = P / np.sum(P), Q / np.sum(Q)
    mix = 0.5 * (P_ + Q_)
    return 0.5 * (kl(P_, mix) + kl(Q_, mix))
