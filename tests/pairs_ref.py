"""Plain numpy restatements of the room-pairs contracts (include/p2pb_hip.h, "room training pairs"), written from the contracts
and used by tests/test_room_pairs.py (no GPU) and tests/test_room_pairs_gpu.py."""
import numpy as np


# ---- assignment ------------------------------------------------------------------------------------------------------
def sequential_assign(nn):
    """point i (ascending) takes the first entry of nn[i] that no point j < i has taken; all taken: nn[i][0], taking nothing"""
    nn = np.asarray(nn)
    taken = set()
    out = np.empty(nn.shape[0], dtype=np.int64)
    for i, row in enumerate(nn):
        for t in row:
            if int(t) not in taken:
                taken.add(int(t))
                out[i] = t
                break
        else:
            out[i] = row[0]
    return out


def deferred_acceptance(nn, m):
    """the parallel loop of csrc/pairs.hip in numpy: every point whose cursor is below K lowers owner[target] to its own index,
    then the points whose target a lower index owns move on by one. -> (assign i64[s], rounds)"""
    nn = np.asarray(nn)
    s, k = nn.shape
    owner = np.full(m, np.iinfo(np.int64).max, dtype=np.int64)
    cur = np.zeros(s, dtype=np.int64)
    ids = np.arange(s)
    rounds = 0
    while True:
        rounds += 1
        live = ids[cur < k]
        tg = nn[live, cur[live]]
        np.minimum.at(owner, tg, live)
        lose = owner[tg] < live
        cur[live[lose]] += 1
        if not lose.any():
            break
    return nn[ids, np.where(cur < k, cur, 0)], rounds


def assign_lists(kind, s, k, m, seed=0):
    """the neighbour-list sets of the tests -> nn i32[s,k] with entries in [0, m)"""
    rng = np.random.default_rng(seed)
    if kind == "random":  # k distinct entries per point
        return np.stack([rng.permutation(m)[:k] for _ in range(s)]).astype(np.int32)
    if kind == "identical":  # everybody wants 0, 1, 2, ...: k + 1 rounds, s - k fall-backs
        return np.tile(np.arange(k, dtype=np.int32), (s, 1))
    if kind == "shifted":  # point i wants i, i + 1, ... (mod m)
        return ((np.arange(s)[:, None] + np.arange(k)[None]) % m).astype(np.int32)
    if kind == "geometric":  # the k nearest of m points to s points of the same surface
        ref = rng.uniform(0, 1, (m, 3)).astype(np.float32)
        ref[:, 2] *= 0.02
        q = (ref[rng.integers(0, m, s)] + rng.normal(0, 0.01, (s, 3))).astype(np.float32)
        return knn_brute(q, ref, k)[0].astype(np.int32)
    raise ValueError(kind)


# ---- k-NN ------------------------------------------------------------------------------------------------------------
def knn_brute(query, ref, k):
    """fp64 squared distances of fp32 inputs; the k smallest ascending, ties by ascending index -> (idx i64[s,k], d2 f64[s,k])"""
    q, r = np.asarray(query, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    idx = np.empty((len(q), k), dtype=np.int64)
    d2 = np.empty((len(q), k))
    for lo in range(0, len(q), 256):
        d = ((q[lo:lo + 256, None, :] - r[None]) ** 2).sum(-1)
        order = np.argsort(d, axis=1, kind="stable")[:, :k]  # (stable: equal distances stay in index order)
        idx[lo:lo + 256] = order
        d2[lo:lo + 256] = np.take_along_axis(d, order, 1)
    return idx, d2


def knn_gaps_ok(query, ref, k, rel=1e-5):
    """consecutive neighbour distances up to rank k + 1 differ by more than `rel` relative for every query: then fp32 and fp64
    arithmetic give the same lists"""
    d2 = knn_brute(query, ref, min(k + 1, len(ref)))[1]
    d = np.sqrt(d2)
    return bool(np.all(np.diff(d, axis=1) > rel * d[:, 1:]))


# ---- mesh ------------------------------------------------------------------------------------------------------------
def tri_areas(verts, faces):
    v = np.asarray(verts, dtype=np.float64)
    a, b, c = (v[np.asarray(faces)[:, j]] for j in range(3))
    cr = np.cross(b - a, c - a)
    return 0.5 * np.sqrt((cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1]) + cr[:, 2] * cr[:, 2])


def sample_mesh(verts, faces, cdf, u, vcol=None):
    """-> (face i64[n], xyz f64[n,3], rgb f64[n,3] | None): searchsorted(cdf, u0 * total, side="right"), weights
    (1 - s, s (1 - u2), s u2), s = sqrt(u1); fp64, NOT yet rounded"""
    cdf, u = np.asarray(cdf, dtype=np.float64), np.asarray(u, dtype=np.float64)
    face = np.minimum(np.searchsorted(cdf, u[:, 0] * cdf[-1], side="right"), len(cdf) - 1)
    s = np.sqrt(u[:, 1])
    w = np.stack([1.0 - s, s * (1.0 - u[:, 2]), s * u[:, 2]], 1)
    tri = np.asarray(faces)[face]

    def mix(values):
        t = np.asarray(values, dtype=np.float64)[tri]  # [n, corner, axis]
        return (w[:, 0, None] * t[:, 0] + w[:, 1, None] * t[:, 1]) + w[:, 2, None] * t[:, 2]

    return face, mix(verts), None if vcol is None else mix(vcol)


# ---- normalisation ---------------------------------------------------------------------------------------------------
def center_fp64(noisy_xyz):
    """the fp64 sum in index order / s (np.cumsum adds sequentially), not yet rounded"""
    p = np.asarray(noisy_xyz, dtype=np.float64)
    return np.cumsum(p, axis=0)[-1] / p.shape[0]


def normalise_fp64(noisy_xyz, clean_xyz):
    """-> (noisy f64[s,3], clean f64[s,3], center f64[3], scale f64) with everything in fp64"""
    c = center_fp64(noisy_xyz)
    d = np.asarray(noisy_xyz, dtype=np.float64) - c
    scale = np.max(np.linalg.norm(d, axis=1))
    return d / scale, (np.asarray(clean_xyz, dtype=np.float64) - c) / scale, c, scale


def ulp32(x):
    return np.spacing(np.float32(np.abs(x))).astype(np.float64)
