"""The set-metric kernels (csrc/setmetrics.hip: p2pb_pairwise_chamfer, p2pb_pairwise_emd, p2pb_occupancy_counts) and the GPU path
of p2p_bridge_amd/evaluation_metrics_fast.py, against the package's existing per-batch ops on expanded inputs and against
tests/golden/set_metrics.npz (the reference's module on the CPU oracle, tools/make_golden_setmetrics.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "set_metrics.npz"))
EINVAL = -22
EXACT_KEYS = ("lgan_cov-CD", "1-NN-CD-acc", "1-NN-CD-acc_t", "1-NN-CD-acc_f", "lgan_cov-EMD", "1-NN-EMD-acc", "1-NN-EMD-acc_t",
              "1-NN-EMD-acc_f")


def E():
    from p2p_bridge_amd import evaluation_metrics_fast

    return evaluation_metrics_fast


def dev(name):
    return torch.from_numpy(G[name]).cuda()


def fixture_dict(prefix):
    return dict(zip(G[prefix + "_keys"].tolist(), G[prefix + "_vals"].tolist()))


def cd_by_existing_op(a, b):
    """float32(sum dist1 / n + sum dist2 / m), summed in float64 from chamfer_3DDist_nograd on the expanded inputs"""
    from p2p_bridge_amd import metrics

    rows = []
    for i in range(a.shape[0]):
        d1, d2, _, _ = metrics.chamfer_3DDist_nograd()(a[i:i + 1].expand(b.shape[0], -1, -1).contiguous(), b)
        rows.append((d1.double().sum(1) / a.shape[1] + d2.double().sum(1) / b.shape[1]).float())
    return torch.stack(rows).cpu().numpy()


def assert_one_ulp(got, want, what):
    ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    ulps = np.where(got == want, 0.0, ulps)
    print(f"{what}: max distance to the existing op = {ulps.max():.2f} fp32 ulp over {got.size} pairs")
    assert ulps.max() <= 1.0, (what, ulps.max())


@pytest.mark.parametrize("a,b", [("ref", "smp"), ("smp", "ref"), ("ref_nm", "smp_nm"), ("smp_nm", "ref_nm"), ("ref", "ref")])
def test_pairwise_chamfer_vs_existing_op_fixture_sets(a, b):
    A, B = dev(a), dev(b)
    got = E().pairwise_chamfer(A, B if a != b else A).cpu().numpy()
    assert_one_ulp(got, cd_by_existing_op(A, B), f"{a} x {b}")


def test_pairwise_chamfer_vs_existing_op_large():
    """48 x 40 clouds, n = 2048 against m = 1024 (a resident 1024-point tile one way, a full 2048-point tile the other)"""
    g = torch.Generator().manual_seed(5)
    A = (torch.rand(48, 2048, 3, generator=g) - 0.5).cuda()
    B = (torch.randn(40, 1024, 3, generator=g) * 0.2).cuda()
    assert_one_ulp(E().pairwise_chamfer(A, B).cpu().numpy(), cd_by_existing_op(A, B), "48 x 40, 2048 / 1024")


def test_pairwise_chamfer_targets_longer_than_one_tile():
    """m = 2500 > the 2048-point LDS tile (the tiled path) and n = 2100 > 2048 queries per pass"""
    g = torch.Generator().manual_seed(6)
    A = torch.rand(5, 2100, 3, generator=g).cuda()
    B = torch.rand(3, 2500, 3, generator=g).cuda()
    assert_one_ulp(E().pairwise_chamfer(A, B).cpu().numpy(), cd_by_existing_op(A, B), "5 x 3, 2100 / 2500")


def test_pairwise_chamfer_vs_fixture():
    """against the reference's matrices: accelerated_cd=True (oracle minima, torch fp32 means) at 2e-6 relative -- torch's fp32
    mean of 256..2048 positive terms carries a few log2(n) 2^-24; accelerated_cd=False (matmul form, which cancels) at twice
    the gap the fixture itself shows between its two forms: measured 1.35e-6 relative (M_rr), so 2.71e-6."""
    mats = {"rs": E().pairwise_chamfer(dev("ref"), dev("smp")), "rr": E().pairwise_chamfer(dev("ref"), dev("ref")),
            "ss": E().pairwise_chamfer(dev("smp"), dev("smp"))}
    gap = 0.0
    for k in mats:
        a, b = G["cd_acc_" + k].astype(np.float64), G["cd_mm_" + k].astype(np.float64)
        assert np.array_equal(a == 0, b == 0)  # (only the diagonals of rr / ss, exactly zero in both forms)
        gap = max(gap, (np.abs(a - b)[a > 0] / a[a > 0]).max())
    print(f"fixture gap between the oracle form and the matmul form: {gap:.3e} relative -> tolerance {2 * gap:.3e}")
    for k, M in mats.items():
        got = M.cpu().numpy()
        np.testing.assert_allclose(got, G["cd_acc_" + k], rtol=2e-6, atol=0)
        np.testing.assert_allclose(got, G["cd_mm_" + k], rtol=2 * gap, atol=0)
    for a, b, key in (("ref_nm", "smp_nm", "cd_nm_rs"), ("smp_nm", "ref_nm", "cd_nm_sr")):
        np.testing.assert_allclose(E().pairwise_chamfer(dev(a), dev(b)).cpu().numpy(), G[key], rtol=2e-6, atol=0)


def test_pairwise_chamfer_symmetric_and_deterministic():
    for name in ("ref", "smp"):
        A = dev(name)
        M = E().pairwise_chamfer(A, A)
        assert torch.equal(M, M.t().contiguous())
        assert torch.equal(M, E().pairwise_chamfer(A, A))
        # the general path on a copy of the same set: the same numbers without the shortcut
        assert torch.equal(M, E().pairwise_chamfer(A, A.clone()))
    A, B = dev("ref"), dev("smp")
    assert torch.equal(E().pairwise_chamfer(A, B), E().pairwise_chamfer(A, B))
    assert torch.equal(E().pairwise_chamfer(A, B), E().pairwise_chamfer(B, A).t().contiguous())


def test_pairwise_emd_vs_fixture_and_existing_op():
    """2e-3 relative against the oracle-built fixture (the project's approxmatch gate: __expf); the gap to the existing
    earth_mover_distance_nograd on expanded inputs (same kernels' arithmetic, match matrix stored, fp32 atomics in the cost) is
    measured (1.4e-7 relative on the fixture sets), printed and held to the same 2e-3. Two calls give identical bytes; a small workspace (chunks of 7 pairs) too."""
    from p2p_bridge_amd import metrics

    worst = 0.0
    for a, b, key in (("ref", "smp", "emd_rs"), ("ref", "ref", "emd_rr"), ("smp", "smp", "emd_ss")):
        A, B = dev(a), dev(b)
        M = E().pairwise_emd(A, B)
        np.testing.assert_allclose(M.cpu().numpy(), G[key], rtol=2e-3, atol=0)
        assert torch.equal(M, E().pairwise_emd(A, B))
        assert torch.equal(M, E().pairwise_emd(A, B, ws_bytes=7 * (3 * A.shape[1] + 2 * B.shape[1]) * 4))
        old = torch.stack([metrics.earth_mover_distance_nograd(A[i:i + 1].expand(B.shape[0], -1, -1).contiguous(), B, transpose=False)
                           for i in range(A.shape[0])])
        gap = ((M - old).abs() / old.abs()).max().item()
        print(f"{key}: max relative gap to earth_mover_distance_nograd on expanded inputs = {gap:.3e}")
        worst = max(worst, gap)
    assert worst <= 2e-3, worst


def test_pairwise_emd_unequal_sizes():
    """n != m (256 against 128: multiR = 2) against the existing op"""
    from p2p_bridge_amd import metrics

    A, B = dev("smp")[:5], dev("ref")[:4, :128].contiguous()
    for X, Y in ((A, B), (B, A)):
        M = E().pairwise_emd(X, Y)
        old = torch.stack([metrics.earth_mover_distance_nograd(X[i:i + 1].expand(Y.shape[0], -1, -1).contiguous(), Y, transpose=False)
                           for i in range(X.shape[0])])
        np.testing.assert_allclose(M.cpu().numpy(), old.cpu().numpy(), rtol=2e-3, atol=0)


@pytest.mark.parametrize("name", ["smp", "ref", "set"])
def test_occupancy_counts_vs_fixture(name):
    """every fixture point; `set` has 17 % of its points rounding to a cell the sphere clip removed (the exact search)"""
    clouds = dev("jsd_set" if name == "set" else name)
    counters, bernoulli = E().occupancy_counts(clouds, int(G["resolution"]), True)
    assert np.array_equal(counters, G[f"jsd_{name}_counters"])
    assert np.array_equal(bernoulli, G[f"jsd_{name}_bernoulli"].astype(np.float64))
    c2, b2 = E().occupancy_counts(clouds, int(G["resolution"]), True)
    assert np.array_equal(c2, counters) and np.array_equal(b2, bernoulli)
    ent, _ = E().entropy_of_occupancy_grid(clouds, int(G["resolution"]), in_sphere=True)
    assert abs(ent - float(G[f"jsd_{name}_entropy"])) <= 1e-12 * float(G[f"jsd_{name}_entropy"])


def test_occupancy_counts_unclipped_grid_vs_host_path():
    clouds = dev("jsd_set")
    got = E().occupancy_counts(clouds, 12, False)
    want = E().occupancy_counts(G["jsd_set"], 12, False)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[0].sum() == 8 * 512


def test_jsd_vs_fixture():
    for a, key in (("smp", "jsd_smp_ref"), ("jsd_set", "jsd_set_ref")):
        got = E().jsd_between_point_cloud_sets(dev(a), dev("ref"), int(G["resolution"]))
        assert abs(got - float(G[key])) <= 1e-12 * float(G[key]), (got, float(G[key]))


@pytest.mark.parametrize("layout", ["bn3", "b3n"])
def test_compute_all_metrics_gpu(layout):
    smp, ref = dev("smp"), dev("ref")
    if layout == "b3n":
        smp, ref = smp.transpose(1, 2).contiguous(), ref.transpose(1, 2).contiguous()
    got = E().compute_all_metrics(smp, ref, 10, verbose=False, accelerated_cd=True)
    want = dict(fixture_dict("cd_acc_all"), **fixture_dict("emd_all"))
    assert sorted(got) == sorted(want)
    for k, w in want.items():
        if k in EXACT_KEYS:
            assert got[k] == w, (k, got[k], w)
        else:
            assert abs(got[k] - w) <= (2e-3 if "EMD" in k else 2e-6) * abs(w), (k, got[k], w)


def test_bad_sizes_are_einval():
    from p2p_bridge_amd._lib import lib, ptr, stream_ptr

    L = lib()
    x = torch.zeros(2, 64, 3, device="cuda")
    out = torch.zeros(4, device="cuda")
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(2, 21952, dtype=torch.int32, device="cuda")
    occ_ws = torch.zeros(L.p2pb_occupancy_ws_bytes(28), dtype=torch.uint8, device="cuda")
    for s, r, n, m in ((0, 2, 64, 64), (2, 0, 64, 64), (2, 2, 0, 64), (2, 2, 64, 0), (-1, 2, 64, 64), (2, 2, 64, -5)):
        assert L.p2pb_pairwise_chamfer(s, r, n, m, ptr(x), ptr(x), ptr(out), ptr(ws), stream_ptr()) == EINVAL
        assert L.p2pb_pairwise_emd(s, r, n, m, ptr(x), ptr(x), ptr(out), ptr(ws), ctypes.c_size_t(1 << 16), stream_ptr()) == EINVAL
        assert L.p2pb_pairwise_chamfer_ws_bytes(s, r) == 0 or s * r > 0
        assert L.p2pb_pairwise_emd_ws_bytes(s, r, n, m) == 0
    # a workspace that cannot hold one pair
    assert L.p2pb_pairwise_emd(2, 2, 64, 64, ptr(x), ptr(x), ptr(out), ptr(ws), ctypes.c_size_t(64), stream_ptr()) == EINVAL
    for clouds, npts, res in ((0, 64, 28), (2, 0, 28), (-2, 64, 28), (2, -1, 28), (2, 64, 1), (2, 64, 0), (2, 64, -3), (2, 64, 81)):
        assert L.p2pb_occupancy_counts(clouds, npts, res, 0, ptr(x), ptr(cnt[0]), ptr(cnt[1]), ptr(occ_ws), stream_ptr()) == EINVAL
    assert L.p2pb_occupancy_counts(2, 64, 2, 1, ptr(x), ptr(cnt[0]), ptr(cnt[1]), ptr(occ_ws), stream_ptr()) == EINVAL  # no cell kept
    assert L.p2pb_occupancy_grid_cells(1, 0) == EINVAL and L.p2pb_occupancy_ws_bytes(1) == 0
    assert L.p2pb_occupancy_grid_cells(28, 0) == 28 ** 3 and L.p2pb_occupancy_grid_cells(28, 1) == len(G["grid_clip"])
    torch.cuda.synchronize()


def test_entry_points_capture_into_a_graph():
    """every launch goes to the caller's stream: the three entry points captured in one torch.cuda.graph and replayed give the
    bytes of the eager calls"""
    from p2p_bridge_amd._lib import call, lib, ptr, stream_ptr

    L = lib()
    A, B, P = dev("ref"), dev("smp"), dev("jsd_set")
    (s, n, _), (r, m, _) = A.shape, B.shape
    res, cells = int(G["resolution"]), len(G["grid_clip"])
    cd, emd = torch.empty(s, r, device="cuda"), torch.empty(s, r, device="cuda")
    occ = torch.empty(2, cells, dtype=torch.int32, device="cuda")
    emd_bytes = L.p2pb_pairwise_emd_ws_bytes(s, r, n, m) // 4  # (several chunks of pairs inside the capture)
    ws = [torch.empty(nb, dtype=torch.uint8, device="cuda")
          for nb in (L.p2pb_pairwise_chamfer_ws_bytes(s, r), emd_bytes, L.p2pb_occupancy_ws_bytes(res))]

    def run():
        call("p2pb_pairwise_chamfer", s, r, n, m, ptr(A), ptr(B), ptr(cd), ptr(ws[0]), stream_ptr())
        call("p2pb_pairwise_emd", s, r, n, m, ptr(A), ptr(B), ptr(emd), ptr(ws[1]), ctypes.c_size_t(emd_bytes), stream_ptr())
        call("p2pb_occupancy_counts", P.shape[0], P.shape[1], res, 1, ptr(P), ptr(occ[0]), ptr(occ[1]), ptr(ws[2]), stream_ptr())

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = [t.clone() for t in (cd, emd, occ)]
    assert np.array_equal(eager[2][0].cpu().numpy().astype(np.float64), G["jsd_set_counters"])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for t in (cd, emd, occ):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for t, e in zip((cd, emd, occ), eager):
        assert torch.equal(t, e)
