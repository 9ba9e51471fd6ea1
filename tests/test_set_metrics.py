"""Host logic of p2p_bridge_amd/evaluation_metrics_fast.py on CPU tensors against tests/golden/set_metrics.npz (the reference's own
module run by tools/make_golden_setmetrics.py): knn, lgan_mmd_cov, the JSD arithmetic, the grid, the result table, and
compute_all_metrics on the pure-torch path. Integer-valued results and text match exactly, floating-point results at 1e-6
relative, the entropy / JSD arithmetic at 1e-12 when fed the fixture's counters. No GPU needed."""
import os

import numpy as np
import pytest
import torch

from p2p_bridge_amd import evaluation_metrics_fast as E

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "set_metrics.npz"))
COUNTS = ("tp", "fp", "fn", "tn")


def fixture_dict(prefix):
    return dict(zip(G[prefix + "_keys"].tolist(), G[prefix + "_vals"].tolist()))


def t(name):
    return torch.from_numpy(G[name])


def assert_stats(got, want, rel=1e-6, exact=()):
    assert sorted(got) == sorted(want)
    for k, w in want.items():
        g = float(got[k])
        if k in exact:
            assert g == w, (k, g, w)
        else:
            assert abs(g - w) <= rel * abs(w), (k, g, w)


@pytest.mark.parametrize("tag", ["cd_acc", "cd_mm", "emd"])
def test_knn_and_lgan_on_fixture_matrices(tag):
    M_rs, M_rr, M_ss = t(tag + "_rs"), t(tag + "_rr"), t(tag + "_ss")
    assert_stats(E.knn(M_rr, M_rs, M_ss, 1, sqrt=False), fixture_dict(tag + "_knn"), exact=COUNTS + ("acc", "acc_t", "acc_f"))
    assert_stats(E.lgan_mmd_cov(M_rs.t()), fixture_dict(tag + "_lgan"), exact=("lgan_cov",))


@pytest.mark.parametrize("i", [0, 1, 2])
def test_knn_and_lgan_with_exact_ties(i):
    Mxx, Mxy, Myy = t(f"tie{i}_xx"), t(f"tie{i}_xy"), t(f"tie{i}_yy")
    for k in (1, 3):
        assert_stats(E.knn(Mxx, Mxy, Myy, k, sqrt=(i == 1)), fixture_dict(f"tie{i}_knn{k}"), exact=COUNTS + ("acc",))
    assert_stats(E.lgan_mmd_cov(Mxy), fixture_dict(f"tie{i}_lgan"), exact=("lgan_cov",))


def test_unit_cube_grid():
    res = int(G["resolution"])
    grid, spacing = E.unit_cube_grid_point_cloud(res, True)
    assert spacing == float(G["grid_spacing"])
    assert grid.dtype == np.float32 and np.array_equal(grid, G["grid_clip"])
    full, _ = E.unit_cube_grid_point_cloud(res, False)
    assert full.shape == (res, res, res, 3) and full.dtype == np.float32
    assert np.array_equal(full[:2, :2, :2], G["grid_full_corner"])
    assert np.array_equal(full.reshape(-1, 3)[np.linalg.norm(full.reshape(-1, 3), axis=1) <= 0.5], grid)


def test_jsd_arithmetic_on_fixture_counters():
    for a, want in (("smp", "jsd_smp_ref"), ("set", "jsd_set_ref")):
        got = E.jensen_shannon_divergence(G[f"jsd_{a}_counters"], G["jsd_ref_counters"])
        assert abs(got - float(G[want])) <= 1e-12 * abs(float(G[want])), (got, float(G[want]))
        P, Q = G[f"jsd_{a}_counters"], G["jsd_ref_counters"]
        assert abs(E._jsdiv(P / P.sum(), Q / Q.sum()) - float(G[want])) < 1e-9
    with pytest.raises(ValueError):
        E.jensen_shannon_divergence(np.array([1.0, -1.0]), np.array([1.0, 1.0]))
    with pytest.raises(ValueError):
        E.jensen_shannon_divergence(np.ones(3), np.ones(4))


@pytest.mark.parametrize("name", ["smp", "ref", "set"])
def test_occupancy_host_path_all_points(name):
    """every fixture point (the generator re-drew the ambiguous ones): counters and touched-cloud counts exactly, then the entropy"""
    clouds = G["jsd_set"] if name == "set" else G[name]
    counters, bernoulli = E.occupancy_counts(clouds, int(G["resolution"]), True)
    assert np.array_equal(counters, G[f"jsd_{name}_counters"])
    assert np.array_equal(bernoulli, G[f"jsd_{name}_bernoulli"].astype(np.float64))
    ent, c2 = E.entropy_of_occupancy_grid(torch.from_numpy(clouds), int(G["resolution"]), in_sphere=True)
    want = float(G[f"jsd_{name}_entropy"])
    assert np.array_equal(c2, counters) and abs(ent - want) <= 1e-12 * want, (ent, want)


def test_jsd_between_sets_host_path():
    got = E.jsd_between_point_cloud_sets(G["jsd_set"], G["ref"], int(G["resolution"]))
    assert abs(got - float(G["jsd_set_ref"])) <= 1e-12 * float(G["jsd_set_ref"])


def _results():
    r = fixture_dict("cd_acc_all")
    r.update(fixture_dict("emd_all"))
    r["jsd"] = float(G["jsd_smp_ref"])
    return r


def test_result_table_text(tmp_path):
    cases = [dict(), dict(dataset="chair", hash="a1b2", step="100", epoch="7"), dict(dataset="-", hash="-"),
             dict(dataset="shapenet-airplane", hash="-", step="", epoch="12")]
    f = str(tmp_path / "r.tsv")
    texts = [E.write_results(f, _results(), **c) for c in cases]
    texts.append(E.write_results(f, dict(_results(), url="http://x/y"), dataset="car", hash="m"))
    assert texts == G["tsv_texts"].tolist()
    assert open(f).read() == str(G["tsv_file"])
    assert E.print_results(_results(), dataset="chair", hash="a1b2", step="3", epoch="") == str(G["plain_text"])
    head, row = E.formulate_results(_results(), "chair", "a1b2", "100", "7")
    assert head == G["formulate_head"].tolist() and row == G["formulate_row"].tolist()


EXACT_KEYS = ("lgan_cov-CD", "1-NN-CD-acc", "1-NN-CD-acc_t", "1-NN-CD-acc_f", "lgan_cov-EMD", "1-NN-EMD-acc", "1-NN-EMD-acc_t",
              "1-NN-EMD-acc_f")


@pytest.mark.parametrize("accelerated,layout", [(False, "bn3"), (True, "bn3"), (True, "b3n")])
def test_compute_all_metrics_cd_on_cpu(accelerated, layout):
    """CD only (metric2=None), both Chamfer forms: the matmul form repeats the reference's operations; the difference form is
    the kernel's arithmetic in torch (fp32 minima, torch's fp32 means: what the reference does around the oracle)"""
    smp, ref = t("smp"), t("ref")
    if layout == "b3n":
        smp, ref = smp.transpose(1, 2).contiguous(), ref.transpose(1, 2).contiguous()
    got = E.compute_all_metrics(smp, ref, 10, verbose=False, accelerated_cd=accelerated, metric2=None)
    assert_stats(got, fixture_dict("cd_acc_all" if accelerated else "cd_mm_all"), exact=EXACT_KEYS)


def test_pairwise_matrices_on_cpu():
    """_pairwise_EMD_CD_ / _sub on CPU tensors: the (M, M) pair, the [1, N_ref] row, n != m"""
    smp, ref = t("smp"), t("ref")
    a, b = E._pairwise_EMD_CD_("CD", ref, smp, 10, require_grad=False, accelerated_cd=True, verbose=False)
    assert a is b and tuple(a.shape) == (20, 24)
    np.testing.assert_allclose(a.numpy(), G["cd_acc_rs"], rtol=1e-6, atol=0)
    row, row2 = E._pairwise_EMD_CD_sub("CD", ref[3], smp, 24, 7, False, False, False)
    assert row is row2 and tuple(row.shape) == (1, 24)
    np.testing.assert_allclose(row.numpy()[0], G["cd_mm_rs"][3], rtol=1e-6, atol=0)
    nm = E._pairwise_EMD_CD_("CD", t("ref_nm"), t("smp_nm"), 5, require_grad=False, accelerated_cd=True, verbose=False)[0]
    np.testing.assert_allclose(nm.numpy(), G["cd_nm_rs"], rtol=1e-6, atol=0)
    with pytest.raises(NotImplementedError):
        E._pairwise_EMD_CD_("L1", ref, smp, 10)


def test_compute_all_metrics_emd_on_cpu():
    """the torch approxmatch (exp in fp32, vectorised sums) against the oracle-built EMD fixture: the project's approxmatch
    gate, 2e-3 relative, on the MMD values; COV and the 1-NN accuracies exactly. A subset keeps the CPU run short."""
    smp, ref = t("smp"), t("ref")
    M = E._pairwise_EMD_CD_("EMD", ref[:6], smp[:8], 3, require_grad=False, verbose=False)[0]
    np.testing.assert_allclose(M.numpy(), G["emd_rs"][:6, :8], rtol=2e-3, atol=0)
    got = E.compute_all_metrics(smp, ref, 10, verbose=False, accelerated_cd=True, metric1="EMD", metric2=None)
    assert_stats(got, fixture_dict("emd_all"), rel=2e-3, exact=EXACT_KEYS)


def test_emd_cd_paired_on_cpu():
    smp, ref = t("smp")[:20], t("ref")
    r = E.EMD_CD(ref, smp, 8, accelerated_cd=True, reduced=False)  # (approxmatch is not symmetric: M_rs[i, i] = emd(ref_i, smp_i))
    assert tuple(r["MMD-CD"].shape) == (20,) and tuple(r["MMD-EMD"].shape) == (20,)
    np.testing.assert_allclose(r["MMD-CD"].numpy(), np.diagonal(G["cd_acc_rs"][:, :20]), rtol=1e-6, atol=0)
    np.testing.assert_allclose(r["MMD-EMD"].numpy(), np.diagonal(G["emd_rs"][:, :20]), rtol=2e-3, atol=0)
    with pytest.raises(AssertionError):
        E.EMD_CD(t("smp"), ref, 8)


def test_module_needs_no_optional_dependency():
    """tabulate / loguru / scipy / sklearn are not guaranteed where the metrics run"""
    import subprocess
    import sys

    code = ("import sys\n"
            "for m in ('tabulate', 'loguru', 'scipy', 'sklearn'):\n    sys.modules[m] = None\n"
            "import p2p_bridge_amd.evaluation_metrics_fast as E\n"
            "import p2p_bridge_amd.evaluate_sets\n"
            "print(E.write_results.__name__)\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root)
    assert r.returncode == 0 and "write_results" in r.stdout, r.stderr[-2000:]
