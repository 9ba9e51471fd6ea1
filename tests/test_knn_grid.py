"""The grid k-NN's interface, as far as it goes without a GPU: the new keywords of its consumers, the checks that come before
any device work, and the two entry points in the header and the binding. The search itself: tests/test_knn_grid_gpu.py."""
import inspect
import os
import re
from ctypes import c_float, c_int, c_void_p

import pytest
import torch

from p2p_bridge_amd import _lib, denoise, image_features, knn_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_consumers_accept_the_keyword_and_keep_their_defaults():
    assert inspect.signature(denoise.knn_points).parameters["method"].default == "brute"
    assert inspect.signature(image_features.interpolate_missing_features).parameters["neighbours"].default == "brute"
    assert inspect.signature(image_features.fuse_scene).parameters["neighbours"].default == "brute"


def test_unknown_method_is_refused_before_any_device_check():
    p = torch.zeros(1, 4, 3)  # (CPU tensors: a device check would raise RuntimeError first)
    with pytest.raises(ValueError, match="method"):
        denoise.knn_points(p, p, K=1, method="kdtree")
    with pytest.raises(ValueError, match="128"):
        denoise.knn_points(p, p, K=129, method="grid")
    feats, count = torch.zeros(16, 2, dtype=torch.float16), torch.ones(16, dtype=torch.int32)
    with pytest.raises(ValueError, match="neighbours"):
        image_features.interpolate_missing_features(feats, count, torch.zeros(16, 3), neighbours="kdtree")
    with pytest.raises(ValueError, match="neighbours"):
        image_features.fuse_scene(torch.zeros(16, 3), [], neighbours="kdtree")


def test_cpu_path_of_the_fill_ignores_the_choice():
    """on CPU tensors interpolate_missing_features runs its own exhaustive search whatever `neighbours` says"""
    g = torch.Generator().manual_seed(0)
    pts = torch.rand(40, 3, generator=g)
    count = (torch.rand(40, generator=g) > 0.3).to(torch.int32)
    feats = (torch.rand(40, 3, generator=g) * count[:, None]).to(torch.float16)
    a = image_features.interpolate_missing_features(feats.clone(), count, pts, k=5)
    b = image_features.interpolate_missing_features(feats.clone(), count, pts, k=5, neighbours="grid")
    assert torch.equal(a, b)


def test_header_declares_and_binding_types_the_entry_points():
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "p2pb_hip.h")).read(), flags=re.S)
    for name in ("p2pb_knn_grid", "p2pb_knn_grid_brute"):
        assert len(re.findall(r"\bint\s+%s\s*\(" % name, text)) == 1, name
    ret, args = _lib.SIGNATURES["p2pb_knn_grid"]
    assert ret is c_int and len(args) == 14
    assert all(args[i] is c_int for i in range(4)) and args[9] is c_float
    assert all(args[i] is c_void_p for i in (4, 5, 6, 7, 8, 10, 11, 12, 13))
    ret, args = _lib.SIGNATURES["p2pb_knn_grid_brute"]
    assert ret is c_int and args == [c_int] * 3 + [c_void_p] * 6
    assert _lib.ABI_VERSION == 13  # (pure additions)
    lib = _lib.lib()
    assert list(lib.p2pb_knn_grid.argtypes) == _lib.SIGNATURES["p2pb_knn_grid"][1]
    assert list(lib.p2pb_knn_grid_brute.argtypes) == _lib.SIGNATURES["p2pb_knn_grid_brute"][1]


def test_entry_points_refuse_bad_sizes_before_any_launch():
    """P2PB_EINVAL comes back from the host-side checks: nothing is launched, no GPU is needed"""
    one = c_void_p(8)  # (never followed)
    good = dict(nq=4, n=200, k=10, ring=3)
    for bad in (dict(k=0), dict(k=129), dict(k=201, n=200), dict(nq=0), dict(n=0), dict(ring=0), dict(ring=17)):
        a = dict(good, **bad)
        assert _lib.ask("p2pb_knn_grid", a["nq"], a["n"], a["k"], a["ring"], None, one, one, one, one, 0.1, one, one, one,
                        None) != 0, bad
    for cell in (0.0, -1.0, float("inf"), float("nan")):
        assert _lib.ask("p2pb_knn_grid", 4, 200, 10, 3, None, one, one, one, one, cell, one, one, one, None) != 0
    for hole in range(5, 13):
        if hole == 9:
            continue
        args = [4, 200, 10, 3, None, one, one, one, one, 0.1, one, one, one, None]
        args[hole] = None
        assert _lib.ask("p2pb_knn_grid", *args) != 0, hole
    for bad in (dict(k=0), dict(k=129), dict(k=201), dict(nq=0), dict(n=0)):
        a = dict(good, **bad)
        assert _lib.ask("p2pb_knn_grid_brute", a["nq"], a["n"], a["k"], None, one, one, one, one, None) != 0, bad
    for hole in range(4, 8):
        args = [4, 200, 10, None, one, one, one, one, None]
        args[hole] = None
        assert _lib.ask("p2pb_knn_grid_brute", *args) != 0, hole


def test_k_above_128_names_the_brute_method():
    ref = torch.zeros(200, 3)
    with pytest.raises(ValueError, match=r'knn_points\(method="brute"\)'):
        knn_grid.knn(ref, ref, 129)
    with pytest.raises(ValueError, match=r'knn_points\(method="brute"\)'):
        knn_grid.PointGrid(ref, 129)
    with pytest.raises(ValueError):
        knn_grid.knn(ref, ref, 0)


def test_cpu_tensors_are_refused():
    ref = torch.zeros(200, 3)
    with pytest.raises(RuntimeError, match="CUDA"):
        knn_grid.PointGrid(ref, 10)
    with pytest.raises(RuntimeError, match="CUDA"):
        knn_grid.knn(ref, ref, 10)
    with pytest.raises(RuntimeError):
        knn_grid.knn(ref.numpy(), ref.numpy(), 10)
    with pytest.raises(RuntimeError):
        denoise.knn_points(ref[None], ref[None], K=3, method="grid")
