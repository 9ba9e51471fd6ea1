"""The grid nearest-point search's interface, as far as it goes without a GPU: the entry point in the header and the binding,
the checks that come before any device work, and the new choice of evaluate_rooms. The search itself:
tests/test_nn_grid_gpu.py."""
import inspect
import os
import re
from ctypes import c_float, c_int, c_void_p

import pytest
import torch

from p2p_bridge_amd import _lib, evaluate_rooms, knn_grid, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_binding_types_the_entry_point():
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "p2pb_hip.h")).read(), flags=re.S)
    found = re.findall(r"\bint\s+p2pb_nn_grid\s*\(([^)]*)\)\s*;", text)
    assert len(found) == 1 and len(found[0].split(",")) == 13
    ret, args = _lib.SIGNATURES["p2pb_nn_grid"]
    assert ret is c_int and len(args) == 13
    assert all(args[i] is c_int for i in range(3)) and args[8] is c_float
    assert all(args[i] is c_void_p for i in (3, 4, 5, 6, 7, 9, 10, 11, 12))
    assert _lib.ABI_VERSION == 13  # (a pure addition)
    assert list(_lib.lib().p2pb_nn_grid.argtypes) == args


def test_entry_point_refuses_bad_sizes_before_any_launch():
    """P2PB_EINVAL comes back from the host-side checks: nothing is launched, no GPU is needed"""
    one = c_void_p(8)  # (never followed)
    good = [4, 200, 3, None, one, one, one, one, 0.1, one, one, one, None]
    for at, bad in ((0, 0), (0, -1), (1, 0), (2, 0), (2, 17), (8, 0.0), (8, -1.0), (8, float("inf")), (8, float("nan"))):
        args = list(good)
        args[at] = bad
        assert _lib.ask("p2pb_nn_grid", *args) != 0, (at, bad)
    for hole in (4, 5, 6, 7, 9, 10, 11):
        args = list(good)
        args[hole] = None
        assert _lib.ask("p2pb_nn_grid", *args) != 0, hole


def test_new_keywords_and_their_defaults():
    assert list(inspect.signature(knn_grid.PointGrid.nearest).parameters) == ["self", "query", "order", "return_stats"]
    p = inspect.signature(metrics.cd_unit_sphere).parameters
    assert p["method"].default == "brute" and p["ref_grid"].default is None and p["normalize"].default is True
    assert list(inspect.signature(metrics.chamfer_grid).parameters) == ["xyz1", "xyz2", "grid1", "grid2"]
    assert inspect.signature(evaluate_rooms.get_mectrics).parameters["ref_grid"].default is None
    assert evaluate_rooms.CD_METHOD_DEFAULT == "brute"


def test_unknown_cd_method_is_refused_before_any_device_work():
    p = torch.zeros(1, 4, 3)  # (CPU tensors: the Chamfer kernels would refuse them with another exception)
    with pytest.raises(ValueError, match="method"):
        metrics.cd_unit_sphere(p, p, method="bogus")
    with pytest.raises(ValueError, match="method"):
        metrics.cd_unit_sphere(p, p, normalize=False, method="bogus")
    with pytest.raises(ValueError, match="ref_grid"):
        metrics.cd_unit_sphere(p, p, method="brute", ref_grid=object())
    with pytest.raises(ValueError, match="cd_method"):
        evaluate_rooms.get_mectrics({"dataset": "arkit", "cd_method": "bogus"}, p[0].numpy(), p[0].numpy())
    with pytest.raises(RuntimeError, match="grad"):
        metrics.chamfer_grid(p.clone().requires_grad_(), p)


def test_cpu_tensors_are_refused():
    ref = torch.zeros(200, 3)
    with pytest.raises(RuntimeError, match="CUDA"):
        metrics.chamfer_grid(ref[None], ref[None])
    with pytest.raises(RuntimeError, match="CUDA"):
        metrics.cd_unit_sphere(ref[None], ref[None], normalize=False, method="grid")


def test_parser_takes_cd_method(capsys):
    ap = evaluate_rooms.build_parser()
    base = ["--data_root", "x", "--dataset", "arkit"]
    assert ap.parse_args(base).cd_method == "brute"
    assert ap.parse_args(base + ["--cd_method", "grid"]).cd_method == "grid"
    assert ap.parse_args(base + ["--cd_method", "brute"]).cd_method == "brute"
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--cd_method", "kdtree"])
    assert "--cd_method" in capsys.readouterr().err
