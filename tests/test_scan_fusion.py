"""Scan fusion without a GPU: the ABI additions, the command line's options, the PLY round trip, CPU tensors, and the sanity of
the CPU restatement (tests/scan_ref.py) that the GPU tests compare against."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import scan_ref
from p2p_bridge_amd import scan_fusion as SF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "p2pb_hip.h")
SCAN = ["p2pb_scan_depth_valid", "p2pb_scan_backproject", "p2pb_scan_cell_keys", "p2pb_scan_segment_mean", "p2pb_scan_big_chunk_rows",
        "p2pb_scan_segment_mean_big", "p2pb_scan_radius_count", "p2pb_scan_knn_grid", "p2pb_scan_knn_brute"]


def test_header_binding_and_library_agree_on_the_scan_entry_points():
    from p2p_bridge_amd import _lib, build

    build.build()
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = sorted(s for s in set(re.findall(r"\b(p2pb_\w+)\s*\(", src)) if s.startswith("p2pb_scan_"))
    assert declared == sorted(SCAN)
    assert sorted(s for s in _lib.SYMBOLS if s.startswith("p2pb_scan_")) == sorted(SCAN)
    so = ctypes.CDLL(_lib.LIB_PATH)
    for s in SCAN:
        assert hasattr(so, s), s
    assert so.p2pb_scan_big_chunk_rows() >= 256


def test_abi_numbers_are_still_13_and_the_header_says_why():
    from p2p_bridge_amd import _lib

    text = open(HDR).read()
    assert int(re.search(r"#define\s+P2PB_ABI_VERSION\s+(\d+)", text).group(1)) == 13 and _lib.ABI_VERSION == 13
    assert ctypes.CDLL(_lib.LIB_PATH).p2pb_version() == 13
    assert re.search(r"p2pb_scan_\*[^;]*WITHOUT a bump", text)


def test_null_and_bad_sizes_are_refused_before_any_launch():
    from p2p_bridge_amd import _lib

    so, null = _lib.lib(), ctypes.c_void_p(0)
    assert so.p2pb_scan_depth_valid(0, null, ctypes.c_float(0.1), ctypes.c_float(1.0), null, null) == -22
    assert so.p2pb_scan_cell_keys(4, null, ctypes.c_float(0.1), null, null, null) == -22
    assert so.p2pb_scan_knn_grid(4, 4, 65, 3, null, null, null, null, ctypes.c_float(0.1), null, null, null) == -22
    assert so.p2pb_scan_knn_brute(4, 3, 4, null, null, null, null, null) == -22


def test_command_line_options_equal_the_reference(golden_dir):
    want = json.load(open(os.path.join(golden_dir, "scan_fusion_options.json")))["options"]
    actions = {a.dest: a for a in SF.build_parser()._actions if a.dest != "help"}
    assert sorted(actions) == sorted(want)
    for name, spec in want.items():
        a = actions[name]
        assert a.option_strings == ["--" + name]
        assert a.default == spec["default"], name
        assert bool(a.required) == bool(spec.get("required", False)), name
        if spec["type"] == "flag":
            assert a.nargs == 0 and a.const is True, name
        else:
            assert a.type is {"str": str, "int": int, "float": float}[spec["type"]], name
    assert vars(SF.default_args(grid_size=0.05))["grid_size"] == 0.05
    with pytest.raises(TypeError):
        SF.default_args(no_such_option=1)


def test_ply_round_trip_through_the_package_reader(tmp_path):
    from p2p_bridge_amd.evaluate_rooms import read_cloud, read_ply

    rng = np.random.default_rng(0)
    pts = rng.normal(size=(257, 3)).astype(np.float32)
    rgb = rng.uniform(0, 255, (257, 3)).astype(np.float32)
    path = str(tmp_path / "iphone.ply")
    SF.write_ply(path, torch.from_numpy(pts), torch.from_numpy(rgb))
    assert np.array_equal(read_cloud(path), pts.astype(np.float64))
    assert read_ply(path)["faces"] is None
    head, body = open(path, "rb").read().split(b"end_header\n")
    assert b"property uchar red" in head and len(body) == 257 * 15
    rec = np.frombuffer(body, dtype=[("xyz", "<f4", 3), ("rgb", "u1", 3)])
    assert np.array_equal(rec["rgb"], np.floor(rgb).astype(np.uint8))
    SF.write_ply(path, pts[:0])
    assert read_cloud(path).shape == (0, 3)


def test_cpu_tensors_raise():
    x = torch.zeros(30, 3)
    for fn in (lambda: SF.voxel_down_sample(x, 0.1), lambda: SF.remove_radius_outliers(x, 3, 0.1),
               lambda: SF.knn_kth_distance(x, x, 2), lambda: SF.outlier_removal(x, 3, 0.1),
               lambda: SF.filter_iphone_scan(x, x),
               lambda: SF.backproject(torch.zeros(4, 4, 3, dtype=torch.uint8), torch.ones(4, 4), np.eye(4), np.eye(3))):
        with pytest.raises(RuntimeError):
            fn()


def test_restatement_on_the_lattice():
    """6^3 lattice of spacing 2^-2: at r = 2^-2 an interior point has itself and six neighbours"""
    g = np.arange(6, dtype=np.float32) * 0.25
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    # the margin rule leaves the lattice's exact ties out: decide at the two radii
    lo, sure = scan_ref.radius_decisions(pts, 7, 0.25)
    assert not sure.any() or lo[sure].sum() == 0  # at r(1 - 1e-6) no neighbour is reached
    keep, sure = scan_ref.radius_decisions(pts, 7, 0.25 * (1 + 1e-5))
    inner = np.all((pts > 0.1) & (pts < 1.2), axis=1)
    assert sure.all() and np.array_equal(keep, inner) and inner.sum() == 64
    kth = scan_ref.kth_distance(pts, pts, 2)
    assert np.allclose(kth, 0.25) and np.all(scan_ref.kth_distance(pts, pts, 1) == 0)
    keys, (mean,) = scan_ref.voxel_means(pts, 0.5)
    assert len(keys) == 27 and np.array_equal(keys[0], [0, 0, 0]) and np.allclose(mean[0], 0.125)
    assert np.array_equal(scan_ref.voxel_means(np.array([[-0.001, 0.0, 0.05]], np.float32), 0.05)[0], [[-1, 0, 1]])


def test_room_generator_is_seeded_and_fp32():
    a, b = scan_ref.room(2000, 3), scan_ref.room(2000, 3)
    assert a.dtype == np.float32 and a.shape == (2000, 3) and np.array_equal(a, b)
    assert not np.array_equal(a, scan_ref.room(2000, 4))
    near_face = np.min(np.minimum(np.abs(a[100:]), np.abs(a[100:] - np.array([1.0, 0.8, 0.6], np.float32))), axis=1)
    assert np.percentile(near_face, 99) < 0.02  # all but the clutter lie on the faces
