"""The parts of the point-to-mesh grid that need no GPU: the planner, the declared and exported symbols, the `method` argument."""
import ctypes
import itertools
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["p2pb_p2m_grid_classify", "p2pb_p2m_grid_count", "p2pb_p2m_grid_fill", "p2pb_p2m_grid_point_face",
       "p2pb_p2m_grid_face_point", "p2pb_p2m_point_face_subset", "p2pb_p2m_face_point_subset"]


def test_planner_is_deterministic_positive_and_monotone():
    from p2p_bridge_amd import p2m_grid as G

    boxes = [((-1, -1, -1), (1, 1, 1)), ((0, 0, 0), (0, 0, 0)), ((100, 50, 0), (101, 51, 1)), ((-1e-9, 0, 0), (1e-9, 0, 0)),
             ((-2e5, 0, 0), (0, 1e5, 1))]
    for (lo, hi), T, med in itertools.product(boxes, (1, 12, 1000, 2_000_000), (0.0, 1e-9, 0.004, 0.5, 30.0)):
        p = G.plan_triangle_grid(lo, hi, T, med)
        assert p == G.plan_triangle_grid(lo, hi, T, med)  # a pure function
        assert p.cell > 0 and p.mag > 0 and p.usable
        assert 1 <= p.max_ring <= 8 and p.cap >= 8 and p.max_cols >= 9
        assert max(abs(v) for v in lo + hi) / p.cell <= 2 ** 18  # every coordinate within mag / 4 keys inside the range
        assert 4 * max(abs(v) for v in lo + hi) / p.cell <= G.KEY_HALF
        assert p.max_incidences == G.INCIDENCES_PER_TRIANGLE * T + 1024  # the stated constant, nothing else
        assert p.cell >= 2 * med  # a typical box overlaps at most 2 cells per axis
    # monotone: a larger mesh never gets a smaller workspace bound, nor one above the stated constant per triangle
    for P in (1, 1000, 3_000_000):
        prev = -1
        for T in (1, 2, 64, 1000, 200_000, 3_000_000):
            b = G.workspace_bound_bytes(P, T)
            assert b > prev and b <= 24 * P + (42 + 12 * G.INCIDENCES_PER_TRIANGLE) * T + 12 * 1024
            prev = b
        assert G.workspace_bound_bytes(P + 1, 1000) > G.workspace_bound_bytes(P, 1000)
    # coordinates the fp32 bounds were not argued for: the plan says so (the index then runs the brute force) and still
    # returns a positive cell
    for lo, hi in (((-1e7, 0, 0), (1e7, 1, 1)), ((0, 0, 0), (float("inf"), 1, 1)), ((float("nan"), 0, 0), (1, 1, 1))):
        p = G.plan_triangle_grid(lo, hi, 100, 0.01)
        assert not p.usable and p.cell > 0


def test_new_symbols_in_header_binding_and_library():
    from p2p_bridge_amd import _lib, build

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "p2pb_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(p2pb_\w+)\s*\(", src))
    build.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert s in declared and s in _lib.SYMBOLS and hasattr(lib, s), s
    assert "point-to-mesh grid" in open(os.path.join(ROOT, "include", "p2pb_hip.h")).read()
    assert _lib.ABI_VERSION == 13 and lib.p2pb_version() == 13  # pure additions


def test_pair_function_is_stated_once():
    csrc = os.path.join(ROOT, "p2p_bridge_amd", "csrc")
    hits = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))
            and re.search(r"float\s+point_triangle_d2\s*\(", open(os.path.join(csrc, f)).read())]
    assert hits == ["p2m_geom.h"]
    for f in ("p2m.hip", "p2m_grid.hip"):
        assert '#include "p2m_geom.h"' in open(os.path.join(csrc, f)).read()


def test_cell_grid_and_wave_best_list_are_stated_once():
    """the key packing and the cell quotient -- what the writers and the readers of sorted cell keys must agree on bit for
    bit -- and the wave's sorted best list each live in one header that their users include"""
    csrc = os.path.join(ROOT, "p2p_bridge_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))}
    for needle in ("<< 42", "floorf(__fdiv_rn("):
        assert [f for f, t in text.items() if needle in t] == ["cell_grid.h"], needle
    for f in ("scan.hip", "p2m_grid.hip"):
        assert '#include "cell_grid.h"' in text[f]
    # the list's mark: a position counted by ballot, the shift by __shfl_up
    lists = [f for f, t in text.items() if "__shfl_up(" in t and re.search(r"__popcll\(__ballot\([^;]*<=", t)]
    assert lists == ["wave_topk.h"]
    assert [f for f, t in text.items() if re.search(r"struct\s+WaveTopk\b", t)] == ["wave_topk.h"]
    for f in ("scan.hip", "pairs.hip"):
        assert '#include "wave_topk.h"' in text[f] and "WaveTopk<" in text[f]


def test_method_argument_rejects_unknown_values():
    from p2p_bridge_amd import metrics as M

    pts, tris = torch.zeros(4, 3), torch.rand(2, 3, 3)
    verts, faces = torch.rand(5, 3), torch.tensor([[0, 1, 2], [2, 3, 4]])
    for fn in (M.point_face_distance, M.face_point_distance):
        with pytest.raises(ValueError, match="method"):
            fn(pts, tris, method="kdtree")
        with pytest.raises(ValueError):
            fn(pts, tris, method="brute", return_stats=True)
    with pytest.raises(ValueError, match="method"):
        M.point_mesh_face_distance(pts, verts, faces, method="")
    with pytest.raises(ValueError, match="method"):
        M.point_mesh_bidir_distance_single_unit_sphere(pts, verts, faces, method="Grid")
    assert M.TriangleGrid.__name__ == "TriangleGrid" and callable(M.plan_triangle_grid)
