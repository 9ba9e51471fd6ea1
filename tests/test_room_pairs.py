"""Room training pairs without a GPU: the numpy restatements of tests/pairs_ref.py against the reference's recorded outputs
(tests/golden/room_pairs.npz, tools/make_golden_room_pairs.py), and the host logic of p2p_bridge_amd/room_pairs.py."""
import json
import os
import zlib

import numpy as np
import pytest

import pairs_ref
from p2p_bridge_amd import evaluate_rooms, room_pairs, scan_fusion


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "room_pairs.npz"))


def _sets(golden):
    return [tuple(x) for x in json.loads(str(golden["assign_sets"]))]


def _lists(golden, n):
    kind, s, k, m = _sets(golden)[n]
    nn = pairs_ref.assign_lists(kind, s, k, m, seed=n)
    assert zlib.crc32(np.ascontiguousarray(nn).tobytes()) == int(golden[f"assign_{n}_crc"]), "the list generator has changed"
    return nn, m


@pytest.mark.parametrize("n", range(7))
def test_restated_assignment_equals_the_reference(golden, n):
    nn, _ = _lists(golden, n)
    assert np.array_equal(pairs_ref.sequential_assign(nn), golden[f"assign_{n}"])


@pytest.mark.parametrize("n", range(7))
def test_deferred_acceptance_model_equals_the_sequential_rule(golden, n):
    nn, m = _lists(golden, n)
    got, rounds = pairs_ref.deferred_acceptance(nn, m)
    assert np.array_equal(got, golden[f"assign_{n}"])
    kind, s, k, _ = _sets(golden)[n]
    if kind == "identical":  # everybody wants the same K entries: one is settled per round, the last round moves nobody
        assert rounds == k + 1 and int((got == 0).sum()) == 1 + s - k
    assert rounds <= s * k


def test_parser_defaults_equal_the_reference(golden_dir):
    want = json.load(open(os.path.join(golden_dir, "room_pairs_options.json")))
    ap = room_pairs.build_parser()
    got = {a.dest: a.default for a in ap._actions if a.dest != "help"}
    got["required"] = sorted(a.dest for a in ap._actions if a.required)
    assert got == want


def test_skip_rules():
    clean = [256, 255, 256, 1000, 0, 256]
    noisy = [32, 500, 31, 256, 300, 255]
    kept, skipped = room_pairs.plan_patches(clean, noisy, 256)
    assert kept == [0, 3, 5] and skipped == 3  # 1 and 4: too few clean points; 2: fewer than npoints // 8 noisy ones
    assert room_pairs.plan_patches([9], [1], 9) == ([0], 0)  # 9 // 8 == 1


def test_pad_draws_follow_the_reference_order():
    patch = np.random.default_rng(0).uniform(-1, 1, (40, 3)).astype(np.float32)
    np.random.seed(42)
    rand_idx, extra = room_pairs.pad_draws(patch, 64)
    after = np.random.randint(0, 1 << 30)
    np.random.seed(42)  # the reference: randint first, then normal with the fp64 diagonal, added in fp64
    want_idx = np.random.randint(0, 40, 24)
    p64 = patch.astype(np.float64)
    diagonal = np.linalg.norm(np.max(p64, axis=0) - np.min(p64, axis=0))
    want = p64[want_idx] + np.random.normal(0, 1e-2 * diagonal, (24, 3))
    assert after == np.random.randint(0, 1 << 30)  # nothing else was drawn
    assert np.array_equal(rand_idx, want_idx) and extra.dtype == np.float32 and np.array_equal(extra, want.astype(np.float32))


def test_pad_draws_reproduce_the_fixture(golden):
    """the recorded patches were padded by the reference after np.random.seed(42): the same draws, patch after patch"""
    noisy = golden["pcd_noisy"]
    np.random.seed(int(golden["seed"]))
    for j in range(int(golden["n_kept"])):
        idxs = golden[f"patch{j}_idxs"]
        L = int(np.flatnonzero(np.diff(idxs) < 0)[0]) + 1  # the radius list is ascending, the duplicates start below its end
        rand_idx, extra = room_pairs.pad_draws(noisy[idxs[:L]], int(golden["npoints"]))
        assert np.array_equal(idxs[L:], idxs[:L][rand_idx])
        want = golden[f"patch{j}_noisy"][L:, :3] * golden[f"patch{j}_scale"] + golden[f"patch{j}_center"]
        assert np.abs(extra - want).max() <= pairs_ref.ulp32(np.abs(want).max())


def test_chunks_stay_under_the_budget():
    runs = room_pairs.chunk_patches(300, 4096, 128, 256 << 20)
    assert runs[0] == (0, 128) and runs[-1] == (256, 300) and all(hi - lo <= 128 for lo, hi in runs)
    assert room_pairs.chunk_patches(3, 4096, 128, 1) == [(0, 1), (1, 2), (2, 3)]
    assert room_pairs.chunk_patches(70000, 16, 16, 256 << 20) == [(0, 65535), (65535, 70000)]  # one launch's patch limit


def test_read_ply_colors_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    pts = rng.normal(size=(50, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (50, 3)).astype(np.uint8)
    path = str(tmp_path / "c.ply")
    scan_fusion.write_ply(path, pts, rgb)
    plain = evaluate_rooms.read_ply(path)
    assert sorted(plain) == ["faces", "points"]  # the default dict is unchanged
    got = evaluate_rooms.read_ply(path, colors=True)
    assert np.array_equal(got["points"], pts.astype(np.float64)) and got["faces"] is None
    assert np.array_equal(got["colors"], rgb / 255.0)
    with open(str(tmp_path / "a.ply"), "w") as f:  # ascii, float colours, one face
        f.write("ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
                "property float red\nproperty float green\nproperty float blue\nelement face 1\n"
                "property list uchar int vertex_indices\nend_header\n0 0 0 0.5 0.25 1\n1 0 0 0 0 0\n0 1 0 1 1 1\n3 0 1 2\n")
    got = evaluate_rooms.read_ply(str(tmp_path / "a.ply"), colors=True)
    assert np.array_equal(got["colors"], [[0.5, 0.25, 1], [0, 0, 0], [1, 1, 1]]) and got["faces"].tolist() == [[0, 1, 2]]
    with open(str(tmp_path / "n.ply"), "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nend_header\n0 0 0\n")
    assert evaluate_rooms.read_ply(str(tmp_path / "n.ply"), colors=True)["colors"] is None


def test_restatements_on_hand_made_cases():
    assert pairs_ref.sequential_assign([[0, 1], [0, 1], [0, 1], [2, 0]]).tolist() == [0, 1, 0, 2]
    q = np.zeros((1, 3), dtype=np.float32)
    ref = np.array([[1, 0, 0], [0, 1, 0], [0.5, 0, 0], [0, 0, 1]], dtype=np.float32)
    assert pairs_ref.knn_brute(q, ref, 3)[0].tolist() == [[2, 0, 1]]  # ties by ascending index
    cdf = np.array([0.5, 1.0, 1.0, 2.0])
    u = np.array([[0.0, 1.0, 0.0], [0.25, 1.0, 1.0], [0.5, 0.0, 0.5]])
    verts = np.eye(3)
    face, xyz, _ = pairs_ref.sample_mesh(verts, np.tile([[0, 1, 2]], (4, 1)), cdf, u)
    assert face.tolist() == [0, 1, 3]  # a value on a boundary goes to the next triangle with area, never to the empty one
    assert xyz.tolist() == [[0, 1, 0], [0, 0, 1], [1, 0, 0]]
