"""What the synthetic occupancies of oracle/occupancy_patterns.py must cover for tests/test_conv_occupancy_gpu.py to mean
something: the per-brick counts at which the compact voxel convolution changes path (empty brick, a partial tile, exactly one
tile, whole tiles, one more / one less than whole tiles, a full brick) and every one of the 27 boundary classes both as a
computed output (inside D1) and as a written constant (outside D2). No GPU, no product code: a changed pattern that loses
coverage fails here."""
import pytest
import torch

from oracle import occupancy_patterns as op


@pytest.fixture(scope="module", params=op.RESOLUTIONS)
def case(request):
    r = request.param
    pats = op.patterns(r)
    return r, pats, op.reference_sets(torch.stack(list(pats.values())))


def test_pattern_names_and_shapes(case):
    r, pats, _ = case
    names = ["full", "corners", "faces", "edges", "single_111", "bern0.003", "bern0.05", "bern0.5", "checker2"]
    if r >= 16:
        names += ["brick_corner", "wall_w7", "wall_w6", "interior_box"]
    assert list(pats) == names
    for name, p in pats.items():
        assert p.dtype == torch.bool and tuple(p.shape) == (r, r, r), name
        assert p.any(), name
    again = op.patterns(r)
    assert all(torch.equal(pats[k], again[k]) for k in pats)  # fixed seeds
    assert pats["corners"].sum() == 8 and pats["faces"].sum() == 6 and pats["edges"].sum() == 3
    assert pats["corners"][0, 0, r - 1] and pats["faces"][r // 2, 0, r // 2] and pats["edges"][r - 1, r // 2, 0]
    assert pats["checker2"].sum() == (r // 2) ** 3 and pats["checker2"][0, 0, 0] and not pats["checker2"][1, 0, 0]


def test_reference_sets_by_hand():
    """the brick order, the local ids and the class index on a case worked by hand: voxel (3, 7, 7) at r = 16"""
    occ = op.patterns(16)["brick_corner"][None]
    s = op.reference_sets(occ)
    assert s.d1.sum() == 27 and s.d2.sum() == 125
    assert s.d1[0, 2:5, 6:9, 6:9].all() and s.d2[0, 1:6, 5:10, 5:10].all()
    # 16 bricks = 4 (bd) x 2 (bh) x 2 (bw); D1 = [2,4]^3 around (3,7,7): bd in {0,1}, bh, bw in {0,1}
    c1 = s.counts[0, 0].view(4, 2, 2)
    assert c1[0].tolist() == [[8, 4], [4, 2]] and c1[1].tolist() == [[4, 2], [2, 1]] and c1[2:].sum() == 0
    assert s.active[0, 0].view(4, 2, 2)[:2].all() and not s.active[0, 0].view(4, 2, 2)[2:].any()
    assert s.active[1, 0].view(4, 2, 2)[:2].all() and not s.active[1, 0].view(4, 2, 2)[2:].any()
    b = op.to_bricks(s.d1)[0, 0]  # brick 0: local ids of (2..3, 6..7, 6..7)
    assert sorted(b.nonzero().flatten().tolist()) == sorted((ld * 8 + lh) * 8 + lw for ld in (2, 3) for lh in (6, 7) for lw in (6, 7))
    assert s.cls[0, 0, 0] == 0 and s.cls[15, 15, 15] == 26 and s.cls[5, 5, 5] == 13 and s.cls[0, 3, 15] == 5 and s.cls[15, 0, 4] == 19
    # a corner voxel: nothing outside the grid is ever set
    s = op.reference_sets(op.patterns(8)["corners"][None])
    assert s.d1.sum() == 64 and s.d2.sum() == 8 * 27


@pytest.mark.parametrize("which", [0, 1], ids=["D1", "D2"])
def test_brick_counts_cover_the_tile_paths(case, which):
    r, pats, s = case
    have = set(s.counts[which].flatten().tolist())
    assert 0 in have
    assert any(1 <= c <= 31 for c in have), sorted(have)
    assert (64 if (r == 8 and which == 1) else 32) in have, sorted(have)
    assert any(c % 32 == 0 and 32 < c < 256 for c in have), sorted(have)
    if r >= 16:
        assert any(c % 32 == 1 for c in have), sorted(have)
        assert any(c % 32 == 31 for c in have), sorted(have)
    assert 256 in have


def test_every_boundary_class_is_computed_and_is_a_constant(case):
    r, pats, s = case
    cls = s.cls.expand_as(s.d1)
    assert set(cls[s.d1].tolist()) == set(range(27))
    assert set(cls[~s.d2].tolist()) == set(range(27))


def test_full_grid(case):
    r, pats, _ = case
    s = op.reference_sets(pats["full"][None])
    assert (s.counts == 256).all() and s.active.all() and s.d1.all() and s.d2.all()


def test_active_bricks_are_the_bricks_that_hold_a_set_voxel(case):
    """brick +- 1 / +- 2 in occupancy terms is the same set as 'holds a voxel of D1 / D2': two derivations, one answer"""
    r, pats, s = case
    assert torch.equal(s.active, s.counts > 0)
