"""The poisoned arena's own tests (oracle/poison_arena.py), on CPU tensors: the carve contract, and that every kind of
violation the GPU tests rely on it to see IS seen -- each one planted with a plain torch write through the arena's
base tensor."""
import re

import pytest
import torch

from oracle.poison_arena import ALIGN, PATCHED, POISON, RESERVE, GuardViolation, PoisonArena

SIZE = 4 << 20
FLOATS = [torch.float32, torch.float64, torch.float16, torch.bfloat16]


def _originals():
    return [getattr(torch if o == "torch" else torch.Tensor, n) for o, n in PATCHED]


def _rec(arena, t):
    assert t.untyped_storage().data_ptr() == arena.base.untyped_storage().data_ptr()
    (r,) = [r for r in arena.records if r["start"] == t.storage_offset() * t.element_size() and r["shape"] == tuple(t.shape)]
    return r


def test_carved_tensors_are_contiguous_aligned_and_poisoned():
    with PoisonArena("cpu", SIZE) as arena:
        src = torch.ones(3, 5)  # (torch.ones is not patched: its storage is the allocator's)
        made = [torch.empty(7, 3), torch.empty((2, 5), dtype=torch.int32), torch.empty(size=(4,), dtype=torch.float64),
                torch.empty(13, dtype=torch.uint8, device="cpu"), torch.empty_like(src), src.new_empty(6, 2),
                src.new_empty((3,), dtype=torch.int64), torch.empty(0), torch.empty(2, 3, 4, 5, 6, memory_format=torch.channels_last_3d)]
        assert arena.n_allocations == len(made)
        for t, shape in zip(made, [(7, 3), (2, 5), (4,), (13,), (3, 5), (6, 2), (3,), (0,), (2, 3, 4, 5, 6)]):
            assert tuple(t.shape) == shape and t.device.type == "cpu"
            assert t.data_ptr() % ALIGN == 0 or t.numel() == 0
            r = _rec(arena, t)
            assert r["end"] - r["start"] == t.numel() * t.element_size()  # no rounding: the guard starts at the last byte
            assert "test_poison_arena.py:" in r["where"]
            assert bool((arena.base[r["start"]:r["end"]] == POISON).all())
        assert all(t.is_contiguous() for t in made[:-1])
        assert made[-1].is_contiguous(memory_format=torch.channels_last_3d)
        # [guard | payload | guard]: at least a guard between any two payloads, before the first and after the last
        spans = sorted((r["start"], r["end"]) for r in arena.records)
        assert spans[0][0] >= arena.guard
        assert all(b[0] - a[1] >= arena.guard for a, b in zip(spans, spans[1:]))
        assert spans[-1][1] + arena.guard + RESERVE <= arena.nbytes
        arena.check_guards()
        # a carved tensor is no autograd view of the base: in-place writes to one leave another's version alone
        v = made[0]._version
        made[1].fill_(3)
        assert made[0]._version == v


@pytest.mark.parametrize("dtype", FLOATS + [torch.int32, torch.int64])
def test_poison_reads_as_nan_or_minus_one(dtype):
    with PoisonArena("cpu", SIZE) as arena:
        t = torch.empty(33, dtype=dtype)
        if dtype in FLOATS:
            assert bool(torch.isnan(t).all())
            with pytest.raises(AssertionError, match="33 of 33"):
                arena.assert_written(t, "t")
        else:
            assert bool((t == -1).all())
            arena.assert_written(t, "t")  # integers: held by equality with the oracle, not here


def test_zeros_are_zero_inside_and_poison_outside():
    with PoisonArena("cpu", SIZE) as arena:
        src = torch.ones(3, 5, dtype=torch.float64)
        for t in (torch.zeros(5, 3), torch.zeros_like(src), src.new_zeros(7), torch.zeros((2, 2), dtype=torch.int32)):
            assert bool((t == 0).all())
            r = _rec(arena, t)
            assert bool((arena.base[r["start"] - arena.guard:r["start"]] == POISON).all())
            assert bool((arena.base[r["end"]:r["end"] + arena.guard] == POISON).all())
        assert torch.zeros_like(src).dtype == torch.float64 and src.new_zeros(7).dtype == torch.float64
        arena.check_guards()


def test_requires_grad_and_autograd_through_a_carved_tensor():
    with PoisonArena("cpu", SIZE):
        w = torch.zeros(4, requires_grad=True)
        assert w.is_leaf and w.requires_grad
        y = torch.empty(4)
        y.copy_(w * 2 + 1)
        y.sum().backward()
        assert torch.equal(w.grad, torch.full((4,), 2.0))


def test_other_devices_and_inactive_calls_pass_through():
    before = _originals()
    with PoisonArena("cpu", SIZE) as arena:
        m = torch.empty(4, device="meta")
        assert m.device.type == "meta" and torch.zeros_like(m).device.type == "meta"
        assert m.new_empty(3).device.type == "meta" and torch.empty_like(torch.ones(2), device="meta").device.type == "meta"
        assert arena.n_allocations == 0
        out = torch.ones(3)
        torch.zeros(3, out=out)  # an explicit destination is the caller's memory
        assert arena.n_allocations == 0 and bool((out == 0).all())
    assert _originals() == before
    lo, hi = arena.base.data_ptr(), arena.base.data_ptr() + arena.nbytes
    t = torch.empty(5)
    assert not lo <= t.data_ptr() < hi and arena.n_allocations == 0


def test_patches_are_restored_after_an_exception_and_arenas_do_not_nest():
    before = _originals()
    own = {n: n in vars(torch.Tensor) for o, n in PATCHED if o == "Tensor"}
    with pytest.raises(KeyError):
        with PoisonArena("cpu", SIZE):
            assert _originals() != before
            with pytest.raises(RuntimeError, match="already active"):
                PoisonArena("cpu", SIZE).__enter__()
            raise KeyError("boom")
    assert _originals() == before
    assert own == {n: n in vars(torch.Tensor) for o, n in PATCHED if o == "Tensor"}


def test_arena_refuses_to_hand_out_its_reserve():
    with PoisonArena("cpu", SIZE) as arena:
        with pytest.raises(MemoryError, match="full"):
            torch.empty(SIZE - RESERVE)
        assert arena.n_allocations == 0
    with pytest.raises(ValueError):
        PoisonArena("cpu", RESERVE)


def _violation(arena):
    with pytest.raises(GuardViolation) as e:
        arena.check_guards()
    arena.check_guards()  # the failed check re-armed the guards
    return str(e.value)


def test_one_element_overrun_is_caught_and_named():
    with PoisonArena("cpu", SIZE) as arena:
        torch.empty(100)
        t = torch.empty(5, 7, dtype=torch.float32)  # 140 bytes: ends off every alignment boundary but the element's
        torch.empty(9)
        r = _rec(arena, t)
        arena.base[r["end"]:r["end"] + 4].view(torch.float32)[0] = 1.0  # t.flatten()[35]
        msg = _violation(arena)
        assert "(5, 7) float32" in msg and re.search(r"first damaged byte at \+[1-4] bytes", msg), msg
        assert re.search(r"last damaged byte at \+4 bytes", msg) and "test_poison_arena.py:" in msg, msg


def test_one_element_underrun_is_caught_and_named():
    with PoisonArena("cpu", SIZE) as arena:
        torch.empty(100)
        t = torch.empty(35, dtype=torch.int32)
        r = _rec(arena, t)
        arena.base[r["start"] - 4:r["start"]].view(torch.int32)[0] = 7  # t[-1]
        msg = _violation(arena)
        assert "(35,) int32" in msg and "first damaged byte at -4 bytes" in msg and "last damaged byte at -1 bytes" in msg, msg


def test_write_into_the_tail_reserve_is_caught():
    with PoisonArena("cpu", SIZE) as arena:
        torch.empty(3)
        t = torch.empty(11, dtype=torch.float64)
        arena.base[arena.nbytes - 8:].view(torch.float64)[0] = 0.0
        msg = _violation(arena)
        r = _rec(arena, t)
        assert "tail reserve" in msg and f"+{arena.nbytes - 8 - r['end'] + 1} bytes" in msg and "(11,) float64" in msg, msg


def test_guard_check_is_on_the_byte_value():
    """a stray write of 0xFF itself is the one write the check cannot see (asserted, so that the limit is on record); any
    other value in a single byte is seen"""
    with PoisonArena("cpu", SIZE) as arena:
        t = torch.empty(4, dtype=torch.uint8)
        r = _rec(arena, t)
        arena.base[r["end"]:r["end"] + 8] = 0xFF  # eight stray bytes of the poison value: invisible
        arena.base[r["start"] - 1] = 0xFF
        arena.check_guards()
        arena.base[r["end"]] = 0xFE
        assert "+1 bytes" in _violation(arena)


def test_assert_written_catches_one_unwritten_element():
    with PoisonArena("cpu", SIZE) as arena:
        for dtype in FLOATS:
            t = torch.empty(6, 50, dtype=dtype)
            t.view(-1)[:299] = 1.0  # everything but the last element of the last row
            with pytest.raises(AssertionError, match=r"1 of 300 .*first at \(5, 49\)"):
                arena.assert_written(t, "t")
            t.view(-1)[299] = 1.0
            arena.assert_written(t, "t")
        arena.check_guards()


def test_nan_next_to_a_put_input_reaches_an_over_reading_result():
    with PoisonArena("cpu", SIZE) as arena:
        host = torch.arange(1.0, 8.0)  # 7 floats: 28 bytes, not a multiple of 16
        x = arena.put(host)
        assert torch.equal(x, host) and x.data_ptr() % ALIGN == 0 and arena.n_allocations == 1
        r = _rec(arena, x)
        honest = torch.empty(1)
        honest[0] = x.sum()
        arena.assert_written(honest, "sum of 7")
        # a "kernel" that loads two float4s for 7 floats and keeps the eighth lane
        wide = arena.base[r["start"]:r["start"] + 32].view(torch.float32)
        greedy = torch.empty(1)
        greedy[0] = wide.sum()
        with pytest.raises(AssertionError, match="NaN"):
            arena.assert_written(greedy, "sum of 8")
        before = arena.base[r["start"] - 4:r["start"]].view(torch.float32)  # and the element before the input
        assert bool(torch.isnan(before).all())
        idx = arena.put(torch.tensor([3, 1, 2], dtype=torch.int32))
        ri = _rec(arena, idx)
        assert int(arena.base[ri["end"]:ri["end"] + 4].view(torch.int32)[0]) == -1  # an over-read index is -1, not huge
        arena.check_guards()  # reading disturbs nothing
