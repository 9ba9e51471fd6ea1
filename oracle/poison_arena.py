"""Poisoned arena: test infrastructure that shows WHERE an operator reads and writes, not only what it computes.

    with PoisonArena("cuda:0", 64 << 20) as arena:
        x = arena.put(host_x)                # input with poison on both sides
        y = wrapper(x)                       # the wrapper's torch.empty / torch.zeros / ... are carved out of the arena
        arena.check_guards()                 # every byte outside the carved payloads is still 0xFF
        arena.assert_written(y, "y")         # no element of a floating-point result was left as it was handed out
        assert arena.n_allocations >= 1      # the wrapper really allocated through the patch

The arena is ONE uint8 tensor filled with the byte 0xFF. Every word of that fill is a quiet NaN in fp32, fp64, fp16 and
bf16 and -1 in int32 / int64: a result element that no kernel wrote is NaN, an input over-read reaches the result as
NaN, and a poisoned index is -1, never a large positive offset (which a NaN pattern such as 0x7FC00000 would be).
While the arena is active the Python-level allocation calls (PATCHED below) for its device return
[guard | payload | guard] slices of it: the payload starts on a 512-byte boundary (the caching allocator's own
alignment), the trailing guard at the payload's last byte without rounding, and the arena ends with a reserve that is
never handed out. Nothing here is meant to fault: a stray tile of a wrong kernel lands in memory the test owns.

What it cannot see: a write that lands inside ANOTHER live payload, an over-read whose value the kernel discards,
allocations made below Python (`.contiguous()`, `.cuda()`, arithmetic) and anything beyond guard / reserve.
Pure torch; importing it needs no GPU. Do not use it inside hipGraph capture (it synchronises and allocates).
"""
import os
import sys

import torch

POISON = 0xFF
ALIGN = 512  # the caching allocator's block alignment
RESERVE = 1 << 20  # never handed out: the arena's tail
PATCHED = (("torch", "empty"), ("torch", "empty_like"), ("torch", "zeros"), ("torch", "zeros_like"),
           ("Tensor", "new_empty"), ("Tensor", "new_zeros"))

_THIS = os.path.abspath(__file__)
_active = None


class GuardViolation(AssertionError):
    pass


def _caller():
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _THIS:
        f = f.f_back
    return "?" if f is None else f"{f.f_code.co_filename}:{f.f_lineno}"


def _norm_device(d):
    d = torch.device(d) if d is not None else (torch.get_default_device() if hasattr(torch, "get_default_device")
                                               else torch.device("cpu"))
    if d.type == "cuda" and d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return d


class PoisonArena:
    def __init__(self, device, nbytes, guard=16384):
        self.device = _norm_device(device)
        self.nbytes, self.guard = int(nbytes), int(guard)
        if self.nbytes < 2 * self.guard + RESERVE + ALIGN:
            raise ValueError(f"arena of {nbytes} bytes cannot hold two guards and its {RESERVE}-byte reserve")
        self.base = torch.full((self.nbytes,), POISON, dtype=torch.uint8, device=self.device)
        self._outside = torch.ones(self.nbytes, dtype=torch.bool, device=self.device)  # True: not inside any payload
        self._shift = (-self.base.data_ptr()) % ALIGN  # arena offsets o with (o - shift) % ALIGN == 0 are aligned addresses
        self._cursor = 0  # end of the last payload
        self.records = []  # dicts: shape, dtype, start, end (byte range of the payload), where (caller's file:line)
        self._saved = None

    # ---- carving ----------------------------------------------------------------------------------------------
    @property
    def n_allocations(self):
        return len(self.records)

    def _empty(self, *args, **kwargs):
        """torch.empty as it was before the patch, whether or not the arena is active"""
        return (torch.empty if self._saved is None else self._saved[("torch", "empty")][0])(*args, **kwargs)

    def _carve(self, shape, stride, dtype, where, zero=False):
        item = self._empty(0, dtype=dtype, device="cpu").element_size()
        numel = 1
        for s in shape:
            numel *= s
        span = 0 if numel == 0 else 1 + sum((s - 1) * st for s, st in zip(shape, stride))  # elements the strides reach
        nbytes = span * item
        start = self._cursor + self.guard
        start += (self._shift - start) % ALIGN
        end = start + nbytes
        if end + self.guard + RESERVE > self.nbytes:
            raise MemoryError(f"PoisonArena of {self.nbytes} bytes is full ({len(self.records)} allocations, next one "
                              f"{nbytes} bytes for {where}): raise the arena size for this case")
        self._cursor = end
        self._outside[start:end] = False
        self.records.append(dict(shape=tuple(shape), dtype=dtype, start=start, end=end, where=where))
        # not a view of self.base: a tensor of its own on the same storage, so that it has its own version counter
        # (autograd checks the saved tensors' versions; in-place writes to a sibling must not bump them)
        t = self._empty(0, dtype=dtype, device=self.device)
        t.set_(self.base.untyped_storage(), start // item, tuple(shape), tuple(stride))
        assert t.data_ptr() % ALIGN == 0 or nbytes == 0, (t.data_ptr(), start)
        if zero and nbytes:
            self.base[start:end].zero_()
        return t

    def put(self, t):
        """copy a (host) tensor into the arena between guards: poison lies directly before and behind its data"""
        t = t.detach()
        c = t.contiguous()
        out = self._carve(c.shape, c.stride(), c.dtype, _caller())
        out.copy_(c)
        return out

    def _alloc(self, key, args, kwargs, like=None):
        orig = self._saved[key][0]
        kw = dict(kwargs)
        dev = kw.get("device")
        if dev is None and like is not None:
            dev = like.device
        passthrough = (kw.get("out") is not None or kw.get("pin_memory") or kw.get("names") is not None
                       or kw.get("layout", torch.strided) is not torch.strided or _norm_device(dev) != self.device)
        if passthrough:
            return orig(*args, **kwargs)
        where = _caller()
        requires_grad = bool(kw.pop("requires_grad", False))
        kw.pop("pin_memory", None)
        kw["device"] = "meta"
        meta = orig(*args, **kw)  # torch's own parsing of sizes, dtype defaults and memory formats
        t = self._carve(meta.shape, meta.stride(), meta.dtype, where, zero=key[1] in ("zeros", "zeros_like", "new_zeros"))
        return t.requires_grad_() if requires_grad else t

    # ---- patching ---------------------------------------------------------------------------------------------
    def __enter__(self):
        global _active
        if _active is not None:
            raise RuntimeError("a PoisonArena is already active")
        owners = {"torch": torch, "Tensor": torch.Tensor}
        saved = {}
        for key in PATCHED:
            owner = owners[key[0]]
            saved[key] = (getattr(owner, key[1]), key[1] in vars(owner))
        self._saved = saved
        arena = self

        def module_fn(key, like):
            def fn(*args, **kwargs):
                return arena._alloc(key, args, kwargs, like=args[0] if like and args else kwargs.get("input"))
            fn.__name__ = key[1]
            return fn

        for key in PATCHED:
            setattr(owners[key[0]], key[1], module_fn(key, like=key[1].endswith("_like") or key[0] == "Tensor"))
        _active = self
        return self

    def __exit__(self, *exc):
        global _active
        owners = {"torch": torch, "Tensor": torch.Tensor}
        for key, (fn, own) in self._saved.items():
            if own:
                setattr(owners[key[0]], key[1], fn)
            else:
                delattr(owners[key[0]], key[1])  # it was inherited: drop our shadow
        self._saved = None
        _active = None
        return False

    # ---- checks -----------------------------------------------------------------------------------------------
    def _nearest(self, pos):
        """(record, signed offset): -k = k bytes before the payload's first byte, +k = k bytes past its last byte"""
        best = None
        for r in self.records:
            off = pos - r["start"] if pos < r["start"] else pos - r["end"] + 1
            if best is None or abs(off) < abs(best[1]):
                best = (r, off)
        return best

    def check_guards(self):
        """synchronise, then assert that every byte outside the carved payloads still holds the poison"""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        bad = (self.base != POISON) & self._outside  # one mask over the arena
        if not bool(bad.any()):
            return
        pos = bad.nonzero().flatten()
        first, last, count = int(pos[0]), int(pos[-1]), int(pos.numel())
        self.base[bad] = POISON  # re-arm: a later check reports later damage only
        msg = [f"{count} guard byte(s) of the arena were overwritten, arena offsets {first}..{last}"]
        if not self.records:
            msg.append("no allocation was made from the arena")
        for name, p in (("first", first), ("last", last)):
            near = self._nearest(p)
            if near is not None:
                r, off = near
                msg.append(f"{name} damaged byte at {off:+d} bytes from the allocation {tuple(r['shape'])} "
                           f"{str(r['dtype']).replace('torch.', '')} [{r['start']}, {r['end']}) made at {r['where']}"
                           + (" (in the arena's tail reserve)" if p >= self.nbytes - RESERVE else ""))
        raise GuardViolation("; ".join(msg))

    def assert_written(self, t, what):
        """a floating-point result holds no NaN: every element was written, from inputs that were not over-read
        (integer results are held by their equality with the oracle: the poison reads as -1)"""
        if not (t.is_floating_point() or t.is_complex()):
            return
        nan = torch.isnan(t)
        if bool(nan.any()):
            idx = nan.nonzero()
            raise AssertionError(f"{what}: {idx.shape[0]} of {t.numel()} elements of {tuple(t.shape)} are NaN (never "
                                 f"written, or computed from bytes outside an input), first at {tuple(idx[0].tolist())}, "
                                 f"last at {tuple(idx[-1].tolist())}")
