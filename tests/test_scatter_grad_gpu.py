"""The scatter-add gradients -- trilinear_devoxelize_backward, grouping_backward(_pitched),
three_nearest_neighbors_interpolate_backward(_pitched), gather_features_backward -- against a float64 restatement of each adjoint
written here (gx[b, ch, idx] += w * gy with scatter_add_ on the CPU), on every kernel form of their dispatch and in both modes.

Forms: scat_grad (csrc/scatter_grad.hip, the one host function behind all of these entry points) rounds scat_rows(L, c, cap)
down to a power of two and launches scat_grad_lds_kernel<K, W, CH> with CH in {1, 2, 4, 8} (devoxelisation: and 16) rows per
workgroup, or the global-atomic scat_grad_kernel for rows beyond 128 KiB (form 0 here). `scat_rows` and that rule are restated
below, and the case tables are held to them where they are made: a table that stops reaching a form fails at import.

Inputs are built directly (indices and weights are arguments of these ops) and every index is in range. Outputs are carved from a
poisoned arena (oracle/poison_arena.py): an element that no kernel wrote is NaN, so "receives nothing -> exactly 0" checks the
kernels' own zero-fill, and a write outside the output fails the guard check.

  exact data   gy integers in [-8, 8], weights multiples of 1/64 in [0, 1]: every product and partial sum is a multiple of 1/64
               below 2^24 / 64 in magnitude while (contributions to one element) * 512 < 2^24 (asserted), hence exact in fp32 in
               ANY order: the result must equal the float64 reference bit for bit, in both modes and on the fallback.
  real data    gy ~ N(0, 1), weights uniform and normalised per point; |got - ref| <= (T_e + 2) * 2^-24 * S_e per element, with
               T_e the number of contributions and S_e the sum of |w * gy|: the worst case of fp32 products and fp32 adds in any
               order. The median |term| of a case is at least 4x its largest bound (asserted on the reference alone), so one
               dropped contribution cannot hide.

Measured on an MI355X: the 221 tests take 4.5 s in all; the slowest, 1.6 s, is the first one (it loads the library), every other
one is below 0.1 s. Worst |got - ref| / bound on real data, default / deterministic mode: devoxelisation 0.470 / 0.452, grouping 0.297 / 0.297, three-NN interpolation
0.477 / 0.448. Every exact-data case is bit equal, in both modes, pitched and on the fallback."""
import contextlib
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ARENA = 8 << 20

# ------------------------------------------------------------------------------------------------- the dispatch, restated

SCAT_LDS_MAX = 128 * 1024
OPS = ("devox", "group", "interp")
CAP = {"devox": 16, "group": 8, "interp": 8}
SLOTS = {"devox": 8, "group": 1, "interp": 3, "gather": 1}  # contributions per point: corners, -, neighbours, -
PATTERNS = ("uniform", "half0", "one", "dup", "zerow", "ends")


def scat_rows(L, c, cap):
    """csrc/scatter_grad.hip scat_rows: rows per workgroup -- what fits 64 KiB, at most cap and c; one row up to 128 KiB; 0 = no fit"""
    if L * 4 > SCAT_LDS_MAX:
        return 0
    return min(max((64 * 1024) // (L * 4), 1), cap, c)


def form(op, L, c):
    """the CH of the scat_grad_lds_kernel<K, W, CH> that scat_grad launches: scat_rows rounded down to a power of two; 0 = the
    global-atomic kernel"""
    ch = scat_rows(L, c, CAP[op])
    return 1 << (ch.bit_length() - 1) if ch else 0


# the two `switch` statements that this rule replaced (cap 16: 1 | 2, 3 | 4..7 | 16 | default; cap 8: 1 | 2, 3 | 8 | default) chose
# the same CH for every value scat_rows can return
for _ch in range(17):
    _p2 = 1 << (_ch.bit_length() - 1) if _ch else 0
    assert {0: 0, 1: 1, 2: 2, 3: 2, 4: 4, 5: 4, 6: 4, 7: 4, 16: 16}.get(_ch, 8) == _p2, _ch
    assert _ch > 8 or {0: 0, 1: 1, 2: 2, 3: 2, 8: 8}.get(_ch, 4) == _p2, _ch


FORMS = {"devox": (0, 1, 2, 4, 8, 16), "group": (0, 1, 2, 4, 8), "interp": (0, 1, 2, 4, 8)}

# (operator, B, c, L, points, pattern). L: r^3 | n | m, the length of a gradient row. points: n | (m, u) | n.
# A devoxelisation L that is a cube goes through the drop-in (which takes r), any other through the ABI (which takes r3).
_T = [
    ("devox", 2, 17, 343, 3000, "uniform"),    # 16, ragged (17 = 16 + 1), L % 4 = 3
    ("devox", 1, 16, 512, 2000, "dup"),        # 16, full workgroups, L % 4 = 0
    ("devox", 2, 11, 333, 2500, "half0"),      # 8 by c < cap, ragged
    ("devox", 1, 9, 2000, 2000, "ends"),       # 8 by L (8 rows in 64 KiB), ragged
    ("devox", 3, 6, 512, 3000, "one"),         # 4 by c, ragged
    ("devox", 2, 5, 4096, 2000, "zerow"),      # 4 by L (r = 16), ragged
    ("devox", 2, 3, 125, 2000, "uniform"),     # 2 by c (scat_rows = 3), ragged
    ("devox", 1, 5, 8000, 3000, "half0"),      # 2 by L (r = 20), ragged
    ("devox", 1, 3, 8191, 2000, "dup"),        # 2 by L, L % 4 = 3
    ("devox", 3, 1, 27, 1500, "zerow"),        # 1 by c = 1
    ("devox", 2, 3, 32768, 3000, "uniform"),   # 1: one row fills 128 KiB (r = 32)
    ("devox", 1, 2, 32767, 3000, "one"),       # 1, Lp = 32768 != L
    ("devox", 1, 2, 8193, 2000, "ends"),       # 1: the first L past two rows
    ("devox", 2, 17, 32769, 3000, "uniform"),  # fallback: the first L past the LDS; 17 = 16 + 1 channels per block
    ("devox", 1, 3, 35937, 2000, "half0"),     # fallback through the drop-in (r = 33)
    ("devox", 1, 5, 32769, 2000, "ends"),
    ("devox", 1, 2, 32769, 3000, "one"),
    ("devox", 2, 3, 32769, 2000, "zerow"),
    ("devox", 1, 3, 32769, 2000, "dup"),
    ("group", 2, 9, 333, (250, 8), "uniform"),     # 8, ragged, L % 4 = 1
    ("group", 1, 8, 2048, (125, 16), "dup"),       # 8: the last L with 8 rows in 64 KiB
    ("group", 2, 5, 4001, (1000, 3), "half0"),     # 4 by L, ragged, L % 4 = 1
    ("group", 3, 6, 100, (37, 64), "one"),         # 4 by c, ragged
    ("group", 2, 3, 8191, (500, 4), "ends"),       # 2 by L, ragged, L % 4 = 3
    ("group", 1, 3, 500, (2000, 1), "uniform"),    # 2 by c (scat_rows = 3)
    ("group", 1, 7, 5000, (300, 10), "uniform"),   # 2 by L (scat_rows = 3), ragged
    ("group", 3, 1, 64, (100, 20), "dup"),         # 1 by c = 1
    ("group", 2, 3, 32768, (750, 4), "uniform"),   # 1: one row fills 128 KiB
    ("group", 1, 2, 8193, (1500, 2), "half0"),     # 1: the first L past two rows
    ("group", 1, 2, 32767, (111, 27), "one"),      # 1, Lp = 32768 != L
    ("group", 2, 9, 32769, (250, 8), "uniform"),   # fallback; 9 = 8 + 1 channels per block
    ("group", 1, 3, 32769, (1000, 3), "ends"),
    ("group", 1, 2, 32769, (300, 10), "half0"),
    ("group", 1, 2, 32769, (111, 27), "one"),
    ("group", 2, 3, 32769, (125, 16), "dup"),
    ("interp", 2, 9, 333, 3000, "uniform"),     # 8, ragged, L % 4 = 1
    ("interp", 1, 8, 2048, 2000, "dup"),        # 8: the last L with 8 rows in 64 KiB
    ("interp", 2, 5, 4001, 3000, "half0"),      # 4 by L, ragged
    ("interp", 3, 6, 100, 2500, "one"),         # 4 by c, ragged
    ("interp", 2, 7, 4096, 2000, "zerow"),      # 4 by L, ragged, L % 4 = 0
    ("interp", 2, 3, 8191, 2000, "ends"),       # 2 by L, ragged, L % 4 = 3
    ("interp", 1, 3, 77, 3000, "uniform"),      # 2 by c (scat_rows = 3)
    ("interp", 1, 7, 5000, 2000, "zerow"),      # 2 by L (scat_rows = 3), ragged
    ("interp", 3, 1, 1, 1000, "uniform"),       # 1 by c = 1; one centre: every neighbour is centre 0
    ("interp", 2, 3, 32768, 3000, "uniform"),   # 1: one row fills 128 KiB
    ("interp", 1, 2, 8193, 3000, "half0"),      # 1: the first L past two rows
    ("interp", 1, 2, 32767, 4000, "one"),       # 1, Lp = 32768 != L
    ("interp", 2, 17, 32769, 3000, "uniform"),  # fallback; 17 = 16 + 1 channels per block
    ("interp", 1, 3, 32769, 2000, "ends"),
    ("interp", 1, 2, 32769, 2000, "half0"),
    ("interp", 1, 2, 32769, 4000, "one"),
    ("interp", 2, 3, 32769, 2000, "zerow"),
    ("interp", 1, 3, 32769, 2000, "dup"),
]
CASES = [dict(op=op, B=B, c=c, L=L, pts=pts, pat=pat, form=form(op, L, c)) for op, B, c, L, pts, pat in _T]


def _npts(c):
    return c["pts"][0] * c["pts"][1] if c["op"] == "group" else c["pts"]


def _cid(c):
    return f"{c['op']}-ch{c['form']}-B{c['B']}c{c['c']}L{c['L']}-{c['pat']}"


assert len({_cid(c) for c in CASES}) == len(CASES)
for _op in OPS:  # every (operator, form) pair, and what each form has to meet: checked where the table is made
    _sub = [c for c in CASES if c["op"] == _op]
    assert {c["form"] for c in _sub} == set(FORMS[_op]), _op
    for _f in FORMS[_op]:
        _of = [c for c in _sub if c["form"] == _f]
        assert _of, (_op, _f)
        assert any(c["B"] >= 2 for c in _of), (_op, _f)  # the pitched variants step from sample to sample
        if _f > 1:  # a ragged last workgroup (CH = 1 has none: every c is a multiple of 1)
            assert any(c["c"] % _f != 0 for c in _of), (_op, _f)
        if 0 < _f < CAP[_op]:  # scat_rows clipped by c (CH = cap needs c >= cap: it cannot be)
            assert any(scat_rows(c["L"], c["c"], CAP[_op]) == c["c"] < scat_rows(c["L"], 1 << 20, CAP[_op]) for c in _of), (_op, _f)
        if 0 < _f:  # ... and chosen by the row length alone
            assert any(scat_rows(c["L"], c["c"], CAP[_op]) == scat_rows(c["L"], 1 << 20, CAP[_op]) for c in _of), (_op, _f)
    _lds = [c for c in _sub if c["form"] > 0]
    assert any(c["L"] % 4 != 0 for c in _lds) and any(c["L"] % 4 == 0 for c in _lds), _op  # Lp != L, Lp == L
    assert {c["L"] % 4 for c in _lds} >= {0, 1, 3}, _op
    assert any(c["L"] == 32768 and c["form"] == 1 for c in _sub), _op  # the last row that fits
    assert any(c["L"] == 32769 and c["form"] == 0 for c in _sub), _op  # the first that does not
    _pats = set(PATTERNS) - ({"zerow"} if _op == "group" else set())  # grouping has no weights
    assert {c["pat"] for c in _sub} == _pats, _op
    assert {c["pat"] for c in _sub if c["form"] == 0} == _pats, _op  # the fallback's zero-fill and atomics meet each pattern too
    assert all(1 <= c["B"] <= 3 and c["c"] <= 24 and _npts(c) <= 4000 for c in _sub), _op
    assert all(c["B"] * c["c"] * c["L"] * 4 + (3 << 20) <= ARENA for c in _sub), _op

LDS_CASES = [c for c in CASES if c["form"] > 0]
MODE_CASES = [(c, det) for c in CASES for det in (False, True) if not (det and c["form"] == 0)]  # (fallback + deterministic: refused)
PITCH_CASES = [c for c in CASES if c["op"] != "devox" and c["B"] >= 2]
for _op in ("group", "interp"):
    assert {c["form"] for c in PITCH_CASES if c["op"] == _op} == set(FORMS[_op]), _op


def _mid(p):
    return _cid(p[0]) + ("-det" if p[1] else "-default")


# ------------------------------------------------------------------------------------------------- inputs and the reference

def _indices(pat, B, K, P, L, gen, group_u=None):
    """i32[B, K, P] in [0, L)"""
    idx = torch.randint(0, L, (B, K, P), generator=gen)
    if pat == "half0":  # half of all contributions on element 0
        idx[torch.rand(B, K, P, generator=gen) < 0.5] = 0
    elif pat == "one":  # every contribution of a sample on one element (another one per sample, none of them special)
        for b in range(B):
            idx[b] = (L // 3 + 7 * b) % L
    elif pat == "ends":  # only the first and the last element of the row
        idx = torch.randint(0, 2, (B, K, P), generator=gen) * (L - 1)
    elif pat == "dup":  # the same index twice inside one point: two corners, two neighbours, two members of one group
        if K > 1:
            idx[:, K - 1] = idx[:, 0]
        else:
            g = idx.view(B, P // group_u, group_u)
            g[:, :, group_u - 1] = g[:, :, 0]
    assert int(idx.min()) >= 0 and int(idx.max()) < L  # no case passes an index out of range
    return idx.int()


def _real_points(c):
    """points of the real-valued variant of a case: as many as keep the contributions per element at a few hundred"""
    K, L, P = SLOTS[c["op"]], c["L"], _npts(c)
    per = {"one": 512, "half0": 1024, "ends": 1024}.get(c["pat"], 128 * L)  # contributions in all
    return max(1, min(P, per // K))


@functools.lru_cache(maxsize=None)
def _data(i, exact):
    """(gy f32[B,c,P], idx i32[B,K,P], w f32[B,K,P] | None, ref f64[B,c,L], S f64[B,c,L], T f64[B,1,L], terms f64) of CASES[i],
    all on the CPU; computed once, shared by the modes and the pitched tests, never written to"""
    c = CASES[i]
    op, B, ch, L, pat = c["op"], c["B"], c["c"], c["L"], c["pat"]
    K = SLOTS[op]
    gen = torch.Generator().manual_seed(1000 + 2 * i + int(exact))
    if op == "group":
        m, u = c["pts"]
        if not exact:
            m = max(1, _real_points(c) // u)
        P = m * u
    else:
        P = _npts(c) if exact else _real_points(c)
    idx = _indices(pat, B, K, P, L, gen, group_u=c["pts"][1] if op == "group" else None)
    if exact:
        gy = torch.randint(-8, 9, (B, ch, P), generator=gen).float()
        w = torch.randint(0, 65, (B, K, P), generator=gen).float() / 64
        if pat == "zerow":
            w[torch.rand(B, K, P, generator=gen) < 0.3] = 0
            w[:, :, ::5] = 0  # and whole points without weight
    else:
        gy = torch.randn(B, ch, P, generator=gen)
        wd = torch.rand(B, K, P, generator=gen, dtype=torch.float64)
        if pat == "zerow":
            wd[torch.rand(B, K, P, generator=gen) < 0.1] = 0
            wd[:, 0] += (wd.sum(1) == 0)
        w = (wd / wd.sum(1, keepdim=True)).float()  # normalised over the 8 corners / 3 neighbours
    if op == "group":
        w = None
    terms = gy.double()[:, :, None, :] * (1.0 if w is None else w.double()[:, None])  # [B, c, K, P]
    terms = terms.expand(B, ch, K, P).reshape(B, ch, K * P)
    index = idx.long()[:, None].expand(B, ch, K, P).reshape(B, ch, K * P)
    ref = torch.zeros(B, ch, L, dtype=torch.float64).scatter_add_(2, index, terms)
    S = torch.zeros(B, ch, L, dtype=torch.float64).scatter_add_(2, index, terms.abs())
    T = torch.zeros(B, L, dtype=torch.float64).scatter_add_(1, idx.long().reshape(B, K * P), torch.ones(B, K * P, dtype=torch.float64))
    return gy, idx, w, ref, S, T[:, None], terms


# ------------------------------------------------------------------------------------------------- the calls

@contextlib.contextmanager
def _mode(det):
    """default or deterministic mode; the flag is 0 again afterwards, whatever happened inside"""
    import p2p_bridge_amd
    from p2p_bridge_amd._lib import lib

    assert lib().p2pb_get_deterministic() == 0
    try:
        if det:
            with p2p_bridge_amd.deterministic():
                assert lib().p2pb_get_deterministic() == 1
                yield
        else:
            yield
    finally:
        assert lib().p2pb_get_deterministic() == 0


def _devox(gy, inds, wgts, r3):
    import ctypes

    from p2p_bridge_amd import pointnet2_batch_cuda as pn2
    from p2p_bridge_amd._lib import call, ptr, stream_ptr

    r = round(r3 ** (1 / 3))
    if r ** 3 == r3:
        return pn2.trilinear_devoxelize_backward(gy, inds, wgts, r)
    b, c, n = gy.shape  # the drop-in takes r; the ABI any r3 (the arguments of pn2.trilinear_devoxelize_backward)
    gx = torch.empty(b, c, r3, dtype=torch.float32, device=gy.device)
    call("p2pb_trilinear_devoxelize_backward", ctypes.c_int(b), ctypes.c_int(c), ctypes.c_int(n), ctypes.c_int(r3), ptr(inds),
         ptr(wgts), ptr(gy), ptr(gx), stream_ptr())
    return gx


def _call(c, gy, idx, w, pitched=False):
    """one operator call on device tensors in the generic layout (gy [B,c,P], idx [B,K,P], w [B,K,P]) -> gx f32[B,c,L]"""
    from p2p_bridge_amd import pointnet2_batch_cuda as pn2

    op, L = c["op"], c["L"]
    if op == "devox":
        return _devox(gy, idx, w, L)
    if op == "group":
        B, ch, P = gy.shape
        u = c["pts"][1]
        f = pn2.grouping_backward_pitched if pitched else pn2.grouping_backward
        return f(gy.view(B, ch, P // u, u), idx.view(B, P // u, u), L)
    if op == "interp":
        f = pn2.three_nearest_neighbors_interpolate_backward_pitched if pitched else pn2.three_nearest_neighbors_interpolate_backward
        return f(gy, idx, w, L)
    return pn2.gather_features_backward(gy, idx[:, 0], L)


def _run(c, gy, idx, w, det=False, pitched=False, times=1):
    """`times` calls in a poisoned arena, in the mode asked for -> the results on the CPU"""
    from oracle.poison_arena import PoisonArena

    with PoisonArena(DEV, ARENA) as arena:
        with _mode(det):
            out = [_call(c, gy, idx, w, pitched) for _ in range(times)]
        arena.check_guards()  # nothing was written outside the outputs
        assert arena.n_allocations == times  # the outputs came from the arena: what no kernel wrote is NaN
    out = [o.cpu() for o in out]
    return out[0] if times == 1 else out


def _to_dev(gy, idx, w):
    return gy.to(DEV), idx.to(DEV), None if w is None else w.to(DEV)


def _first_diff(got, ref):
    bad = (got.double() != ref) | torch.isnan(got)
    where = bad.nonzero()
    if where.shape[0] == 0:
        return "equal"
    k = tuple(where[0].tolist())
    return f"{where.shape[0]} of {ref.numel()} elements differ, first at {k}: got {got[k].item()!r}, reference {ref[k].item()!r}"


# ------------------------------------------------------------------------------------------------- the tests

def _check_exact_inputs(c, T):
    assert float(T.max()) * 512 < 2 ** 24  # every partial sum is exact in fp32
    if c["pat"] in ("one", "ends") and c["L"] > 2:
        assert bool((T == 0).any())  # elements that receive nothing


@pytest.mark.parametrize("case_mode", MODE_CASES, ids=_mid)
def test_exact_data_is_bit_equal_to_fp64(case_mode):
    """integers times multiples of 1/64: bit equality with the float64 scatter-add in any summation order; untouched elements
    come out exactly 0 on a poisoned output buffer"""
    c, det = case_mode
    gy, idx, w, ref, _, T, _ = _data(CASES.index(c), True)
    _check_exact_inputs(c, T)
    got = _run(c, *_to_dev(gy, idx, w), det=det)
    assert got.dtype == torch.float32 and got.shape == ref.shape
    assert torch.equal(got.double(), ref), _first_diff(got, ref)
    assert bool((got[(T == 0).expand_as(got)] == 0).all())


@pytest.mark.parametrize("case_mode", MODE_CASES, ids=_mid)
def test_real_data_within_the_fp32_worst_case(case_mode):
    """|got - ref| <= (T_e + 2) * 2^-24 * S_e element-wise; in deterministic mode a second call gives the same bits"""
    c, det = case_mode
    gy, idx, w, ref, S, T, terms = _data(CASES.index(c), False)
    bound = (T + 2) * 2.0 ** -24 * S
    # on the reference alone: one dropped contribution cannot hide inside the bound
    assert float(terms.abs().median()) >= 4 * float(bound.max()), (float(terms.abs().median()), float(bound.max()), float(T.max()))
    got = _run(c, *_to_dev(gy, idx, w), det=det, times=2 if det else 1)
    if det:
        assert torch.equal(got[0], got[1])
        got = got[0]
    err = (got.double() - ref).abs()
    assert not bool(torch.isnan(got).any())
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{_mid(case_mode)}: T_max = {int(T.max())}, worst |got - ref| / bound = {ratio:.4f}, median |term| / largest bound = "
          f"{float(terms.abs().median()) / float(bound.max()):.0f}")
    assert bool((err <= bound).all()), ratio
    assert bool((got[(T == 0).expand_as(got)] == 0).all())


@pytest.mark.parametrize("lo", (0, 3))
@pytest.mark.parametrize("c", PITCH_CASES, ids=_cid)
def test_pitched_reads_a_channel_slice_in_place(c, lo):
    """gy = big[:, lo:hi] of a wider tensor whose other channels hold 1e6: the pitched variants equal the contiguous call and the
    float64 reference bit for bit, at every CH and on the fallback, in both modes"""
    from p2p_bridge_amd import pointnet2_batch_cuda as pn2

    gy, idx, w, ref, _, T, _ = _data(CASES.index(c), True)
    _check_exact_inputs(c, T)
    B, ch, P = gy.shape
    big = torch.full((B, lo + ch + 5, P), 1e6)
    big[:, lo:lo + ch] = gy
    big, idx_d, w_d = _to_dev(big, idx, w)
    sl = big[:, lo:lo + ch]
    assert not sl.is_contiguous() and pn2.sample_pitch(sl) == (lo + ch + 5) * P  # read in place, not through a copy
    plain = _run(c, sl.contiguous(), idx_d, w_d)
    for det in (False, True):
        if det and c["form"] == 0:
            continue  # (refused: test_deterministic_mode_refuses_rows_beyond_the_lds)
        got = _run(c, sl, idx_d, w_d, det=det, pitched=True)
        assert torch.equal(got, plain), (det, _first_diff(got, plain.double()))
        assert torch.equal(got.double(), ref), (det, _first_diff(got, ref))


@pytest.mark.parametrize("op", OPS)
def test_deterministic_mode_refuses_rows_beyond_the_lds(op):
    """L = 32769 under deterministic(): P2PB_EINVAL (devoxelisation through the drop-in: its worded error), the flag is restored,
    and the same inputs in default mode afterwards are right"""
    from p2p_bridge_amd._lib import P2PBError

    c = next(c for c in CASES if c["op"] == op and c["L"] == 32769)
    gy, idx, w, ref, _, _, _ = _data(CASES.index(c), True)
    dev = _to_dev(gy, idx, w)
    with pytest.raises(P2PBError, match=r"failed with code -22"):
        _run(c, *dev, det=True)
    if op != "devox":
        with pytest.raises(P2PBError, match=r"pitched failed with code -22"):
            _run(c, *dev, det=True, pitched=True)
    got = _run(c, *dev)
    assert torch.equal(got.double(), ref), _first_diff(got, ref)
    if op == "devox":  # r = 33: the drop-in's own words
        c = next(c for c in CASES if c["op"] == op and c["L"] == 33 ** 3)
        gy, idx, w, ref, _, _, _ = _data(CASES.index(c), True)
        dev = _to_dev(gy, idx, w)
        with pytest.raises(P2PBError, match=r"no deterministic kernel for r = 33 \(r\^3 = 35937"):
            _run(c, *dev, det=True)
        got = _run(c, *dev)
        assert torch.equal(got.double(), ref), _first_diff(got, ref)


GATHER = [dict(op="gather", B=2, c=5, L=333, pts=3000, pat="half0", form=None),   # duplicates on every element, heavy on 0
          dict(op="gather", B=3, c=3, L=4001, pts=1000, pat="uniform", form=None),  # duplicates and elements that receive nothing
          dict(op="gather", B=1, c=1, L=70000, pts=257, pat="ends", form=None)]     # two elements take everything


@pytest.mark.parametrize("c", GATHER, ids=_cid)
@pytest.mark.parametrize("det", (False, True), ids=("default", "det"))
def test_gather_features_backward_adds_on_duplicate_indices(c, det):
    """gather_features_backward is a global atomicAdd scatter: indices that repeat add up, the rest of the row is exactly 0"""
    B, ch, L, P = c["B"], c["c"], c["L"], c["pts"]
    gen = torch.Generator().manual_seed(77 + L)
    idx = _indices(c["pat"], B, 1, P, L, gen)
    gy = torch.randint(-8, 9, (B, ch, P), generator=gen).float()
    ref = torch.zeros(B, ch, L, dtype=torch.float64).scatter_add_(2, idx.long().expand(B, ch, P), gy.double())
    T = torch.zeros(B, L, dtype=torch.float64).scatter_add_(1, idx.long()[:, 0], torch.ones(B, P, dtype=torch.float64))
    assert float(T.max()) >= 2 and bool((T == 0).any()) and float(T.max()) * 512 < 2 ** 24
    got = _run(c, gy.to(DEV), idx.to(DEV), None, det=det)
    assert torch.equal(got.double(), ref), _first_diff(got, ref)
