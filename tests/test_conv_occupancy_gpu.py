"""The sparse voxel convolutions and the voxeliser on occupancies a normalised cloud never produces (oracle/occupancy_patterns.py):
occupied voxels on the grid's corners, edges and faces, full bricks and a full grid, per-brick counts of exactly 0, 1, 32, 32k,
32k +- 1 and 256, and batches whose samples differ wildly (a full grid between eight corner voxels and a single voxel).
tests/test_occupancy_patterns.py (no GPU) states what the pattern set covers.

Grids are built on the host: x = randn * occ, cnt = occ. Every case runs a first convolution on x and a second one, in far-field
form, on its output; every test id names r, the channel counts (ragged / aligned / odd, below), the arithmetic, the form and the pattern (= the sample):

  lists       active_lists / brick_lists against reference_sets, exactly
  bits        compact, list-driven and the pre-split variants give the dense form's bits (outputs; statistics of the pre-split
              variants too; compact vs dense statistics within 1e-5)
  partial     listed_only / active_only: same bits inside the set, same statistics, NOTHING written outside (NaN-prefilled output)
  fp64        first convolution within the per-product bound of tests/test_conv_math_gpu.py (f16x3: 3 * 2^-22 + 2^-20, bf16x6
              and the exact-fp32 kernel: 2^-20, of conv(|x|, |w|) + |bias|); second convolution within 1e-4 of max |ref| over
              the sample AND within each of the 27 boundary classes on its own (max over the class's voxels on both sides)
  statistics  slot sums against the kernel's own output in double: a slot sums at most 256 fp32 values, so per sample and
              channel |sum S1 - sum y| <= 2^-16 sum |y| and |sum S2 - sum y^2| <= 2^-16 sum y^2 (256 * 2^-24; derived)
  voxeliser   explicit integer coordinates with multiplicities 1, 2, 3 cycling and one voxel of 70 points: counts exact,
              gather == avg_voxelize_forward bit for bit, split grid == conv3d_presplit(grid), grid within
              4 * cn * 2^-24 * (sum |f| / cn) of the fp64 mean and exactly 0 on empty voxels

Measured on an MI355X (worst over every case of this file; the bound in brackets):
    first convolution, |y - ref| / (conv(|x|, |w|) + |bias|), the same for the dense, compact and list-driven forms (same bits):
        f16x3 2.5e-7 [1.67e-6]   bf16x6 3.4e-7 [9.5e-7]   fp32 (dense, list-driven) 3.4e-7 [9.5e-7]
    second convolution, whole sample, / max |ref| [1e-4], the same for every form:  f16x3 6.1e-7   bf16x6 7.3e-7   fp32 9.8e-7
    second convolution per boundary class 0..26, / max |ref| over the class's own voxels [1e-4], in units of 1e-7:
        f16x3   1.7 3.8 1.8 2.3 3.3 1.9 1.5 2.9 2.0 2.4 3.2 1.7 3.0 6.1 3.9 2.1 2.9 2.0 1.8 2.4 1.6 2.6 3.7 2.6 1.6 2.1 1.4
        bf16x6  1.7 3.0 2.2 2.7 5.0 2.6 1.7 3.3 2.0 2.2 4.5 3.2 4.9 7.3 4.7 2.4 4.7 3.4 1.8 3.0 1.7 3.1 5.3 2.4 2.5 2.8 1.9
        fp32    2.0 3.2 2.9 2.8 5.9 2.8 1.7 3.4 2.2 2.8 6.0 4.1 5.2 9.8 5.5 2.9 5.2 3.5 1.9 3.4 2.0 3.2 7.0 3.1 2.1 2.9 2.0
        (the interior class 13 is the worst; the 8 corner classes 0, 2, 6, 8, 18, 20, 24, 26 stay below 2.9e-7)
    statistics against the own output [2^-16 = 1.53e-5]: sum 1.1e-7 (compact), 7.0e-8 (dense), 4.9e-8 (list-driven); sum of squares
        1.5e-7 (compact), 8.1e-8 (dense), 6.9e-8 (list-driven); compact / list-driven vs dense statistics 8.5e-8 / 6.2e-8 [1e-5]
    voxeliser: 0.23 of its bound
Wall time of the 1964 tests on an MI355X: 6 s (4 s under P2PB_CONV_MATH=bf16x6, where the f16x3 half skips); no test above 0.4 s.
"""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from oracle import occupancy_patterns as op

pytestmark = pytest.mark.gpu

TOL = 1e-4                            # second convolution, of max |ref| (tests/test_fused_gpu.py)
ACC = 2.0 ** -20                      # fp32 accumulation of <= 1728 products, relative to sum |x||w| (tests/test_conv_math_gpu.py)
BOUND_F16 = 3 * 2.0 ** -22 + ACC
BOUND1 = {"f16x3": BOUND_F16, "bf16x6": ACC, "fp32": ACC}  # fp32: exact products, the same accumulation
STAT = 2.0 ** -16                     # 256 values per slot * 2^-24

RAGGED, ALIGNED = (19, 40, 24), (16, 32, 64)  # (C, C1, C2): WM = 2 then WM = 1 / WM = 1 then WM = 2
ODD = (19, 38, 22)  # output channel counts that are no multiple of 4: the scalar stores of both wave layouts (40 and 24 store 16 bytes)


def _order(r):
    """every pattern of r, `full` between `corners` and `single_111`"""
    names = list(op.patterns(r))
    rest = [n for n in names if n not in ("corners", "full", "single_111")]
    return ["corners", "full", "single_111"] + rest


# key -> (r, pattern names = the samples of the batch, (C, C1, C2))
CASES = {}
for _r in (8, 16):
    for _tag, _shape in (("ragged", RAGGED), ("aligned", ALIGNED), ("odd", ODD)):
        CASES[f"r{_r}-{_tag}"] = (_r, _order(_r), _shape)
CASES["r32-ragged"] = (32, ["full", "corners", "wall_w7", "bern0.05"], RAGGED)
CASES["r8-alone-aligned"] = (8, ["full"], ALIGNED)   # B = 1: na == total, ni == 0 and nothing else in the launch
CASES["r16-alone-ragged"] = (16, ["full"], RAGGED)

SPLIT_FORMS = ("compact", "sparse")
PRE_FORMS = ("dense_pre", "compact_pre", "sparse_pre")


def _forms(r, math, with_dense=False, pre=True):
    f = ["dense"] if with_dense else []
    if math != "fp32":
        f.append("compact")
    if r >= 16:
        f.append("sparse")
    if math == "f16x3" and pre:
        f += [p for p in PRE_FORMS if r >= 16 or p != "sparse_pre"]
    return f


def _params(maths=("f16x3", "bf16x6", "fp32"), forms=None):
    out = []
    for key, (r, names, _) in CASES.items():
        for math in maths:
            for form in (forms(r, math) if forms else [None]):
                for b, name in enumerate(names):
                    out.append(pytest.param(key, math, form, b, id="-".join(str(t) for t in (key, math, form, name) if t is not None)))
    return out


def swish(v):
    return v * torch.sigmoid(v)


_HOST, _DEV, _OUT, _WORST = {}, {}, {}, {}


def worst(name, value, bound):
    value = float(value)
    if value >= _WORST.get(name, (-1.0, 0))[0]:
        _WORST[name] = (value, bound)
    return value


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for k in sorted(_WORST):
        print(f"\nMEASURED {k}: {_WORST[k][0]:.3e} [{_WORST[k][1]:.3e}]", end="")
    print()


def host(key):
    """host inputs and fp64 references of one case, built once and never modified"""
    if key not in _HOST:
        r, names, (C, C1, C2) = CASES[key]
        pats = op.patterns(r)
        occ = torch.stack([pats[n] for n in names])
        B = len(names)
        g = torch.Generator().manual_seed(1000 * r + C)
        x = torch.randn(B, r, r, r, C, generator=g) * occ[..., None]
        w1, b1 = torch.randn(C1, C, 3, 3, 3, generator=g) / (27 * C) ** 0.5, torch.randn(C1, generator=g)
        w2, b2 = torch.randn(C2, C1, 3, 3, 3, generator=g) / (27 * C1) ** 0.5, torch.randn(C2, generator=g)
        sc, sh = torch.rand(B, C1, generator=g) + 0.5, torch.randn(B, C1, generator=g)
        cl = lambda t: t.permute(0, 2, 3, 4, 1).contiguous()
        x64 = x.permute(0, 4, 1, 2, 3).double()
        y1 = F.conv3d(x64, w1.double(), b1.double(), padding=1)
        mag1 = F.conv3d(x64.abs(), w1.double().abs(), padding=1) + b1.double().abs()[None, :, None, None, None]
        xin = swish(y1 * sc.double()[:, :, None, None, None] + sh.double()[:, :, None, None, None])
        y2 = F.conv3d(xin, w2.double(), b2.double(), padding=1)
        _HOST[key] = dict(r=r, names=names, B=B, C=C, C1=C1, C2=C2, occ=occ, sets=op.reference_sets(occ), x=x, w1=w1, b1=b1, w2=w2,
                          b2=b2, sc=sc, sh=sh, ref1=cl(y1), mag1=cl(mag1), ref2=cl(y2))
    return _HOST[key]


def _conv_from(w, bias):
    conv = torch.nn.Conv3d(w.shape[1], w.shape[0], 3, padding=1)
    with torch.no_grad():
        conv.weight.copy_(w), conv.bias.copy_(bias)
    return conv.cuda()


def dev(key):
    """device copies, the lists and the far-field constants of one case"""
    if key not in _DEV:
        from p2p_bridge_amd import fused
        h = host(key)
        d = dict(x=h["x"].cuda(), cnt=h["occ"].view(h["B"], -1).int().cuda(), conv1=_conv_from(h["w1"], h["b1"]),
                 conv2=_conv_from(h["w2"], h["b2"]), sc=h["sc"].cuda(), sh=h["sh"].cuda())
        with torch.no_grad():
            d["a"], d["k"] = fused.conv3d_far_field(d["conv1"].bias, d["conv2"], d["sc"], d["sh"], True)
            d["lists"], d["counts"] = fused.active_lists(d["cnt"], h["r"])
            if h["r"] >= 16:
                d["blists"], d["bcounts"] = fused.brick_lists(d["cnt"], h["r"])
        for n in ("ref1", "mag1", "ref2"):
            d[n] = h[n].cuda()
        d["d2"] = h["sets"].d2.cuda()
        d["cls"] = h["sets"].cls.cuda().flatten()
        nb = h["sets"].active.shape[2]
        # voxels of the second convolution's active bricks
        act = h["sets"].active[1].view(h["B"], h["r"] // 4, h["r"] // 8, h["r"] // 8)
        d["act2"] = act.repeat_interleave(4, 1).repeat_interleave(8, 2).repeat_interleave(8, 3).cuda()
        assert nb == (h["r"] // 4) * (h["r"] // 8) ** 2
        _DEV[key] = d
    return _DEV[key]


@contextlib.contextmanager
def arithmetic(math):
    from p2p_bridge_amd import fused
    if math == "f16x3" and not (fused.conv_math() == "f16x3" and fused.lib().p2pb_get_split_terms() == 16):
        pytest.skip("the default arithmetic (f16x3); the suite runs under P2PB_CONV_MATH=" + fused.conv_math())
    with (fused.split_math("bf16x6") if math == "bf16x6" else contextlib.nullcontext()), torch.no_grad():
        yield "fp32" if math == "fp32" else "bf16x6"  # `math=` of the entry points: split kernels (in the arithmetic in force) or fp32


@contextlib.contextmanager
def poisoned_output(c_out, like):
    """the next 5-d torch.empty whose last extent is c_out returns a NaN-filled tensor: what the kernel leaves unwritten stays NaN"""
    poison = torch.full_like(like, float("nan"))
    real_empty = torch.empty
    shape_of = lambda a: tuple(a[0]) if len(a) == 1 and isinstance(a[0], (tuple, list)) else a
    torch.empty = lambda *a, **kw: poison if (len(shape_of(a)) == 5 and shape_of(a)[-1] == c_out) else real_empty(*a, **kw)
    try:
        yield poison
    finally:
        torch.empty = real_empty


def outputs(key, math):
    """form -> (y1, st1, y2, st2) of the two convolutions, each form on its own first output; "<form>/part" -> (y2, st2) of the
    listed_only / active_only launch on a NaN-prefilled output. Computed once per (case, arithmetic)."""
    if (key, math) in _OUT:
        return _OUT[(key, math)]
    from p2p_bridge_amd import fused
    h, d = host(key), dev(key)
    r, C2 = h["r"], h["C2"]
    x, conv1, conv2, sc, sh, a, k = d["x"], d["conv1"], d["conv2"], d["sc"], d["sh"], d["a"], d["k"]
    o = {}
    with arithmetic(math) as m:
        cl = dict(channels_last=True)
        y1, s1 = fused.conv3d_k3(x, conv1, compact=True, math=m, **cl)
        y2, s2 = fused.conv3d_k3(y1, conv2, sc, sh, swish=True, compact=True, math=m, in_sub=a, out_class=k, **cl)
        o["dense"] = (y1, s1, y2, s2)
        if math != "fp32":
            L, N = d["lists"], d["counts"]
            c1, t1 = fused.conv3d_k3_compact(x, conv1, L, N, 0)
            c2, t2 = fused.conv3d_k3_compact(c1, conv2, L, N, 1, sc, sh, True, in_sub=a, out_class=k)
            o["compact"] = (c1, t1, c2, t2)
            with poisoned_output(C2, c2) as p:
                got = fused.conv3d_k3_compact(c1, conv2, L, N, 1, sc, sh, True, in_sub=a, out_class=k, listed_only=True)
            assert got[0].data_ptr() == p.data_ptr()
            o["compact/part"] = got
        if r >= 16:
            L, N = d["blists"], d["bcounts"]
            b1, t1 = fused.conv3d_k3_sparse(x, conv1, L, N, 0, math=m, **cl)
            b2, t2 = fused.conv3d_k3_sparse(b1, conv2, L, N, 1, sc, sh, True, in_sub=a, out_class=k, math=m, **cl)
            o["sparse"] = (b1, t1, b2, t2)
            with poisoned_output(C2, b2) as p:
                got = fused.conv3d_k3_sparse(b1, conv2, L, N, 1, sc, sh, True, in_sub=a, out_class=k, math=m, active_only=True, **cl)
            assert got[0].data_ptr() == p.data_ptr()
            o["sparse/part"] = got
        if math == "f16x3":
            xs = fused.conv3d_presplit(x)
            p1, t1 = fused.conv3d_k3(xs, conv1, compact=True, pre=True, **cl)
            p2, t2 = fused.conv3d_k3(fused.conv3d_presplit(p1, sc, sh, True, a), conv2, out_class=k, compact=True, pre=True, **cl)
            o["dense_pre"] = (p1, t1, p2, t2)
            L, N = d["lists"], d["counts"]
            p1, t1 = fused.conv3d_k3_compact(xs, conv1, L, N, 0, pre=True)
            operand = fused.conv3d_presplit(p1, sc, sh, True, a)
            p2, t2 = fused.conv3d_k3_compact(operand, conv2, L, N, 1, out_class=k, pre=True)
            o["compact_pre"] = (p1, t1, p2, t2)
            with poisoned_output(C2, p2) as p:
                got = fused.conv3d_k3_compact(operand, conv2, L, N, 1, out_class=k, pre=True, listed_only=True)
            assert got[0].data_ptr() == p.data_ptr()
            o["compact_pre/part"] = got
            if r >= 16:
                L, N = d["blists"], d["bcounts"]
                p1, t1 = fused.conv3d_k3_sparse(xs, conv1, L, N, 0, pre=True, **cl)
                operand = fused.conv3d_presplit(p1, sc, sh, True, a)
                p2, t2 = fused.conv3d_k3_sparse(operand, conv2, L, N, 1, out_class=k, pre=True, **cl)
                o["sparse_pre"] = (p1, t1, p2, t2)
                with poisoned_output(C2, p2) as p:
                    got = fused.conv3d_k3_sparse(operand, conv2, L, N, 1, out_class=k, pre=True, active_only=True, **cl)
                assert got[0].data_ptr() == p.data_ptr()
                o["sparse_pre/part"] = got
    _OUT[(key, math)] = o
    return o


# ---------------------------------------------------------------------------------------------------------- 1. list builders

@pytest.mark.parametrize("key,math,form,b", _params(maths=(None,)))
def test_active_lists(key, math, form, b):
    """every list is a permutation of 0..255 whose first `count` entries are exactly D1 / D2; the counts themselves"""
    h, d = host(key), dev(key)
    lists, counts = d["lists"][:, b].cpu().long(), d["counts"][:, b].cpu().long()
    assert torch.equal(counts, h["sets"].counts[:, b]), (counts.tolist(), h["sets"].counts[:, b].tolist())
    assert torch.equal(lists.sort(dim=-1).values, torch.arange(256).expand_as(lists))
    for which, dset in enumerate((h["sets"].d1, h["sets"].d2)):
        want = op.to_bricks(dset[b : b + 1])[0]
        first = torch.arange(256).expand_as(lists[which]) < counts[which][:, None]
        listed = torch.zeros_like(want).scatter_(1, lists[which], first)
        bad = (listed != want).any(1).nonzero().flatten().tolist()
        assert not bad, f"D{which + 1}: bricks {bad} list other voxels than the reference set"


@pytest.mark.parametrize("key,math,form,b", [p for p in _params(maths=(None,)) if CASES[p.values[0]][0] >= 16])
def test_brick_lists(key, math, form, b):
    """active and inactive lists partition the (sample, brick) pairs, the active ones are the reference's (occupancy within
    brick +- 1 / +- 2); a full grid has na == total and ni == 0"""
    h, d = host(key), dev(key)
    lists, counts = d["blists"].cpu().long(), d["bcounts"].cpu().tolist()
    total = lists.shape[1]
    nb = total // h["B"]
    for which in (0, 1):
        na, ni = counts[2 * which], counts[2 * which + 1]
        assert na + ni == total and na == int(h["sets"].active[which].sum()), (which, na, ni)
        act, ina = lists[2 * which, :na], lists[2 * which + 1, :ni]
        mine_a, mine_i = act[act // nb == b] % nb, ina[ina // nb == b] % nb
        assert torch.equal(mine_a.sort().values, h["sets"].active[which, b].nonzero().flatten()), which
        assert torch.equal(torch.cat([mine_a, mine_i]).sort().values, torch.arange(nb)), which
        if h["names"][b] == "full":
            assert len(mine_i) == 0 and len(mine_a) == nb
        if h["names"] == ["full"]:
            assert na == total and ni == 0


# ---------------------------------------------------------------------------------------------------------- 2. same bits

def stats_of(st):
    s = st.double().sum(0)  # one sample: [slots, C, 2] -> [C, 2]
    return s[..., 0], s[..., 1]


def rel(a, ref):
    return ((a - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


@pytest.mark.parametrize("key,math,form,b", _params(forms=_forms))
def test_same_bits_as_the_dense_form(key, math, form, b):
    o = outputs(key, math)
    y1, s1, y2, s2 = (t[b] for t in o["dense"])
    f1, t1, f2, t2 = (t[b] for t in o[form])
    for conv, (y, f) in enumerate(((y1, f1), (y2, f2)), 1):
        ne = (y != f).any(-1)
        assert not ne.any(), f"convolution {conv}: {int(ne.sum())} voxels differ, first at flat index {int(ne.flatten().nonzero()[0])}"
    if form in PRE_FORMS:  # the same kernel form on the fp32 operand: outputs AND statistics, bit for bit
        q1, u1, q2, u2 = (t[b] for t in o[form[:-4]])
        assert torch.equal(f1, q1) and torch.equal(f2, q2)
        assert torch.equal(t1, u1) and torch.equal(t2, u2)
    for conv, (s, t) in enumerate(((s1, t1), (s2, t2)), 1):  # other slots, same sums
        for i, what in enumerate(("sum", "sum of squares")):
            e = worst(f"statistics, {form} vs dense, {math}", rel(stats_of(t)[i], stats_of(s)[i]), 1e-5)
            assert e < 1e-5, f"convolution {conv}, {what}: {e:.3e}"


# ---------------------------------------------------------------------------------------------------------- 3. partial writes

@pytest.mark.parametrize("key,math,form,b", _params(forms=lambda r, math: [f for f in _forms(r, math) if f != "dense_pre"]))
def test_listed_only_and_active_only(key, math, form, b):
    """second convolution: same bits inside the set (D2, compact / the active bricks, list-driven), the same statistics, nothing
    written anywhere else; the full grid comes back without a NaN"""
    h, d, o = host(key), dev(key), outputs(key, math)
    inside = (d["d2"] if form.startswith("compact") else d["act2"])[b]
    y2, st2 = o[form][2][b], o[form][3][b]
    p2, pst2 = (t[b] for t in o[form + "/part"])
    assert torch.equal(pst2, st2), "statistics differ from the full form's"
    assert torch.equal(p2[inside], y2[inside]), "outputs inside the set differ from the full form's"
    assert torch.isnan(p2[~inside]).all(), f"{int((~torch.isnan(p2[~inside])).sum())} values written outside the set"
    if h["names"][b] == "full":
        assert inside.all() and not torch.isnan(p2).any()


# ---------------------------------------------------------------------------------------------------------- 4. against fp64

@pytest.mark.parametrize("key,math,form,b", _params(forms=lambda r, math: _forms(r, math, with_dense=True, pre=False)))
def test_against_fp64(key, math, form, b):
    h, d, o = host(key), dev(key), outputs(key, math)
    y1, _, y2, _ = (t[b] for t in o[form])
    e1 = worst(f"first convolution, {form}, {math}", ((y1.double() - d["ref1"][b]).abs() / d["mag1"][b]).max(), BOUND1[math])
    ref2 = d["ref2"][b]
    err = (y2.double() - ref2).abs().flatten(0, 2).amax(1)  # per voxel
    top = ref2.abs().flatten(0, 2).amax(1)
    e2 = worst(f"second convolution, {form}, {math}, whole sample", err.max() / top.max(), TOL)
    cls = d["cls"]
    cerr = torch.zeros(27, dtype=torch.float64, device="cuda").scatter_reduce_(0, cls, err, "amax")
    ctop = torch.zeros(27, dtype=torch.float64, device="cuda").scatter_reduce_(0, cls, top, "amax")
    ec = (cerr / ctop).cpu()
    for c in range(27):
        worst(f"second convolution, {math}, class {c:2d}", ec[c], TOL)
    print(f"{key} {math} {form} {h['names'][b]}: conv1 {e1:.3e}, conv2 {e2:.3e}, worst class {int(ec.argmax())} {ec.max().item():.3e}")
    assert e1 < BOUND1[math], f"first convolution: {e1:.3e} of conv(|x|, |w|) + |bias|"
    assert e2 < TOL, f"second convolution: {e2:.3e} of max |ref|"
    bad = {c: f"{ec[c].item():.3e}" for c in range(27) if not ec[c] < TOL}
    assert not bad, f"second convolution, boundary classes over {TOL} of their own max |ref|: {bad}"


# ---------------------------------------------------------------------------------------------------------- 5. statistics

@pytest.mark.parametrize("key,math,form,b", _params(forms=lambda r, math: _forms(r, math, with_dense=True, pre=False)))
def test_statistics_against_own_output(key, math, form, b):
    o = outputs(key, math)
    for conv in (1, 2):
        y = o["dense"][2 * conv - 2][b].double().flatten(0, 2)  # [r^3, C]
        s1, s2 = stats_of(o[form][2 * conv - 1][b])
        e1 = worst(f"statistics sum, {form}, {math}", ((s1 - y.sum(0)).abs() / y.abs().sum(0)).max(), STAT)
        e2 = worst(f"statistics sum of squares, {form}, {math}", ((s2 - (y * y).sum(0)).abs() / (y * y).sum(0)).max(), STAT)
        assert e1 <= STAT, f"convolution {conv}: |sum S1 - sum y| = {e1:.3e} sum |y|"
        assert e2 <= STAT, f"convolution {conv}: |sum S2 - sum y^2| = {e2:.3e} sum y^2"


# ---------------------------------------------------------------------------------------------------------- voxeliser

def _points(occ_b, gen):
    """bool[B, r, r, r] -> (vox i32[B, 3, N], multiplicity i32[B, r^3]): every occupied voxel 1, 2, 3, 1, ... times in id order, the
    middle one 70 times; padded to one N with further points of the sample's own occupied voxels, round-robin; shuffled"""
    B, r = occ_b.shape[0], occ_b.shape[1]
    ids, n = [], 0
    for b in range(B):
        v = occ_b[b].flatten().nonzero().flatten()
        mult = torch.arange(len(v)) % 3 + 1
        mult[len(v) // 2] = 70
        ids.append(v.repeat_interleave(mult))
        n = max(n, len(ids[-1]))
    vox = torch.empty(B, 3, n, dtype=torch.int32)
    cnt = torch.zeros(B, r ** 3, dtype=torch.int32)
    for b in range(B):
        v = occ_b[b].flatten().nonzero().flatten()
        pad = v[torch.arange(n - len(ids[b])) % len(v)]
        p = torch.cat([ids[b], pad])
        p = p[torch.randperm(n, generator=gen)]
        vox[b, 0], vox[b, 1], vox[b, 2] = p // (r * r), (p // r) % r, p % r
        cnt[b] = torch.bincount(p, minlength=r ** 3).int()
    return vox, cnt


def _vox_cases():
    out = []
    for r in (8, 16):
        for C in (19, 16):
            out.append(pytest.param(r, C, [n for n in _order(r) if n != "full"], id=f"r{r}-C{C}-patterns"))
            out.append(pytest.param(r, C, ["full"], id=f"r{r}-C{C}-full"))
    return out


@pytest.mark.parametrize("r,C,names", _vox_cases())
def test_voxeliser_on_the_patterns(r, C, names):
    from p2p_bridge_amd import fused
    from p2p_bridge_amd import pointnet2_batch_cuda as ext
    pats = op.patterns(r)
    occ = torch.stack([pats[n] for n in names])
    g = torch.Generator().manual_seed(r + C)
    vox, mult = _points(occ, g)
    B, N = vox.shape[0], vox.shape[2]
    assert mult.max() >= 70 and torch.equal(mult > 0, occ.view(B, -1))
    f = torch.randn(B, C, N, generator=g)
    ind = (vox[:, 0].long() * r + vox[:, 1]) * r + vox[:, 2]
    s = torch.zeros(B, C, r ** 3, dtype=torch.float64).scatter_add_(2, ind[:, None].expand(B, C, N), f.double())
    sabs = torch.zeros(B, C, r ** 3, dtype=torch.float64).scatter_add_(2, ind[:, None].expand(B, C, N), f.double().abs())
    cn = mult.double()[:, None].clamp_min(1)
    mean = (s / cn).permute(0, 2, 1).reshape(B, r, r, r, C)
    bound = (4 * cn * 2.0 ** -24 * (sabs / cn)).permute(0, 2, 1).reshape(B, r, r, r, C)
    dvox, df = vox.cuda(), f.cuda()
    cnt, ws = fused.voxel_sort(dvox, r)
    assert torch.equal(cnt.cpu(), mult)
    grid = fused.voxelize_cl_gather(df, cnt, ws, r)
    want, _, cnt2 = ext.avg_voxelize_forward(df, dvox, r)
    assert torch.equal(cnt2.view(B, -1).cpu(), mult)
    assert torch.equal(grid, want.view(B, C, r, r, r).permute(0, 2, 3, 4, 1))
    if fused.conv_math() == "f16x3" and fused.lib().p2pb_get_split_terms() == 16:  # the S format is the f16x3 arithmetic's
        gs = fused.voxelize_cl_gather(df, cnt, ws, r, split=True)
        assert torch.equal(gs.view(torch.int32), fused.conv3d_presplit(grid).view(torch.int32))
    err = (grid.cpu().double() - mean).abs()
    e = worst("voxeliser, error / bound", (err / bound.clamp_min(1e-300))[occ].max(), 1.0)
    for b, name in enumerate(names):
        assert (err[b] <= bound[b]).all(), f"{name}: {(err[b] / bound[b].clamp_min(1e-300))[occ[b]].max().item():.3f} of the bound"
        assert (grid[b].cpu()[~occ[b]] == 0).all(), f"{name}: an empty voxel is not 0"
    assert e <= 1.0
