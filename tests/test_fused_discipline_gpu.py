"""The fused launches of the sampler that tests/test_memory_discipline_gpu.py did not call, inside the same poisoned arena
(oracle/poison_arena.py) and under the same four checks -- guards intact, results free of NaN, allocation through the arena,
parity --: interp_add, pw_conv_pool_gather, voxel_sort / voxelize_cl_gather, conv3d_presplit and the `pre=True` convolutions,
conv3d_far_field(_gn), pvconv_tail, minmax_act_pool_gn, minmax_act, affine_act, affine_act_max and the pw_conv arms
(point_major, ci_lo / ci_hi, fin=, the wide-layer pre-pass).

Every input is built on the host and `put` into the arena, modules go through `put_module`, and parity is ALWAYS against a
host reference that runs no HIP: fp64 torch on the CPU, or oracle/cpu_ops.py where the contract is bit-exactness (a launch
whose input is another launch's output -- partials, {min, max}, a first convolution's grid -- is held to the host reference of
ITS operation on the downloaded input, and the chain as a whole to fp64 of the host inputs where a tolerance exists). Where the
suite already holds two wrappers to each other's bits (test_gn_merged_gpu.py, test_conv_presplit_gpu.py,
test_fused_gpu.py) that equality is asserted as well, inside the arena. Tolerances are those of the file named next to each
family; the two that existed nowhere (FF_TOL, GN_TOL below) are four times the error of the same chain in fp32 on the host.

Cases that cannot reach the arm the shape was chosen for say so next to them: (2, 64, 130, 8) of the voxeliser (r^3 < 4 N: the
one-pass split kernel; (2, 64, 128, 8) beside it takes the occupied one) and (M, U) = (7, 8) of affine_act_max (refused by the
launcher, held as a refusal). None skips on the default build (f16x3); under P2PB_CONV_MATH=bf16x6 / fp32 the gathered GEMM and
the pre-split convolutions skip, as their own files do.

Run time on an MI355X: 145 cases in 3.9 s on their own; the whole `-m gpu` suite took 311.2 s with this file in it (3380 tests),
so about 307 s without it (the parent commit's 3235 tests, same box, same run).
"""
import pytest
import torch

from oracle import cpu_ops
from oracle.poison_arena import PoisonArena
from test_gn_merged_gpu import _norm, _partials
from test_memory_discipline_gpu import ARENA_BYTES, TOL, cloud, eq, put_module, rel_err, run, stats_of, swish

pytestmark = pytest.mark.gpu

F64 = torch.float64

# conv3d_far_field's a / K against the fp64 constant-grid convolution. The same chain in fp32 on the host (act(prev_bias * scale
# + shift), torch conv3d of the 3 x 3 x 3 constant grid) is FF_HOST_FP32 off fp64 at worst over the cases of
# test_conv3d_far_field; the HIP result is allowed four times that. Measured on an MI355X: 2.76e-7 (K), 1.05e-7 (a), both
# below the host's own fp32 figure.
FF_HOST_FP32 = 8.67e-7
FF_TOL = 4 * FF_HOST_FP32
# pvconv_tail / minmax_act_pool_gn outputs (and every folded GroupNorm's scale / shift / channel mean) against the fp64
# restatement from the partials: the same formulas in fp32 on the host are GN_HOST_FP32 off at worst over the cases of
# test_pvconv_tail and test_minmax_act_pool_gn (3.99e-7 over the first, 1.68e-6 over the second: var = E[x^2] - mean^2 cancels
# in fp32). Measured on an MI355X: 1.37e-7 (pvconv_tail aff_a), 1.03e-7 (minmax_act_pool_gn y), under 5e-8 for every scale / shift
# -- the kernels combine the partials in double, what is left is the rounding of the fp32 results and the fast exp / reciprocal.
GN_HOST_FP32 = 1.68e-6
GN_TOL = 4 * GN_HOST_FP32

_WORST = {}  # measured worst errors per family, printed by every case (run with -s to read them)


def note(family, kind, value):
    key = (family, kind)
    _WORST[key] = max(_WORST.get(key, 0.0), value)
    print(f"[{family}] {kind} = {value:.3e} (worst so far {_WORST[key]:.3e})")
    return value


@pytest.fixture
def arena():
    with PoisonArena("cuda", ARENA_BYTES) as a:
        yield a


@pytest.fixture(scope="module")
def fused():
    from p2p_bridge_amd import fused as f

    return f


def act(x, on):
    return swish(x) if on else x


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- host references shared by the families below ---------------------------------------------------------------------

def gn_ref(part, count, groups, gamma, beta, style, eps, dt=F64):
    """GroupNorm(+AdaGN) folded to a per-(sample, channel) affine, from the {sum, sum of squares} partials [B, nslots, C, 2] on the
    host (the formulas test_fused_gpu.py::test_gn_affine_params checks): group mean and biased variance from the sums over
    slots and the group's channels, scale = gamma * rstd (* factor), shift = (beta - mean * rstd * gamma) (* factor + bias),
    and the per-channel mean of the normalised tensor from the channel's own sum -> (scale, shift, chmean) [B, C] in `dt`"""
    p = part.to(dt)
    s, q = p[..., 0].sum(1), p[..., 1].sum(1)
    b, c = s.shape
    cg = c // groups
    n = count * cg
    mean = s.view(b, groups, cg).sum(2) / n
    var = (q.view(b, groups, cg).sum(2) / n - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    mean, rstd = mean.repeat_interleave(cg, 1), rstd.repeat_interleave(cg, 1)
    scale = rstd * gamma.to(dt)
    shift = beta.to(dt) - mean * scale
    if style is not None:
        scale, shift = scale * style[:, :c].to(dt), shift * style[:, :c].to(dt) + style[:, c:].to(dt)
    return scale, shift, scale * (s / count) + shift


def norm_pair(arena, c, groups, b, styled, seed):
    """the norm parameters `_norm` of test_gn_merged_gpu.py builds, as host tensors and as their copies in the arena; the style
    rows are a column slice of the wider matrix in both"""
    gamma, beta, style = _norm(c, groups, b, styled, seed)
    hg, hb, hs, ds = gamma.cpu(), beta.cpu(), None, None
    if styled:
        wide, off = style._base.cpu(), style.storage_offset()
        hs, ds = wide[:, off:off + 2 * c], arena.put(wide)[:, off:off + 2 * c]
    return (hg, hb, hs), (arena.put(hg), arena.put(hb), ds)


def check_gn(what, got, part, count, groups, host_norm, eps, want_mean=False):
    """(scale, shift, chmean | None) of a folded norm against gn_ref of the downloaded partials, at GN_TOL"""
    ref = gn_ref(part.cpu(), count, groups, *host_norm, eps)
    r32 = gn_ref(part.cpu(), count, groups, *host_norm, eps, dt=torch.float32)
    errs = []
    for name, g, r, r_ in zip(("scale", "shift", "chmean"), got, ref, r32):
        if g is None:
            assert name == "chmean" and not want_mean
            continue
        note("gn", f"host fp32 {what}", rel_err(r_, r))
        errs.append((name, note("gn", f"hip {what} {name}", rel_err(g, r))))
    assert all(e < GN_TOL for _, e in errs), errs


# ---- 1. interp_add (csrc/neighbors.hip three_interp_add_kernel; tolerance: test_fused_gpu.py::test_first_layer_before_interpolation)

# n: one 64-point tile holding one point, a tile short by one, a tile over by one, two tiles and a ragged third; c: less than one
# 64-channel chunk, exactly one, one and a ragged second
@pytest.mark.parametrize("with_add,with_bias", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("c", [3, 64, 72])
@pytest.mark.parametrize("n", [1, 63, 65, 130])
def test_interp_add(arena, fused, n, c, with_add, with_bias):
    B, m = 2, 5
    g = torch.Generator().manual_seed(n * 100 + c)
    cz = torch.randn(B, c, m, generator=g)
    idx = torch.randint(0, m, (B, 3, n), generator=g, dtype=torch.int32)
    idx[:, :, 0] = torch.tensor([0, m - 1, m - 1], dtype=torch.int32)  # rows 0 and m - 1, one index twice in a point's three
    assert idx.min() == 0 and idx.max() == m - 1
    w = torch.rand(B, 3, n, generator=g)
    w = w / w.sum(1, keepdim=True)
    add = torch.randn(B, c, n, generator=g) if with_add else None
    bias = torch.randn(c, generator=g) if with_bias else None
    ref = sum(w[:, k, None, :].double() * cz.double().gather(2, idx[:, k, None, :].long().expand(-1, c, -1)) for k in range(3))
    if with_add:
        ref = ref + add.double()
    if with_bias:
        ref = ref + bias.double()[None, :, None]
    didx, dw = arena.put(idx), arena.put(w)
    dadd = arena.put(add) if with_add else None
    dbias = arena.put(bias) if with_bias else None
    # channel-major cz: the wrapper carves the point-major copy as a workspace. m = 5 is no multiple of 4, so pw_conv could not
    # have produced the point-major layout itself; interp_add takes it at any m, and the host transposes it here
    y, st = run(arena, fused.interp_add, arena.put(cz), didx, dw, add=dadd, bias=dbias)
    y_pm, st_pm = run(arena, fused.interp_add, arena.put(cz.transpose(1, 2)), didx, dw, add=dadd, bias=dbias, point_major=True)
    assert y.shape == (B, c, n) and st.shape == (B, (n + 63) // 64 * 2, c, 2)
    assert rel_err(y, ref) < 1e-5
    assert rel_err(stats_of(st)[1], (ref * ref).sum(2)) < 1e-5
    eq(y_pm, y, "point-major y"), eq(st_pm, st, "point-major statistics")


# ---- 2. pw_conv_pool_gather (csrc/pointwise.hip, pw_wide_kernel<GATHER>; tolerances:
# test_fused_gpu.py::test_set_abstraction_last_layer_on_the_gathered_operand, minmax_act: test_pw_conv_neighbour_pool) -----

@pytest.mark.parametrize("with_fin", [False, True])
@pytest.mark.parametrize("B,N,M,U,Ci,Co", [(1, 300, 37, 8, 40, 24), (2, 130, 12, 16, 64, 128)])
def test_pw_conv_pool_gather(arena, fused, B, N, M, U, Ci, Co, with_fin):
    if not fused.gather_pool_supported(Ci, Co, M, U):
        pytest.skip(f"gather_pool_supported({Ci}, {Co}, {M}, {U}) is False (conv math {fused.conv_math()}: the f16x3 form only)")
    torch.manual_seed(B * 7 + U)
    z, cx = torch.randn(B, N, Ci), torch.randn(B, M, Ci)
    idx = torch.randint(0, N, (B, M, U), dtype=torch.int32)
    idx[:, 0, 0], idx[:, -1, -1] = 0, N - 1
    conv = torch.nn.Conv2d(Ci, Co, 1)
    sc, sh = torch.rand(B, Ci) + 0.5, torch.randn(B, Ci)
    sc2, sh2 = torch.randn(B, Co), torch.randn(B, Co)
    with torch.no_grad():
        grouped = (z.double()[torch.arange(B)[:, None, None], idx.long()] - cx.double()[:, :, None, :]).permute(0, 3, 1, 2)
        h = swish(grouped * sc[:, :, None, None].double() + sh[:, :, None, None].double())
        out = torch.einsum("oc,bcmu->bomu", conv.weight.view(Co, Ci).double(), h) + conv.bias.double()[None, :, None, None]
        put_module(arena, conv)
        dz, dcx, didx, dsc, dsh = arena.put(z), arena.put(cx), arena.put(idx), arena.put(sc), arena.put(sh)
        st, mm = run(arena, fused.pw_conv_pool_gather, dz, dcx, didx, conv, dsc, dsh, True)
        if with_fin:
            host_norm, dev_norm = norm_pair(arena, Co, 8, B, B == 2, seed=Co)
            st_f, mm_f, aff = run(arena, fused.pw_conv_pool_gather, dz, dcx, didx, conv, dsc, dsh, True,
                                  fin=(float(M * U), 8, *dev_norm, 1e-5, False))
            eq(st_f, st, "statistics with fin"), eq(mm_f, mm, "minmax with fin")
            check_gn("gather fin", aff, st_f, float(M * U), 8, host_norm, 1e-5)
        assert st.shape[0] == B and st.shape[2:] == (Co, 2) and mm.shape == (B, Co, M, 2)
        assert rel_err(mm[..., 1], out.amax(-1)) < TOL and rel_err(mm[..., 0], out.amin(-1)) < TOL
        s1, s2 = stats_of(st)
        assert rel_err(s1, out.sum((2, 3))) < TOL * 10 or (s1 - out.sum((2, 3))).abs().max() < 1e-3
        assert rel_err(s2, (out * out).sum((2, 3))) < TOL
        # the per-neighbourhood max through minmax_act: against its own inputs in fp64 (1e-5), and end to end (swish falls, then
        # rises: its maximum over a neighbourhood is at the smallest or the largest raw value)
        got = run(arena, fused.minmax_act, mm, arena.put(sc2), arena.put(sh2))
        aff2 = lambda t: swish(t.double().cpu() * sc2[:, :, None].double() + sh2[:, :, None].double())
        assert rel_err(got, torch.maximum(aff2(mm[..., 0]), aff2(mm[..., 1]))) < 1e-5
        assert rel_err(got, swish(out * sc2[:, :, None, None].double() + sh2[:, :, None, None].double()).amax(-1)) < TOL


# ---- 3. voxel_sort / voxelize_cl_gather (csrc/voxel_coords.hip, voxel_gather.hip; bit-exact against the oracle) --------------------------------

# (B, C, N, r, seed of the cloud). Arms of p2pb_avg_voxelize_cl_gather (fp32 grid) | p2pb_avg_voxelize_cl_gather_split:
#   (2, 35, 301, 4)  : C % 4 != 0: zero-fill + vox_gather_cl_occ_kernel | zero-fill + vox_gather_cl_occ_split_kernel<false>; the
#                      planted voxel holds more than 64 points: the loop arm of vox_sort_kernel
#   (1, 16, 64, 4)   : C % 4 == 0, r^3 = 64 < 4 N: vox_gather_cl_all_kernel<true> | vox_gather_cl_split_kernel<true>. N = 64 cannot
#                      hold a voxel of more than 64 points
#   (2, 12, 257, 4)  : the same one-pass kernels; C = 12 is ragged against the split kernel's 8-channel thread and 16-channel
#                      chunk (its second thread loads one quad, its chunk is padded by four channels); one more point than a
#                      256-thread block of the count / fill kernels; the planted voxel holds 65 points or more
#   (2, 64, 130, 8)  : C % 4 == 0 and r^3 = 512 < 4 N = 520: this shape CANNOT reach the occupied split kernel (the launcher wants
#                      r^3 >= 4 N, that is N <= 128 at r = 8); it takes the one-pass kernels at four whole chunks per voxel and one
#                      ragged 32-point tile of the transpose. The next shape reaches that arm
#   (2, 64, 128, 8)  : r^3 = 512 >= 4 N: vox_gather_cl_all_kernel<true> | zero-fill + vox_gather_cl_occ_split_kernel<true>
#   (1, 36, 1000, 16): r^3 = 4096 >= 4 N, C = 36 (three chunks, the last one padded by twelve channels, its second thread
#                      without channels): vox_gather_cl_all_kernel<true> | vox_gather_cl_occ_split_kernel<true>
# The arms only an A/B switch reaches (vox_gather_cl_all_kernel<false>, vox_gather_cl_split_kernel<false>, the occupied forms on
# 16-byte rows at r^3 < 4 N): tests/test_voxel_switch_arms_gpu.py runs this file's test on the first five shapes with the switch set.
VOX_SHAPES = [(2, 35, 301, 4, 0), (1, 16, 64, 4, 2), (2, 12, 257, 4, 0), (2, 64, 130, 8, 0), (2, 64, 128, 8, 0), (1, 36, 1000, 16, 0)]


def vox_case(B, C, N, r, seed):
    """voxel coordinates of the existing file's `cloud`, the first quarter of the last sample's points moved into ONE voxel (that
    of the first point behind the quarter), and features"""
    _, vox = cpu_ops.voxel_coords(cloud(B, N, seed=seed), r)
    q = N // 4
    vox[B - 1, :, :q] = vox[B - 1, :, q:q + 1]
    f = torch.randn(B, C, N, generator=torch.Generator().manual_seed(N + C))
    return vox, f


@pytest.mark.parametrize("B,C,N,r,seed", VOX_SHAPES)
def test_voxel_sort_and_gather(arena, fused, B, C, N, r, seed):
    vox, f = vox_case(B, C, N, r, seed)
    grid0, _, cnt0 = cpu_ops.avg_voxelize_forward(f, vox, r)
    have = set(cnt0.unique().tolist())
    assert {1, 2, 3, 4, 5} <= have, sorted(have)
    if N // 4 >= 64:  # (N = 64, 128 and 130 cannot: a quarter of their points is 16 or 32)
        assert cnt0.max().item() > 64
    cnt, ws = run(arena, fused.voxel_sort, arena.put(vox), r)  # ws: a workspace, guards only
    eq(cnt, cnt0, "cnt")
    df = arena.put(f)
    g = run(arena, fused.voxelize_cl_gather, df, cnt, ws, r)
    assert g.shape == (B, r, r, r, C)
    eq(bits(g), bits(grid0.view(B, C, r, r, r).permute(0, 2, 3, 4, 1)), "fp32 grid")
    gs = run(arena, fused.voxelize_cl_gather, df, cnt, ws, r, split=True)
    cpad = (C + 15) // 16 * 16
    assert gs.shape == (B, r, r, r, cpad)
    eq(bits(gs), bits(run(arena, fused.conv3d_presplit, g)), "split grid == presplit(fp32 grid)")
    # S format (include/p2pb_hip.h): per voxel [chunk][plane][khalf][8 halves], channel = chunk * 16 + khalf * 8 + i
    halves = gs.view(torch.int16).view(B, r ** 3, cpad // 16, 2, 2, 8).permute(0, 1, 3, 2, 4, 5).reshape(B, r ** 3, 2, cpad)
    assert not halves[..., C:].any(), "padded channels of the split grid"
    assert halves[..., :C].any()


@pytest.mark.parametrize("B,C,N,r", [(2, 19, 301, 8), (1, 64, 130, 4)])
def test_devoxelize_affine_add(arena, fused, B, C, N, r):
    """devoxelize_affine(channels_last=True, add=(h, scale, shift)): trilinear(grid * a + b) + swish(h * scale + shift), the join
    behind a PVConv. The interpolation is the oracle's (its weights sum to one, so the affine commutes with it); 1e-5 as
    test_voxelize_cl_devoxelize_cl"""
    g = torch.Generator().manual_seed(N + C)
    norm, _ = cpu_ops.voxel_coords(cloud(B, N, seed=3), r)
    dense = torch.randn(B, C, r, r, r, generator=g)
    a, b_, hs, hb = (torch.randn(B, C, generator=g) for _ in range(4))
    h = torch.randn(B, C, N, generator=g)
    plain = cpu_ops.trilinear_devoxelize_forward(r, False, norm, dense.view(B, C, -1).contiguous())[0].double()
    ref = plain * a[:, :, None].double() + b_[:, :, None].double() + swish(h.double() * hs[:, :, None].double() + hb[:, :, None].double())
    got = run(arena, fused.devoxelize_affine, arena.put(dense.permute(0, 2, 3, 4, 1)), arena.put(norm), r, arena.put(a), arena.put(b_),
              channels_last=True, add=(arena.put(h), arena.put(hs), arena.put(hb)))
    assert got.shape == (B, C, N) and rel_err(got, ref) < 1e-5


# ---- 4. conv3d_presplit and the pre=True convolutions (csrc/conv3d.hip PreStage; bits: test_conv_presplit_gpu.py, fp64:
# the 1e-5 of test_fused_gpu.py::test_conv3d_split_is_fp32_faithful) -------------------------------------------------------

def _dilate(m):
    return torch.nn.functional.max_pool3d(m, 3, 1, 1)


@pytest.mark.parametrize("C,r", [(16, 8), (19, 8), (64, 8), (19, 16)])
def test_presplit_convolutions(arena, fused, C, r):
    """C = 16: one whole chunk; 19: a ragged second chunk, scalar loads (C % 4 != 0); 64: four chunks. A PVConv's pair: conv1 on the
    plain pre-split grid, conv2 on presplit(y1, scale, shift, swish, in_sub)"""
    if fused.conv_math() != "f16x3":
        pytest.skip("the pre-split format is the f16x3 arithmetic's")
    B, C2 = 2, 24
    g = torch.Generator().manual_seed(r + C)
    occ = torch.zeros(B, r, r, r)
    for b in range(B):  # a sparse slab of another depth per sample, and one voxel in the far corner
        k = r // 4 + 1 + b
        occ[b, :k, : r // 2 + 1, : r // 2 - 1] = (torch.rand(k, r // 2 + 1, r // 2 - 1, generator=g) < 0.15).float()
    occ[-1, -1, -1, -1] = 1.0
    x = torch.randn(B, r, r, r, C, generator=g) * occ[..., None]
    conv1, conv2 = torch.nn.Conv3d(C, C, 3, padding=1), torch.nn.Conv3d(C, C2, 3, padding=1)
    sc, sh = torch.rand(B, C, generator=g) + 0.5, torch.randn(B, C, generator=g)
    cl = lambda t: t.permute(0, 4, 1, 2, 3)
    with torch.no_grad():
        w1, b1, w2, b2 = conv1.weight.double(), conv1.bias.double(), conv2.weight.double(), conv2.bias.double()
        ref1 = torch.nn.functional.conv3d(cl(x).double(), w1, b1, padding=1)
        put_module(arena, conv1), put_module(arena, conv2)
        dx, cnt = arena.put(x), arena.put(occ.view(B, -1).int())
        dsc, dsh = arena.put(sc), arena.put(sh)
        gs = run(arena, fused.conv3d_presplit, dx)
        assert gs.shape == (B, r, r, r, (C + 15) // 16 * 16)
        # first convolution: dense, compact
        y1, st1 = run(arena, fused.conv3d_k3, dx, conv1, compact=True, channels_last=True)
        y1p, st1p = run(arena, fused.conv3d_k3, gs, conv1, compact=True, channels_last=True, pre=True)
        eq(y1p, y1, "dense pre"), eq(st1p, st1, "dense pre statistics")
        assert rel_err(cl(y1p), ref1) < 1e-5
        assert rel_err(stats_of(st1p)[1], (ref1 * ref1).flatten(2).sum(2)) < TOL
        lists, counts = run(arena, fused.active_lists, cnt, r)
        c1, s1 = run(arena, fused.conv3d_k3_compact, dx, conv1, lists, counts, 0)
        c1p, s1p = run(arena, fused.conv3d_k3_compact, gs, conv1, lists, counts, 0, pre=True)
        eq(c1p, c1, "compact pre"), eq(s1p, s1, "compact pre statistics"), eq(c1p, y1, "compact == dense")
        # second convolution in far-field form: the operand is swish(y1 * scale + shift) - a, split once
        ref2 = torch.nn.functional.conv3d(swish(cl(y1.cpu()).double() * sc[:, :, None, None, None].double()
                                                + sh[:, :, None, None, None].double()), w2, b2, padding=1)
        a, k = run(arena, fused.conv3d_far_field, conv1.bias, conv2, dsc, dsh, True)
        op2 = run(arena, fused.conv3d_presplit, y1, dsc, dsh, True, a)
        c2, s2 = run(arena, fused.conv3d_k3_compact, y1, conv2, lists, counts, 1, dsc, dsh, True, in_sub=a, out_class=k)
        c2p, s2p = run(arena, fused.conv3d_k3_compact, op2, conv2, lists, counts, 1, out_class=k, pre=True)
        eq(c2p, c2, "compact pre, second"), eq(s2p, s2, "compact pre statistics, second")
        assert rel_err(cl(c2p), ref2) < 1e-5
        assert rel_err(stats_of(s2p)[1], (ref2 * ref2).flatten(2).sum(2)) < TOL
        d2p, t2p = run(arena, fused.conv3d_k3, run(arena, fused.conv3d_presplit, y1, dsc, dsh, True), conv2, compact=True,
                       channels_last=True, pre=True)
        d2, t2 = run(arena, fused.conv3d_k3, y1, conv2, dsc, dsh, swish=True, compact=True, channels_last=True)
        eq(d2p, d2, "dense pre, second"), eq(t2p, t2, "dense pre statistics, second")
        assert rel_err(cl(d2p), ref2) < 1e-5
        # listed_only: y is written in part. include/p2pb_hip.h, p2pb_conv3d_k3_forward_compact: "flags bit 5 (32 ...): the
        # constants of the UNLISTED voxels are left unwritten (statistics still exact)". The listed part (D2) and the statistics
        # are the full form's bits, the unlisted part is still the arena's poison
        c2l, s2l = run(arena, fused.conv3d_k3_compact, op2, conv2, lists, counts, 1, out_class=k, pre=True, listed_only=True,
                       partial=(0,))
        in_d2 = _dilate(_dilate(occ[:, None]))[:, 0] > 0
        assert 0 < in_d2.sum() < in_d2.numel()
        eq(s2l, s2p, "listed_only statistics"), eq(c2l.cpu()[in_d2], c2p.cpu()[in_d2], "listed_only, listed part")
        assert (bits(c2l).cpu()[~in_d2] == -1).all(), "listed_only wrote outside its set"
        if r == 16:  # the list-driven form (brick lists)
            bl, bc = run(arena, fused.brick_lists, cnt, r)
            b1, u1 = run(arena, fused.conv3d_k3_sparse, dx, conv1, bl, bc, 0, channels_last=True)
            b1p, u1p = run(arena, fused.conv3d_k3_sparse, gs, conv1, bl, bc, 0, channels_last=True, pre=True)
            eq(b1p, b1, "sparse pre"), eq(u1p, u1, "sparse pre statistics")
            assert rel_err(cl(b1p), ref1) < 1e-5
            b2, u2 = run(arena, fused.conv3d_k3_sparse, y1, conv2, bl, bc, 1, dsc, dsh, True, in_sub=a, out_class=k, channels_last=True)
            b2p, u2p = run(arena, fused.conv3d_k3_sparse, op2, conv2, bl, bc, 1, out_class=k, channels_last=True, pre=True)
            eq(b2p, b2, "sparse pre, second"), eq(u2p, u2, "sparse pre statistics, second")
            assert rel_err(cl(b2p), ref2) < 1e-5


# ---- 5. conv3d_far_field / conv3d_far_field_gn (csrc/conv3d_farfield.hip; tolerance FF_TOL, measured as stated above) ------

def far_field_ref(prev_bias, w, bias, scale, shift, on, dt):
    """a = act(prev_bias * scale + shift); K[b, cls] = the output at voxel (cd, ch, cw), cls = (cd * 3 + ch) * 3 + cw, of
    conv3d(padding = 1) on the 3 x 3 x 3 grid that holds a[b] in every voxel: every boundary class of a grid is one of its voxels"""
    a = act(prev_bias.to(dt)[None, :] * scale.to(dt) + shift.to(dt), on)
    b, ci = a.shape
    y = torch.nn.functional.conv3d(a.view(b, ci, 1, 1, 1).expand(b, ci, 3, 3, 3).contiguous(), w.to(dt), bias.to(dt), padding=1)
    return a, y.reshape(b, -1, 27).transpose(1, 2)


def check_far_field(what, a, k, prev_bias, w, bias, scale, shift, on):
    a64, k64 = far_field_ref(prev_bias, w, bias, scale, shift, on, F64)
    a32, k32 = far_field_ref(prev_bias, w, bias, scale, shift, on, torch.float32)
    note("far_field", f"host fp32 {what}", max(rel_err(a32, a64), rel_err(k32, k64)))
    assert a.shape == a64.shape and k.shape == k64.shape
    errs = [note("far_field", f"hip {what} a", rel_err(a, a64)), note("far_field", f"hip {what} K", rel_err(k, k64))]
    assert max(errs) < FF_TOL, errs


# ci = 8: one chunk of the weight pack; 24: three chunks, none of the four-at-a-time groups; 64 -> 48: two four-chunk groups,
# two 32-channel output blocks the second of them half full; co = 40: a ragged second block
@pytest.mark.parametrize("on", [True, False])
@pytest.mark.parametrize("b,ci,co,groups", [(2, 8, 16, 8), (1, 24, 40, 8), (2, 64, 48, 32)])
def test_conv3d_far_field(arena, fused, b, ci, co, groups, on):
    torch.manual_seed(ci + co)
    conv = torch.nn.Conv3d(ci, co, 3, padding=1)
    prev_bias = torch.randn(ci) * 0.1
    sc, sh = torch.rand(b, ci) + 0.5, torch.randn(b, ci)
    with torch.no_grad():
        w, bias = conv.weight.clone(), conv.bias.clone()  # host copies: the module's parameters move into the arena
        put_module(arena, conv)
        dpb = arena.put(prev_bias)
        a, k = run(arena, fused.conv3d_far_field, dpb, conv, arena.put(sc), arena.put(sh), on)
        check_far_field("plain", a, k, prev_bias, w, bias, sc, sh, on)
        # the merged launch, a short slot table (3 slots): scale / shift against the fp64 GroupNorm of the partials, a / K against
        # the far-field reference of the scale / shift it returned, and the two launches' bits (test_gn_merged_gpu.py)
        count, nslots = 512.0, 3
        part = _partials(b, nslots, ci, count, seed=2).cpu()
        host_norm, dev_norm = norm_pair(arena, ci, groups, b, b == 2, seed=3)
        dpart = arena.put(part)
        sc1, sh1, a1, k1 = run(arena, fused.conv3d_far_field_gn, dpb, conv, dpart, (count, groups, *dev_norm, 1e-5, False), on)
        check_gn("far_field_gn", (sc1, sh1, None), part, count, groups, host_norm, 1e-5)
        check_far_field("gn", a1, k1, prev_bias, w, bias, sc1.cpu(), sh1.cpu(), on)
        sc0, sh0, _ = run(arena, fused.gn_affine_params, dpart, count, groups, *dev_norm, 1e-5)
        a0, k0 = run(arena, fused.conv3d_far_field, dpb, conv, sc0, sh0, on)
        for name, u, v in (("scale", sc0, sc1), ("shift", sh0, sh1), ("a", a0, a1), ("K", k0, k1)):
            eq(v, u, f"merged {name}")


# ---- 6. pvconv_tail, minmax_act_pool_gn, minmax_act (csrc/pvconv_finish.hip, csrc/pointwise_act.hip; tolerance GN_TOL) -------

def tail_ref(part2, count2, groups2, norm2, eps2, se, point, dt):
    """the tail of a PVConv's voxel branch from the partials: the folded norm, the SE3d gate sigmoid(W2 relu(W1 chmean)) multiplied
    into scale and shift (test_fused_gpu.py::test_se_gate_affine), and the point branch's folded norm"""
    a, b_, chmean = gn_ref(part2, count2, groups2, *norm2, eps2, dt=dt)
    if se is not None:
        gate = torch.sigmoid(torch.relu(chmean @ se[0].to(dt).t()) @ se[1].to(dt).t())
        a, b_ = a * gate, b_ * gate
    if point is None:
        return a, b_, None, None
    partp, countp, groupsp, normp, epsp = point
    scp, shp, _ = gn_ref(partp, countp, groupsp, *normp, epsp, dt=dt)
    return a, b_, scp, shp


# (b, c, nslots2, cp, se, point): cg = 2, 5 and 25 channels per group (256 / cg partial accumulators per channel: 128, 51 -- one
# idle thread -- and 10 -- six idle threads), a slot table shorter than the accumulators (3), hidden = 2, 5, 25; all four
# combinations of se and point at cp = c, and one point branch of another width (cp = 24)
TAIL_CASES = [(b, c, ns, c, se, pt) for b, c, ns in [(2, 16, 8), (1, 40, 3), (2, 200, 64)] for se in (False, True)
              for pt in (False, True)] + [(2, 16, 8, 24, True, True)]


@pytest.mark.parametrize("styled", [False, True])
@pytest.mark.parametrize("b,c,nslots2,cp,with_se,with_point", TAIL_CASES)
def test_pvconv_tail(arena, fused, b, c, nslots2, cp, with_se, with_point, styled):
    torch.manual_seed(c + nslots2)
    n, count2, eps = 200, float(nslots2 * 64), 1e-5
    part2 = _partials(b, nslots2, c, count2, seed=5).cpu()
    host2, dev2 = norm_pair(arena, c, 8, b, styled, seed=6)
    se = dse = point = dpoint = None
    if with_se:
        se = (torch.randn(c // 8, c) * 0.2, torch.randn(c, c // 8) * 0.2)
        dse = (arena.put(se[0]), arena.put(se[1]))
    if with_point:
        partp = _partials(b, (n + 255) // 256 * 4, cp, float(n), seed=7).cpu()
        hostp, devp = norm_pair(arena, cp, 8, b, styled, seed=8)
        point = (partp, float(n), 8, hostp, eps)
        dpoint = (arena.put(partp), (float(n), 8, *devp, eps, False))
    dpart2 = arena.put(part2)
    got = run(arena, fused.pvconv_tail, dpart2, (count2, 8, *dev2, eps, True), dse, dpoint)
    ref = tail_ref(part2, count2, 8, host2, eps, se, point, F64)
    r32 = tail_ref(part2, count2, 8, host2, eps, se, point, torch.float32)
    assert (got[2] is None and got[3] is None) == (not with_point)
    errs = []
    for name, g, r, r_ in zip(("aff_a", "aff_b", "scale_p", "shift_p"), got, ref, r32):
        if r is not None:
            note("gn", "host fp32 pvconv_tail", rel_err(r_, r))
            assert g.shape == r.shape
            errs.append((name, note("gn", f"hip pvconv_tail {name}", rel_err(g, r))))
    assert all(e < GN_TOL for _, e in errs), errs
    # the four launches it replaces: the same bits (test_gn_merged_gpu.py)
    sc, sh, mean = run(arena, fused.gn_affine_params, dpart2, count2, 8, *dev2, eps, want_mean=True)
    ra, rb = run(arena, fused.se_gate_affine, mean, dse[0], dse[1], sc, sh) if with_se else (sc, sh)
    eq(got[0], ra, "aff_a == separate launches"), eq(got[1], rb, "aff_b == separate launches")
    if with_point:
        rscp, rshp, _ = run(arena, fused.gn_affine_params, dpoint[0], float(n), 8, *devp, eps)
        eq(got[2], rscp, "scale_p == gn_affine_params"), eq(got[3], rshp, "shift_p == gn_affine_params")


def pool_ref(mm, scale, shift, on, dt=F64):
    lo, hi = mm[..., 0].to(dt).amin(1), mm[..., 1].to(dt).amax(1)
    return torch.maximum(act(lo * scale.to(dt) + shift.to(dt), on), act(hi * scale.to(dt) + shift.to(dt), on))


# nmm = 2, 15: minmax_act's serial kernel (minmax_act_kernel, nslots > 0: one thread per (sample, channel) walks the slots); 16, 40:
# minmax_act_pool_kernel (8 slot classes per workgroup: two slots each, and five). minmax_act_pool_gn always takes the pool
# kernel: at nmm = 2 six of its slot classes stay empty. c = 8: a quarter of a 32-channel workgroup, one channel per group;
# c = 96: three workgroups, 12 channels per group, so a workgroup's channels span four groups
@pytest.mark.parametrize("on", [True, False])
@pytest.mark.parametrize("c", [8, 96])
@pytest.mark.parametrize("nmm", [2, 15, 16, 40])
def test_minmax_act_pool_gn(arena, fused, nmm, c, on):
    b, groups, eps = 2, 8, 1e-5
    npos = nmm * 64
    g = torch.Generator().manual_seed(nmm + c)
    lo = torch.randn(b, nmm, c, generator=g) - 1.0
    mm = torch.stack([lo, lo + torch.rand(b, nmm, c, generator=g) * 3], dim=-1)
    part = _partials(b, (npos + 255) // 256 * 4, c, float(npos), seed=9).cpu()
    host_norm, dev_norm = norm_pair(arena, c, groups, b, False, seed=11)
    dmm, dpart = arena.put(mm), arena.put(part)
    y, sc1, sh1 = run(arena, fused.minmax_act_pool_gn, dmm, dpart, (float(npos), groups, *dev_norm, eps, False), on)
    check_gn("minmax_act_pool_gn", (sc1, sh1, None), part, float(npos), groups, host_norm, eps)
    sc64, sh64, _ = gn_ref(part, float(npos), groups, *host_norm, eps)
    sc32, sh32, _ = gn_ref(part, float(npos), groups, *host_norm, eps, dt=torch.float32)
    ref = pool_ref(mm, sc64, sh64, on)
    note("gn", "host fp32 minmax_act_pool_gn", rel_err(pool_ref(mm, sc32, sh32, on, torch.float32), ref))
    assert y.shape == (b, c)
    assert note("gn", "hip minmax_act_pool_gn y", rel_err(y, ref)) < GN_TOL
    # minmax_act(global_pool=True) on host-built scale / shift (1e-5: test_pw_conv_global_pool), and the two launches' bits
    hsc, hsh = sc64.float(), sh64.float()
    got = run(arena, fused.minmax_act, dmm, arena.put(hsc), arena.put(hsh), on, global_pool=True)
    assert got.shape == (b, c) and rel_err(got, pool_ref(mm, hsc, hsh, on)) < 1e-5
    two = run(arena, fused.minmax_act, dmm, sc1, sh1, on, global_pool=True)
    if nmm >= 16:
        eq(y, two, "merged == gn_affine_params -> minmax_act")
    assert torch.allclose(y, two, rtol=0, atol=0)


# minmax_act_kernel's nslots == 0 arm (one thread per (sample, channel, neighbourhood)): 70 elements, less than one block and
# an odd row of 7; 8320 = 32 blocks and a half
@pytest.mark.parametrize("on", [True, False])
@pytest.mark.parametrize("B,C,M", [(2, 5, 7), (1, 64, 130)])
def test_minmax_act_per_neighbourhood(arena, fused, B, C, M, on):
    g = torch.Generator().manual_seed(C + M)
    lo = torch.randn(B, C, M, generator=g) - 1.0
    mm = torch.stack([lo, lo + torch.rand(B, C, M, generator=g) * 3], dim=-1)
    sc, sh = torch.randn(B, C, generator=g), torch.randn(B, C, generator=g)
    got = run(arena, fused.minmax_act, arena.put(mm), arena.put(sc), arena.put(sh), on)
    f = lambda t: act(t.double() * sc[:, :, None].double() + sh[:, :, None].double(), on)
    assert got.shape == (B, C, M) and rel_err(got, torch.maximum(f(mm[..., 0]), f(mm[..., 1]))) < 1e-5


# ---- 7. affine_act, affine_act_max, the pw_conv arms (tolerances: test_fused_gpu.py::test_affine_act_and_max, TOL) ----------

# P = 1: one element per row; 63 and 1021: the scalar kernel (P % 4 != 0), less than a block and four blocks less three; 1024:
# the 16-byte kernel, one full block of quads
@pytest.mark.parametrize("on", [True, False])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("B,C,P", [(2, 5, 1), (1, 24, 63), (2, 3, 1021), (1, 8, 1024)])
def test_affine_act(arena, fused, B, C, P, with_res, on):
    g = torch.Generator().manual_seed(C + P)
    x, res = torch.randn(B, C, P, generator=g), torch.randn(B, C, P, generator=g)
    sc, sh = torch.randn(B, C, generator=g), torch.randn(B, C, generator=g)
    ref = act(x.double() * sc[:, :, None].double() + sh[:, :, None].double(), on)
    if with_res:
        ref = ref + res.double()
    got = run(arena, fused.affine_act, arena.put(x), arena.put(sc), arena.put(sh), on, arena.put(res) if with_res else None)
    assert got.shape == (B, C, P) and rel_err(got, ref) < (1e-5 if on else 1e-6)


@pytest.mark.parametrize("M,U", [(48, 32), (8, 8)])
def test_affine_act_max(arena, fused, M, U):
    """(8, 8): 64 positions, the smallest plane the launcher takes at u = 8 (see the refusal below)"""
    B, C = 2, 24
    g = torch.Generator().manual_seed(M + U)
    x = torch.randn(B, C, M * U, generator=g)
    sc, sh = torch.randn(B, C, generator=g), torch.randn(B, C, generator=g)
    z = swish(x.double() * sc[:, :, None].double() + sh[:, :, None].double())
    got = run(arena, fused.affine_act_max, arena.put(x), arena.put(sc), arena.put(sh), M, U)
    assert got.shape == (B, C, M) and rel_err(got, z.view(B, C, M, U).amax(3)) < 1e-5


def test_affine_act_max_refuses_a_plane_of_56(arena, fused):
    """(M, U) = (7, 8) cannot reach affine_act_max_kernel: p2pb_affine_act_max (csrc/pointwise_act.hip) takes planes of whole waves
    only, (m * u) % 64 == 0, and returns P2PB_EINVAL for 7 x 8 = 56 positions before anything is launched (the network's planes
    are 32-neighbour ones). The refusal is what is held here: an error, nothing allocated beyond the result, no guard touched."""
    B, C, M, U = 2, 24, 7, 8
    x, sc, sh = arena.put(torch.randn(B, C, M * U)), arena.put(torch.randn(B, C)), arena.put(torch.randn(B, C))
    with pytest.raises(RuntimeError, match="p2pb_affine_act_max failed with code -22"):
        fused.affine_act_max(x, sc, sh, M, U)
    arena.check_guards()


# the whole-row maximum (u = 0, affine_act_rowmax_kernel: 256 threads per row): a row of four strides less three, and of four
@pytest.mark.parametrize("P", [1021, 1024])
def test_affine_act_max_global(arena, fused, P):
    B, C = 2, 24
    g = torch.Generator().manual_seed(P)
    x = torch.randn(B, C, P, generator=g)
    sc, sh = torch.randn(B, C, generator=g), torch.randn(B, C, generator=g)
    z = swish(x.double() * sc[:, :, None].double() + sh[:, :, None].double())
    got = run(arena, fused.affine_act_max, arena.put(x), arena.put(sc), arena.put(sh), P, 0)
    assert got.shape == (B, C) and rel_err(got, z.amax(2)) < 1e-5


@pytest.mark.parametrize("math", [None, "fp32"])
def test_pw_conv_point_major(arena, fused, math):
    """point_major=True (flags bit 5): y f32[B, P, Cout]; by default the narrow-layer f16x3 kernel, with math="fp32" the
    streaming fp32 one"""
    B, ci, co, P = 2, 40, 24, 52
    torch.manual_seed(ci + co + P)
    x = torch.randn(B, ci, P)
    conv = torch.nn.Conv1d(ci, co, 1)
    with torch.no_grad():
        ref = torch.nn.functional.conv1d(x.double(), conv.weight.double(), conv.bias.double())
        put_module(arena, conv)
        dx = arena.put(x)
        y, st = run(arena, fused.pw_conv, dx, conv, stats=False, point_major=True, math=math)
        assert st is None and y.shape == (B, P, co) and rel_err(y.transpose(1, 2), ref) < TOL
        eq(y.transpose(1, 2), run(arena, fused.pw_conv, dx, conv, stats=False, math=math)[0], "point-major == channel-major")


@pytest.mark.parametrize("P", [52, 53])  # 16-byte rows (the wide kernels), and rows that are not (pw_conv_kernel)
def test_pw_conv_channel_slices(arena, fused, P):
    """W [g ; skip] + bias as W[:, :40] g (no bias) + (W[:, 40:] skip + bias): both input-channel slices of one Conv1d(40 + 16, 24)"""
    B, cg, cs, co = 2, 40, 16, 24
    torch.manual_seed(P)
    g, skip = torch.randn(B, cg, P), torch.randn(B, cs, P)
    conv = torch.nn.Conv1d(cg + cs, co, 1)
    with torch.no_grad():
        w, bias = conv.weight.double(), conv.bias.double()
        put_module(arena, conv)
        ya, sta = run(arena, fused.pw_conv, arena.put(g), conv, stats=False, ci_lo=0, ci_hi=cg, use_bias=False)
        yb, stb = run(arena, fused.pw_conv, arena.put(skip), conv, ci_lo=cg, ci_hi=cg + cs)
        refb = torch.nn.functional.conv1d(skip.double(), w[:, cg:], bias)
        assert sta is None and rel_err(ya, torch.nn.functional.conv1d(g.double(), w[:, :cg])) < TOL
        assert rel_err(yb, refb) < TOL and rel_err(stats_of(stb)[1], (refb * refb).sum(2)) < TOL


@pytest.mark.parametrize("styled,want_mean", [(False, False), (True, True), (False, True)])
def test_pw_conv_fin(arena, fused, styled, want_mean):
    """fin=: the GroupNorm that follows, finished behind the producer (scale, shift, channel mean of the layer's own partials)"""
    B, ci, co, P, groups = 2, 40, 24, 52, 8
    torch.manual_seed(ci + P)
    x = torch.randn(B, ci, P) * 2 + 0.5
    conv = torch.nn.Conv1d(ci, co, 1)
    with torch.no_grad():
        ref = torch.nn.functional.conv1d(x.double(), conv.weight.double(), conv.bias.double())
        put_module(arena, conv)
        host_norm, dev_norm = norm_pair(arena, co, groups, B, styled, seed=P)
        dx = arena.put(x)
        y, st, aff = run(arena, fused.pw_conv, dx, conv, fin=(float(P), groups, *dev_norm, 1e-5, want_mean))
        assert rel_err(y, ref) < TOL and rel_err(stats_of(st)[1], (ref * ref).sum(2)) < TOL
        assert (aff[2] is not None) == want_mean
        check_gn("pw_conv fin", aff, st, float(P), groups, host_norm, 1e-5, want_mean)
        # what the folded affine is for: y * scale + shift is the GroupNorm (+ style) of the fp64 convolution
        gn = torch.nn.functional.group_norm(ref, groups, host_norm[0].double(), host_norm[1].double(), 1e-5)
        if styled:
            gn = gn * host_norm[2][:, :co, None].double() + host_norm[2][:, co:, None].double()
        assert rel_err(ref * aff[0].double().cpu()[:, :, None] + aff[1].double().cpu()[:, :, None], gn) < TOL
        y0, st0 = run(arena, fused.pw_conv, dx, conv)
        eq(y, y0, "y with fin"), eq(st, st0, "statistics with fin")
        # the pooling entry point takes the same finisher: same partials, same affine
        none, st_p, mm, aff_p = run(arena, fused.pw_conv, dx, conv, pool_u=4, store=False,
                                    fin=(float(P), groups, *dev_norm, 1e-5, want_mean))
        assert none is None
        eq(st_p, st, "pooled statistics with fin")
        for u, v in zip(aff, aff_p):
            assert (u is None and v is None) or torch.equal(u, v)
        pooled = ref.view(B, co, P // 4, 4)
        assert rel_err(mm[..., 0], pooled.amin(3)) < TOL and rel_err(mm[..., 1], pooled.amax(3)) < TOL


def test_pw_conv_wide_layer_prepass(arena, fused):
    """co = 520 = nine 64-channel blocks on the non-split arm (ci = 8 < PW_SPLIT_MIN_CIN) with in_scale given: pw_conv applies the
    folded norm + Swish in one affine_act pass and runs the plain GEMM on its result"""
    B, ci, co, P = 1, 8, 520, 12
    assert not fused.use_split_pw(ci, co, P) and (co + 63) // 64 >= 9
    torch.manual_seed(co)
    x = torch.randn(B, ci, P)
    conv = torch.nn.Conv1d(ci, co, 1)
    sc, sh = torch.rand(B, ci) + 0.5, torch.randn(B, ci)
    with torch.no_grad():
        ref = torch.nn.functional.conv1d(swish(x.double() * sc[:, :, None].double() + sh[:, :, None].double()), conv.weight.double(),
                                         conv.bias.double())
        put_module(arena, conv)
        dx, dsc, dsh = arena.put(x), arena.put(sc), arena.put(sh)
        n0 = arena.n_allocations
        y, st = run(arena, fused.pw_conv, dx, conv, dsc, dsh, swish=True)
        assert any(r["shape"] == (B, ci, P) and "fused.py" in r["where"] for r in arena.records[n0:]), "the pre-pass did not run"
        assert rel_err(y, ref) < TOL and rel_err(stats_of(st)[1], (ref * ref).sum(2)) < TOL
