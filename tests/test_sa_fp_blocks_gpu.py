"""PointNetSAModule, PointNetFPModule and Pnet2Stage (pvcnn_unet.py), each built alone, on every dispatch path of its forward,
against the float64 restatement tests/blocks_ref.py (pinned to the CPU oracle by tests/test_blocks_ref.py).

The discrete decisions -- FPS centres, ball-query lists, 3-NN indices -- come from the product's integer ops
(furthest_point_sampling_forward, ball_query, three_nn), which test_ops_parity_gpu.py and test_oracle_bruteforce.py pin to the
oracle; every value is then computed in float64 on the CPU (the interpolation weights included), so a rounding flip cannot make
a case flaky. `_form()` asserts, with the predicates the modules themselves use, which branch each case takes: a case cannot
drift onto another branch unnoticed.

Path ids, the branch predicates asserted, and the branch reached (pvcnn_unet.py):
  S1   geo, fused, pm (N % 4 == M % 4 == 0), two layers, gather_pool_supported      -> pw_conv_pool_gather (f16x3 only)
  S2   geo, fused, pm, three layers (S2) / c1 % 8 != 0 (S2b): no gather-pool; pool_supported(M U, U)
                                                                                     -> group_sub point-major, _run_fused(first) pooled
  S3   the same with U = 12 (S3) / U = 2 (S3b): pool_supported false                 -> _run_fused(first), unpooled tail:
       act_max_supported false (S3): affine_act + row maximum; true (S3b): affine_act_max
  S4   geo, fused, not pm (N = 301, M = 37)                                          -> group_sub channel-major (+ workspace)
  S5   one layer: nl == 1 with first; U = 16 (S5a): affine_act_max, U = 12 (S5b): affine_act + row maximum
  S6   use_split_pw(128, 128, M U) (false under fp32)                                -> split-operand GEMM inside _run_fused, 3 arithmetics
  S7   geo, eval, grad enabled: fused.enabled false                                  -> group_concat -> mlp.run -> dense
  S8   no geo, eval, no_grad                                                         -> FPS + BallQuery + _run_fused(first=None)
  S9   training (and with P2PB_EXPERIMENT group_concat=0: grouping + cat)            -> dense forward + every gradient
  S10  data.features is None on the geo path (fused, and eval with grad) and the no-geo path
  F1   geo, fused, skip + lower_temb, pm (M % 4 == 0)                                -> interp_add(add=) point-major, time bias
  F2   geo, fused, no skip (bias = conv0.bias), with and without lower_temb
  F3   geo, fused, M % 4 != 0                                                        -> interp_add channel-major (+ workspace)
  F4   M = 3 (every fine point interpolates from the same three)
  F5   one layer: nl == 1 with first                                                 -> affine_act
  F6   the network's fallback: temb concatenated into lower_features (Cg = 30), lower_temb None; and the F1 case in that
       form, against the SAME reference tensor as F1
  F7   geo, eval, grad enabled                                                       -> three_interpolate + cat + dense
  F8   no geo: nearest_neighbor_interpolate; eval no_grad and training with all gradients
  P1   _fusable, pool_supported(N, 0)                                                -> pooled GEMM epilogues + minmax_act_pool_gn
  P2   _fusable, N % 4 != 0: pool_supported false                                    -> affine_act_max
  P3   not _fusable: widths 40 and 72 (MyGroupNorm passes C % 32 channels through)   -> dense, eval no_grad and training
  P4   not _fusable: last_mlp_layers non-empty                                       -> dense, eval
  P5   training: every parameter's and the coordinates' gradient

Pooled forms compute max(act(a min + b), act(a max + b)), right only because Swish is quasi-convex: every set-abstraction
and Pnet2Stage case draws its GroupNorm bias from N(BIAS_MEAN, 1) and weight from U(0.5, 1.5) and asserts, on the float64
reference, that at least MIN_SHARE of the pooled rows take their value from the row MINIMUM (a kernel pooling the maximum alone
fails them). Shares of the cases at BIAS_MEAN = -2, computed on the CPU with the oracle's FPS / ball query: see SA_CASES.

Tolerances (test_pvconv_block_gpu.py's): outputs within TOL = 1e-4 of max|ref| AND every output channel within TOL of its own
max|ref|; gradients by relative L2 per tensor under GRAD_TOL = 5e-4. Every case prints what it measured (`pytest -rP`).

Measured on an MI355X (worst over the cases of the path, under P2PB_CONV_MATH=f16x3 and =bf16x6), error / max|ref| and worst
per-channel error / that channel's max|ref|:
    S1 3.1e-7 / 5.3e-6   S2 6.3e-7 / 1.2e-5   S2b 3.9e-7 / 2.9e-6   S3 3.9e-7 / 1.6e-6   S3b 2.5e-7 / 1.8e-6   S4 3.4e-7 / 1.4e-6
    S5 2.2e-7 / 1.4e-6   S6 6.0e-7 / 5.2e-6 (f16x3 3.6e-6, bf16x6 2.6e-6, fp32 5.2e-6)    S7 3.4e-7 / 1.4e-6   S8 3.4e-7 / 5.3e-6
    S9 3.4e-7 / 5.3e-6, gradients (relative L2) <= 6.3e-6 (group_concat=0: the same)      S10 7.8e-7 / 1.4e-6
    F1 3.1e-7 / 1.1e-6   F2 3.4e-7 / 1.3e-6   F3 2.0e-7 / 4.9e-7   F4 2.8e-7 / 4.7e-7   F5 2.4e-7 / 3.2e-7   F6 4.2e-7 / 1.5e-6
    F7 2.1e-7 / 6.6e-7   F8 4.7e-7 / 1.1e-6, gradients <= 6.6e-6
    P1 9.7e-7 / 3.9e-6   P2 4.2e-7 / 6.0e-6   P3 1.0e-6 / 7.9e-6, gradients <= 1.7e-5   P4 2.5e-6 / 2.8e-5 (the restatement's
    own fp32 evaluation: 2.4e-5)   P5 1.4e-6 / 7.3e-6, gradients <= 2.3e-5
S4 prints which pooling form ran: 37 * 8 = 296 positions, pool_supported -> the pooled epilogue.
Wall time of the 40 tests on an MI355X: 4 s (one skip, S1, under bf16x6).

Found by these tests and fixed in pvcnn_unet.py: the geo branch of PointNetSAModule dereferenced data.features = None (S10);
SharedMLP._run_fused handed affine_act_max planes its kernel refuses -- U no power of two, or M U no multiple of 64 -- and
the set abstraction ended in `p2pb_affine_act_max failed with code -22` (S3, S5 at U = 12)."""
import functools

import pytest
import torch

import blocks_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-4
GRAD_TOL = 5e-4  # relative L2 per gradient tensor
E = 16  # cond_dim of the AdaGN cases and width of the time embedding
B = 2
BIAS_MEAN = -2.0
MIN_SHARE = 0.05
MATHS = ("f16x3", "bf16x6", "fp32")

# radius: about 2 sqrt(U / N) -- a cap of chord r holds N r^2 / 4 of N points on the unit sphere, so the mean count in range is
# about U and both kinds of neighbourhood occur: lists padded with their first index (fewer than U in range) and full ones.
# Measured on the CPU (the oracle's FPS and ball query, the float64 reference alone) -- fraction of centres with a padded list /
# with a full list / share of pooled rows taken from the row minimum at BIAS_MEAN = -2:
#   S1 0.43 / 0.57 / 0.44   S2 0.54 / 0.46 / 0.56   S2b 0.52 / 0.48 / 0.60   S3 0.49 / 0.51 / 0.65   S3b 0.23 / 0.77 / 0.36   S4 0.32 / 0.68 / 0.49
#   S5a 0.40 / 0.60 / 0.48  S5b 0.51 / 0.49 / 0.56  S6 0.48 / 0.52 / 0.46    S10 0.42 / 0.58 / 0.84
#   Pnet2Stage (first / second maximum): P1 0.54 / 0.68   P2 0.58 / 0.67   P3 0.49 / 0.62   P4 0.47 / 0.61
# (radii of 0.3 at N = 256 and 0.12 at N = 301 would hold about 6 and 1 points on average, far below these U)
SA_CASES = {
    "S1": dict(N=256, M=64, U=16, C=13, widths=[24, 40], radius=0.5, cond=True, temb=True),
    "S2": dict(N=256, M=64, U=32, C=13, widths=[32, 32, 64], radius=0.7, cond=True, temb=False),
    # (c1 = 20 is no multiple of 8: the module is built with gn_groups = 4)
    "S2b": dict(N=256, M=64, U=32, C=13, widths=[20, 40], radius=0.7, cond=False, temb=False, groups=4),
    "S3": dict(N=256, M=64, U=12, C=13, widths=[24, 40], radius=0.43, cond=False, temb=False),
    # (U = 2: no pooled epilogue either -- pool_supported takes 4 .. 64 --, but a plane the affine_act_max kernel itself takes)
    "S3b": dict(N=256, M=64, U=2, C=13, widths=[24, 40], radius=0.18, cond=True, temb=False),
    "S4": dict(N=301, M=37, U=8, C=5, widths=[40, 24], radius=0.33, cond=True, temb=True),
    "S5a": dict(N=256, M=64, U=16, C=13, widths=[32], radius=0.5, cond=True, temb=False),
    "S5b": dict(N=256, M=64, U=12, C=13, widths=[32], radius=0.43, cond=False, temb=False),
    "S6": dict(N=256, M=64, U=16, C=13, widths=[128, 128], radius=0.5, cond=True, temb=False),
    "S10": dict(N=256, M=64, U=16, C=None, widths=[24, 40], radius=0.5, cond=False, temb=False),
}
FP_CASES = {
    "F1": dict(N=256, M=64, Cg=32, Cs=19, widths=[40, 24], cond=True, temb=True),
    "F2a": dict(N=256, M=64, Cg=32, Cs=None, widths=[40, 24], cond=False, temb=True),
    "F2b": dict(N=256, M=64, Cg=32, Cs=None, widths=[40, 24], cond=True, temb=False),
    "F3": dict(N=301, M=37, Cg=32, Cs=19, widths=[40, 24], cond=True, temb=True),
    "F4": dict(N=64, M=3, Cg=32, Cs=19, widths=[40, 24], cond=False, temb=True),
    "F5": dict(N=256, M=64, Cg=32, Cs=19, widths=[24], cond=True, temb=True),
    "F6": dict(N=256, M=64, Cg=30, Cs=19, widths=[40, 24], cond=True, temb=True),
}
# (mlp1, mlp2) as Pnet2Stage takes them: mlp2's channel list is [2 * mlp1[-1]] + mlp2.
#
# Pnet2Stage's output is [B, C]: a channel's "own max|ref|" is the larger of B = 2 pooled values, each Swish(x*) of ONE winning
# pre-activation x*. Both samples share the channel's (weight, bias) and their normalised rows have the same spread, so in a
# channel whose bias is about -2.8 times its weight BOTH winners sit at Swish's zero crossing. There the relative error of
# the value is |Swish'(x) / Swish(x)| dx ~ dx / |x|: with the dx ~ 3e-6 that fp32 leaves on a pre-activation after four to six
# layers, a winner at |x*| = 0.02 is 1e-4 of its channel's maximum away from float64 in ANY fp32 evaluation (measured: the
# restatement itself in fp32 1.2e-4 (P1) and 2.2e-4 (P4) per channel at 1e-6 of the tensor's maximum; torch's fp32 CPU kernels
# the same). Such a draw measures the zero crossing, not the kernel. So the bias of the LAST norm is drawn from
# N(BIAS_MEAN, 1) conditioned on |x*| >= PNET_MIN_WINNER for every (sample, channel) of the float64 reference: a channel that
# misses it draws its bias again (pnet_setup; a bias of the last norm moves that channel's pre-activations and nothing else).
# |x*| >= 0.3 bounds the amplification 1 / |x| + 1 by 4.4: per-channel floor 1.3e-5, an eighth of TOL. Rows won by their
# very negative minimum are untouched: Swish'(x) / Swish(x) -> 1 there. Asserted by _pnet_case; drawn from the reference alone.
PNET_MIN_WINNER = 0.3
PNET_CASES = {
    "P1": dict(N=256, mlp1=[3, 32, 64], mlp2=[128, 256]),
    "P2": dict(N=301, mlp1=[3, 32, 64], mlp2=[128, 256]),
    "P3": dict(N=256, mlp1=[3, 40, 72], mlp2=[72, 96]),
    "P4": dict(N=256, mlp1=[3, 32, 32, 64], mlp2=[64, 128, 256]),
}


def _form(key, math=None):
    """the branch the case takes, from the predicates of PointNetSAModule.forward / SharedMLP._run_fused /
    PointNetFPModule.forward / Pnet2Stage.forward -- asserted to be the one the case is there for"""
    from p2p_bridge_amd import fused

    math = math or fused.conv_math()
    if key in SA_CASES:
        c = SA_CASES[key]
        N, M, U, w = c["N"], c["M"], c["U"], c["widths"]
        pm = N % 4 == 0 and M % 4 == 0
        gather = pm and len(w) == 2 and fused.gather_pool_supported(w[0], w[1], M, U)
        pool = len(w) > 1 and fused.pool_supported(M * U, U)
        split = any(fused.use_split_pw(a, b, M * U) for a, b in zip(w[:-1], w[1:]))
        want = {"S1": (True, True, True, False), "S2": (True, False, True, False), "S2b": (True, False, True, False),
                "S3": (True, False, False, False), "S3b": (True, False, False, False), "S4": (False, False, True, False), "S5a": (True, False, False, False),
                "S5b": (True, False, False, False), "S6": (True, False, True, math != "fp32"),
                "S10": (True, True, True, False)}[key]
        if math != "f16x3" and key in ("S1", "S10"):  # (the gather-pool kernel exists in the f16x3 arithmetic only)
            want = (True, False, True, False)
        assert (pm, gather, pool, split) == want, (key, math, (pm, gather, pool, split))
        if key == "S2b":
            assert w[0] % 8 != 0
        # the unpooled tail: affine_act_max takes power-of-two neighbourhoods in whole waves; else affine_act + row maximum
        act_max = fused.act_max_supported(M, U)
        if key in ("S3", "S3b", "S5a", "S5b"):
            assert act_max == (key in ("S3b", "S5a")), (key, act_max)
        return dict(pm=pm, gather=gather, pool=pool, split=split, act_max=act_max)
    if key in FP_CASES:
        c = FP_CASES[key]
        pm = c["M"] % 4 == 0
        assert pm == (key not in ("F3", "F4")), key
        if key == "F6":
            assert c["Cg"] % 4 != 0  # (the predicate under which PVCNN2Unet.forward concatenates instead of passing lower_temb)
        return dict(pm=pm)
    c = PNET_CASES[key]
    return dict(pool=fused.pool_supported(c["N"], 0))


# ------------------------------------------------------------------------------------------------- inputs and modules


def _cloud(N, gen):
    """a noisy unit sphere f32[B,3,N] (test_pvconv_block_gpu._cloud "surface")"""
    p = torch.randn(B, 3, N, generator=gen, dtype=torch.float64)
    return (p / p.norm(dim=1, keepdim=True) + 0.01 * torch.randn(B, 3, N, generator=gen, dtype=torch.float64)).float()


def _randomise(mod, gen, pooled):
    """the norms' affine parameters away from (1, 0) and the style Linears away from their small initial weights, so that a
    swapped / dropped one shows; pooled: weight U(0.5, 1.5), bias N(BIAS_MEAN, 1) (the rows pooled at their minimum)"""
    from p2p_bridge_amd.pvcnn_unet import AdaGN

    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, torch.nn.GroupNorm):
                if pooled:
                    m.weight.copy_(0.5 + torch.rand(m.weight.shape, generator=gen))
                    m.bias.copy_(BIAS_MEAN + torch.randn(m.bias.shape, generator=gen))
                else:
                    m.weight.add_(0.3 * torch.randn(m.weight.shape, generator=gen))
                    m.bias.add_(0.3 * torch.randn(m.bias.shape, generator=gen))
            elif isinstance(m, AdaGN):
                m.emd.weight.copy_(0.2 * torch.randn(m.emd.weight.shape, generator=gen))
                m.emd.bias.add_(0.1 * torch.randn(m.emd.bias.shape, generator=gen))
    return mod


def _seed(key):
    return sum(ord(ch) * (31 ** i) for i, ch in enumerate(key)) % 100000


def sa_setup(key, device="cuda"):
    """-> (module, inputs dict) of a set-abstraction case; deterministic per key (built on the CPU, then moved)"""
    from p2p_bridge_amd.pvcnn_unet import PointNetSAModule

    c = SA_CASES[key]
    torch.manual_seed(_seed(key))
    mod = PointNetSAModule(c["M"], c["radius"], c["U"], c["C"] or 0, list(c["widths"]), gn_groups=c.get("groups", 8),
                           cond_dim=E if c["cond"] else 0)
    mod.level = 0
    gen = torch.Generator().manual_seed(_seed(key) + 1)
    _randomise(mod, gen, True)
    inp = dict(coords=_cloud(c["N"], gen), feats=None if c["C"] is None else torch.randn(B, c["C"], c["N"], generator=gen),
               te=torch.randn(B, E, generator=gen) if c["temb"] else None,
               cond=torch.randn(B, E, generator=gen) if c["cond"] else None,
               gy=torch.randn(B, c["widths"][-1], c["M"], generator=gen))
    return mod.to(device), {k: (None if v is None else v.to(device)) for k, v in inp.items()}


def fp_setup(key, device="cuda"):
    from p2p_bridge_amd.pvcnn_unet import PointNetFPModule

    c = FP_CASES[key]
    torch.manual_seed(_seed(key))
    mod = PointNetFPModule(c["Cg"] + (E if c["temb"] else 0) + (c["Cs"] or 0), list(c["widths"]), cond_dim=E if c["cond"] else 0)
    mod.level = 0
    gen = torch.Generator().manual_seed(_seed(key) + 1)
    _randomise(mod, gen, False)
    inp = dict(coords=_cloud(c["N"], gen), g=torch.randn(B, c["Cg"], c["M"], generator=gen),
               skip=None if c["Cs"] is None else torch.randn(B, c["Cs"], c["N"], generator=gen),
               te=torch.randn(B, E, generator=gen) if c["temb"] else None,
               cond=torch.randn(B, E, generator=gen) if c["cond"] else None,
               gy=torch.randn(B, c["widths"][-1], c["N"], generator=gen))
    return mod.to(device), {k: (None if v is None else v.to(device)) for k, v in inp.items()}


def pnet_setup(key, device="cuda"):
    from p2p_bridge_amd.pvcnn_unet import Pnet2Stage

    c = PNET_CASES[key]
    torch.manual_seed(_seed(key))
    mod = Pnet2Stage(list(c["mlp1"]), list(c["mlp2"]))
    gen = torch.Generator().manual_seed(_seed(key) + 1)
    _randomise(mod, gen, True)
    inp = dict(coords=_cloud(c["N"], gen), gy=torch.randn(B, c["mlp2"][-1], generator=gen))
    last = (list(mod.mlp2.last_mlp_layers) or [mod.mlp2.shared_mlp_1])[-1].mlp[1].group_norm
    assert last.num_channels == c["mlp2"][-1]
    for _ in range(50):  # (PNET_MIN_WINNER: the last norm's bias, conditioned on no winner at Swish's zero crossing)
        bad = pnet_winners(mod, inp["coords"]).abs().amin(0) < PNET_MIN_WINNER
        if not bad.any():
            break
        with torch.no_grad():
            last.bias[bad] = BIAS_MEAN + torch.randn(int(bad.sum()), generator=gen)
    return mod.to(device), {k: v.to(device) for k, v in inp.items()}


def pnet_winners(mod, coords):
    """the pre-activation x* [B, C] whose Swish is the pooled output, per (sample, channel) of the float64 reference"""
    keep = {}
    with torch.no_grad():
        R.pnet2_stage(_d(coords), _params64(mod), keep)
    lo, hi = keep["mlp2"].min(dim=-1).values, keep["mlp2"].max(dim=-1).values
    return torch.where(R.swish(lo) > R.swish(hi), lo, hi)


def _params64(mod, grad=False):
    return {k: v.detach().double().cpu().requires_grad_(grad) for k, v in mod.named_parameters()}


def _d(t, grad=False):
    return None if t is None else t.detach().double().cpu().requires_grad_(grad)


# ------------------------------------------------------------------------------------------------- decisions and references


def sa_decisions(coords, c, ops):
    """(FPS indices i32[B,M], ball-query lists i32[B,M,U]) from `ops` (the product's extension module; oracle.cpu_ops in
    test_blocks_ref.py, which checks the cases' input conditions without a GPU); both kinds of neighbourhood must occur"""
    coords = coords.contiguous()
    fps = ops.furthest_point_sampling_forward(coords, c["M"])
    nidx = ops.ball_query(ops.gather_features_forward(coords, fps), coords, c["radius"], c["U"])
    full = nidx[:, :, -1] != nidx[:, :, 0]  # (a list with fewer than U points in range repeats its first index to the end)
    n_full, n_padded = int(full.sum()), int((~full).sum())
    assert n_full > 0 and n_padded > 0, (n_full, n_padded)
    return fps, nidx, n_padded / full.numel()


@functools.lru_cache(maxsize=None)
def _sa_case(key):
    """module, inputs, decisions and the float64 reference of a case: computed once, shared by the tests of every path that
    runs the case, and left unchanged"""
    from p2p_bridge_amd import pointnet2_batch_cuda as ext

    c = SA_CASES[key]
    mod, inp = sa_setup(key)
    fps, nidx, padded = sa_decisions(inp["coords"], c, ext)
    temb = None if inp["te"] is None else inp["te"][:, :, None].expand(-1, -1, c["N"])
    keep = {}
    with torch.no_grad():
        ref = R.sa_block(_d(inp["feats"]), _d(inp["coords"]), _d(temb), _d(inp["cond"]), _params64(mod), fps.cpu(), nidx.cpu(),
                         groups=c.get("groups", 8), keep=keep)
    share = R.min_share(keep["pre_act"])
    print(f"MEASURED {key} padded lists {padded:.2f} full {1 - padded:.2f}; pooled rows taken from the row minimum {share:.3f}")
    assert share >= MIN_SHARE, (key, share)
    return mod, inp, (fps, nidx), ref


def fp_decisions(coords, M, ops):
    """(coarse coordinates = the FPS centres f32[B,3,M], 3-NN indices i32[B,3,N])"""
    coords = coords.contiguous()
    lower = ops.gather_features_forward(coords, ops.furthest_point_sampling_forward(coords, M))
    idx3 = ops.three_nearest_neighbors_interpolate_forward(coords, lower, lower)[1]
    return lower, idx3


@functools.lru_cache(maxsize=None)
def _fp_case(key):
    from p2p_bridge_amd import pointnet2_batch_cuda as ext

    c = FP_CASES[key]
    mod, inp = fp_setup(key)
    lower, idx3 = fp_decisions(inp["coords"], c["M"], ext)
    assert torch.equal(ext.three_nn(inp["coords"].contiguous(), lower)[0], idx3)  # (the geometry stream's search: the same lists)
    with torch.no_grad():
        ref = R.fp_block(_d(inp["coords"]), _d(inp["skip"]), _d(lower), _d(inp["g"]), _d(inp["te"]), _d(inp["cond"]),
                         _params64(mod), idx3.cpu())
    return mod, inp, (lower, idx3), ref


@functools.lru_cache(maxsize=None)
def _pnet_case(key):
    mod, inp = pnet_setup(key)
    keep = {}
    with torch.no_grad():
        ref = R.pnet2_stage(_d(inp["coords"]), _params64(mod), keep)
        ref32 = R.pnet2_stage(inp["coords"].cpu(), {k: v.detach().cpu() for k, v in mod.named_parameters()}).double()
    shares = {k: R.min_share(v) for k, v in keep.items()}
    own = ((ref32 - ref).abs().amax(0) / ref.abs().amax(0)).max().item()
    winner = pnet_winners(mod, inp["coords"]).abs().min().item()
    print(f"MEASURED {key} pooled rows taken from the row minimum {shares}; smallest winning |pre-activation| {winner:.3f}; "
          f"the restatement's own fp32 per-channel error {own:.2e}")
    assert min(shares.values()) >= MIN_SHARE, (key, shares)
    assert winner >= PNET_MIN_WINNER, (key, winner)  # (see PNET_CASES)
    return mod, inp, ref


# ------------------------------------------------------------------------------------------------- comparisons


def _check_out(out, ref, what):
    """-> (error / max|ref|, worst per-channel error / that channel's max|ref|), asserted below TOL"""
    out, ref = out.detach().double().cpu(), ref.detach()
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    assert torch.isfinite(out).all(), what
    err = (out - ref).abs()
    dims = tuple(d for d in range(ref.dim()) if d != 1)
    glob = err.max().item() / ref.abs().max().item()
    per = (err.amax(dims) / ref.abs().amax(dims).clamp(min=1e-30)).max().item()
    print(f"MEASURED {what} out {glob:.2e} per-channel {per:.2e}")
    assert glob < TOL, (what, glob)
    assert per < TOL, (what, per)
    return glob, per


def _rel_l2(a, b, scale=None):
    den = b.norm() if scale is None else torch.maximum(b.norm(), scale.norm())
    return ((a.detach().double().cpu() - b).norm() / den.clamp(min=1e-30)).item()


def _check_grads(mod, mine, ref, what):
    """mine / ref: name -> gradient (product fp32 / float64 autograd); every parameter of `mod` joins under its own name.
    A convolution's bias in front of a GroupNorm with ONE channel per group only moves that group's mean: its exact gradient is 0
    and a relative error has no meaning -- it is measured against the gradient of the same layer's weight there"""
    mine = dict(mine, **{k: v.grad for k, v in mod.named_parameters()})
    one_per_group = set()
    mods = dict(mod.named_modules())
    for name, m in mods.items():
        if isinstance(m, torch.nn.GroupNorm) and m.num_channels == m.num_groups:
            # SharedMLP: layers.{3i} conv, layers.{3i+1}[.norm]; _PnetMLP: mlp.0 conv, mlp.1.group_norm
            head, idx = name.replace(".group_norm", "").replace(".norm", "").rsplit(".", 1)
            conv = f"{head}.{int(idx) - 1}"
            if mods[conv].out_channels == m.num_channels:
                one_per_group.add(conv + ".bias")
    worst = (0.0, None)
    for name, g64 in ref.items():
        assert mine.get(name) is not None and g64 is not None, (what, name)
        scale = ref[name[:-len("bias")] + "weight"] if name in one_per_group else None
        err = _rel_l2(mine[name], g64, scale)
        worst = max(worst, (err, name))
        assert err < GRAD_TOL, (what, name, err)
    print(f"MEASURED {what} worst gradient {worst[1]} {worst[0]:.2e} over {len(ref)} tensors")
    return worst


class _math:
    """`with _math(name):` fused.set_conv_math for the block (None: the environment's)"""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        from p2p_bridge_amd import fused

        self.prev = fused._conv_math_override  # (set_conv_math returns the resolved name: restoring that would pin it process-wide)
        if self.name is not None:
            fused.set_conv_math(self.name)

    def __exit__(self, *exc):
        from p2p_bridge_amd import fused

        if self.name is not None:
            fused.set_conv_math(self.prev)


_streams = {}


def _geometry(coords, sa):
    """the coordinate-only preparation of the network's geometry stream for one level: FPS + ball query, and the 3-NN lists
    of the feature propagation back to `coords`"""
    from p2p_bridge_amd.pvcnn_unet import Geometry

    if "side" not in _streams:
        _streams["side"] = torch.cuda.Stream()
    return Geometry({"voxel": [], "sa": [sa], "fp": [None]}, coords, _streams["side"])


# ------------------------------------------------------------------------------------------------- set abstraction


def _sa_forward(key, geo, math=None):
    """the module's forward on the case -> PVCData; the caller chooses train / eval and the grad mode"""
    from p2p_bridge_amd.pvcnn_unet import PVCData, temb_broadcast

    c = SA_CASES[key]
    mod, inp, _, _ = _sa_case(key)
    with _math(math):
        data = PVCData(features=inp["feats"], coords=inp["coords"], cond=inp["cond"],
                       time_emb=None if inp["te"] is None else temb_broadcast(inp["te"], c["N"]))
        if geo:
            data.geo = _geometry(inp["coords"], dict(centers=c["M"], radius=c["radius"], neighbors=c["U"]))
        data = mod(data)
        if geo:
            torch.cuda.current_stream().wait_event(data.geo.join)
        torch.cuda.synchronize()
        if geo:
            assert torch.equal(data.geo.sa[0][1], _sa_case(key)[2][1])  # (the lists the reference was given)
    return data


def _sa_check(key, data, what):
    c = SA_CASES[key]
    _, inp, _, (ref, ref_centers, ref_temb) = _sa_case(key)
    res = _check_out(data.features, ref, what)
    assert torch.equal(data.coords.cpu().double(), ref_centers), what  # (a gather: exact)
    if inp["te"] is None:
        assert data.time_emb is None
    else:
        assert data.time_emb.shape == (B, E, c["M"]) and torch.equal(data.time_emb.cpu().double(), ref_temb), what
    return res


def _sa_eval(key, geo, grad, math=None):
    mod = _sa_case(key)[0]
    mod.eval()
    with torch.set_grad_enabled(grad):
        return _sa_forward(key, geo, math)


@pytest.mark.parametrize("key", ["S1", "S2", "S2b", "S3", "S3b", "S4", "S5a", "S5b"])
def test_sa_geo_fused(key):
    """S1 - S5: eval, no_grad, geometry stream: the first layer before the grouping, in each of its forms"""
    from p2p_bridge_amd import fused

    if key == "S1" and fused.conv_math() != "f16x3":
        pytest.skip("S1 is the gather-pool form, which exists in the f16x3 arithmetic only (S8 / S9 run the shape elsewhere)")
    form = _form(key)
    _sa_check(key, _sa_eval(key, True, False), f"{key} geo fused {form}")


@pytest.mark.parametrize("math", MATHS)
def test_sa_split_layer(math):
    """S6: a 128 -> 128 layer on the split-operand GEMM inside _run_fused (the exact-fp32 kernel under fp32)"""
    with _math(math):
        form = _form("S6", math)
    _sa_check("S6", _sa_eval("S6", True, False, math), f"S6 {math} {form}")


def test_sa_geo_eval_with_grad():
    """S7: eval with autograd on: group_concat -> SharedMLP.run -> dense"""
    _form("S4")
    _sa_check("S4", _sa_eval("S4", True, True), "S7 (S4 shape) geo eval grad")


@pytest.mark.parametrize("key", ["S1", "S4"])
def test_sa_no_geo(key):
    """S8: eval, no_grad, no geometry stream: the module's own FPS + BallQuery, then _run_fused(first=None)"""
    _sa_check(key, _sa_eval(key, False, False), f"S8 ({key} shape) no geo")


def _sa_train(key, what):
    mod, inp, (fps, nidx), _ = _sa_case(key)
    from p2p_bridge_amd.pvcnn_unet import PVCData, temb_broadcast

    c = SA_CASES[key]
    mod.train()
    mod.zero_grad(set_to_none=True)
    feats = inp["feats"].detach().clone().requires_grad_(True)
    cond = None if inp["cond"] is None else inp["cond"].detach().clone().requires_grad_(True)
    try:
        data = mod(PVCData(features=feats, coords=inp["coords"], cond=cond,
                           time_emb=None if inp["te"] is None else temb_broadcast(inp["te"], c["N"])))
        data.features.backward(inp["gy"])
        torch.cuda.synchronize()
    finally:
        mod.eval()
    _sa_check(key, data, what)
    p = _params64(mod, grad=True)
    f64, c64 = _d(feats, True), _d(cond, cond is not None)
    out, _, _ = R.sa_block(f64, _d(inp["coords"]), None, c64, p, fps.cpu(), nidx.cpu(), groups=c.get("groups", 8))
    out.backward(_d(inp["gy"]))
    ref = {"features": f64.grad, **{k: v.grad for k, v in p.items()}}
    mine = {"features": feats.grad}
    if cond is not None:
        ref["cond"], mine["cond"] = c64.grad, cond.grad
    _check_grads(mod, mine, ref, what)
    mod.zero_grad(set_to_none=True)


@pytest.mark.parametrize("key", ["S1", "S4"])
def test_sa_training(key):
    """S9: train(): output and the gradients of the features, cond and every conv / norm / emd parameter"""
    _sa_train(key, f"S9 ({key} shape) training")


def test_sa_training_grouping_and_cat(monkeypatch):
    """S9 with P2PB_EXPERIMENT group_concat=0: BallQuery's two groupings, subtraction and concatenation"""
    from p2p_bridge_amd import _experiment

    monkeypatch.setenv("P2PB_EXPERIMENT", _experiment.setting(group_concat=0))
    _sa_train("S4", "S9 (S4 shape) training group_concat=0")


@pytest.mark.parametrize("path", ["geo-fused", "geo-grad", "nogeo", "train"])
def test_sa_xyz_only(path):
    """S10: data.features is None -- the grouped tensor is the relative coordinates alone on every path, as BallQuery.forward
    has it (the geo branch dereferenced None before this test)"""
    from p2p_bridge_amd.pvcnn_unet import PVCData

    if path == "geo-fused":
        form = _form("S10")
        _sa_check("S10", _sa_eval("S10", True, False), f"S10 geo fused {form}")
    elif path == "geo-grad":
        _sa_check("S10", _sa_eval("S10", True, True), "S10 geo eval grad")
    elif path == "nogeo":
        _sa_check("S10", _sa_eval("S10", False, False), "S10 no geo")
    else:
        mod, inp, _, _ = _sa_case("S10")
        mod.train()
        try:
            data = mod(PVCData(features=None, coords=inp["coords"]))
            torch.cuda.synchronize()
        finally:
            mod.eval()
        _sa_check("S10", data, "S10 training forward")


# ------------------------------------------------------------------------------------------------- feature propagation


def _fp_forward(key, geo, folded, grad_inputs=False):
    """folded: lower_temb carries the time embedding (the fused network's form); otherwise it is concatenated into
    lower_features as PVCNN2Unet.forward's fallback and the reference do. -> (PVCData, lower_features, skip) as handed over"""
    from p2p_bridge_amd.pvcnn_unet import PVCData, temb_broadcast

    c = FP_CASES[key]
    mod, inp, (lower, idx3), _ = _fp_case(key)
    te = inp["te"]
    g = inp["g"] if (folded or te is None) else torch.cat([inp["g"], te[:, :, None].expand(-1, -1, c["M"])], dim=1)
    skip, cond = inp["skip"], inp["cond"]
    if grad_inputs:
        g = g.detach().clone().requires_grad_(True)
        skip = None if skip is None else skip.detach().clone().requires_grad_(True)
        cond = None if cond is None else cond.detach().clone().requires_grad_(True)
    data = PVCData(features=skip, coords=inp["coords"], lower_coords=lower, lower_features=g, cond=cond,
                   time_emb=None if te is None else temb_broadcast(te, c["M"]), lower_temb=te if folded else None)
    if geo:
        data.geo = _geometry(inp["coords"], dict(centers=c["M"], radius=0.5, neighbors=4))
    data = mod(data)
    if geo:
        torch.cuda.current_stream().wait_event(data.geo.join)
    torch.cuda.synchronize()
    if geo:  # (the coarse level and the lists the reference was given)
        assert torch.equal(data.geo.sa[0][0], lower) and torch.equal(data.geo.fp[0][0], idx3)
    return data, g, skip, cond


def _fp_check(key, data, what):
    c = FP_CASES[key]
    _, inp, _, ref = _fp_case(key)
    res = _check_out(data.features, ref, what)
    if inp["te"] is None:
        assert data.time_emb is None
    else:  # (the time embedding comes back broadcast over the N fine points)
        assert torch.equal(data.time_emb, inp["te"][:, :, None].expand(-1, -1, c["N"])), what
    return res


def _fp_eval(key, geo, folded, grad):
    mod = _fp_case(key)[0]
    mod.eval()
    with torch.set_grad_enabled(grad):
        return _fp_forward(key, geo, folded)[0]


@pytest.mark.parametrize("key", ["F1", "F2a", "F2b", "F3", "F4", "F5"])
def test_fp_geo_fused(key):
    """F1 - F5: eval, no_grad, geometry stream: the first layer before the interpolation, the time embedding as a bias"""
    form = _form(key)
    _fp_check(key, _fp_eval(key, True, True, False), f"{key} geo fused {form}")


@pytest.mark.parametrize("key", ["F6", "F1"])
def test_fp_geo_fused_concatenated_temb(key):
    """F6: the time embedding concatenated into lower_features, lower_temb None (Cg = 30: what the network does when a
    channel count is no multiple of 4) -- and the F1 case in that form, held to the SAME reference tensor as F1's folded form:
    the two forms compute the same function"""
    _form(key)
    _fp_check(key, _fp_eval(key, True, False, False), f"F6 ({key} case) geo fused, temb concatenated")


def test_fp_geo_eval_with_grad():
    """F7: eval with autograd on: three_interpolate + cat + SharedMLP.run -> dense"""
    _fp_check("F3", _fp_eval("F3", True, False, True), "F7 (F3 shape) geo eval grad")


@pytest.mark.parametrize("key", ["F1", "F3"])
def test_fp_no_geo(key):
    """F8: eval, no_grad, no geometry stream: nearest_neighbor_interpolate, then the fused SharedMLP"""
    _fp_check(key, _fp_eval(key, False, False, False), f"F8 ({key} shape) no geo")


@pytest.mark.parametrize("key", ["F1", "F3"])
def test_fp_training(key):
    """F8: train(): output and the gradients of lower_features, the skip features, cond and every parameter"""
    c = FP_CASES[key]
    mod, inp, (lower, idx3), _ = _fp_case(key)
    what = f"F8 ({key} shape) training"
    mod.train()
    mod.zero_grad(set_to_none=True)
    try:
        data, g, skip, cond = _fp_forward(key, False, False, grad_inputs=True)
        data.features.backward(inp["gy"])
        torch.cuda.synchronize()
    finally:
        mod.eval()
    _fp_check(key, data, what)
    p = _params64(mod, grad=True)
    g64, s64, c64 = _d(g, True), _d(skip, True), _d(cond, True)
    out = R.fp_block(_d(inp["coords"]), s64, _d(lower), g64, None, c64, p, idx3.cpu())
    out.backward(_d(inp["gy"]))
    ref = {"lower_features": g64.grad, "skip": s64.grad, "cond": c64.grad, **{k: v.grad for k, v in p.items()}}
    _check_grads(mod, {"lower_features": g.grad, "skip": skip.grad, "cond": cond.grad}, ref, what)
    mod.zero_grad(set_to_none=True)


# ------------------------------------------------------------------------------------------------- Pnet2Stage


def _pnet_check(key, what, train=False):
    mod, inp, ref = _pnet_case(key)
    fusable = mod._fusable()
    assert fusable == (key in ("P1", "P2")), key
    form = _form(key)
    assert form["pool"] == (key != "P2"), (key, form)
    if not train:
        mod.eval()
        with torch.no_grad():
            out = mod(inp["coords"])
        torch.cuda.synchronize()
        return _check_out(out, ref, f"{what} fusable={fusable} {form}")
    mod.train()
    mod.zero_grad(set_to_none=True)
    coords = inp["coords"].detach().clone().requires_grad_(True)
    try:
        out = mod(coords)
        out.backward(inp["gy"])
        torch.cuda.synchronize()
    finally:
        mod.eval()
    _check_out(out, ref, what)
    p = _params64(mod, grad=True)
    c64 = _d(coords, True)
    R.pnet2_stage(c64, p).backward(_d(inp["gy"]))
    _check_grads(mod, {"coords": coords.grad}, {"coords": c64.grad, **{k: v.grad for k, v in p.items()}}, what)
    mod.zero_grad(set_to_none=True)


@pytest.mark.parametrize("key", ["P1", "P2", "P3", "P4"])
def test_pnet2_stage_eval(key):
    """P1 / P2: the fused form with pooled epilogues / with affine_act_max; P3 / P4: the forms _fusable() refuses, on dense"""
    _pnet_check(key, f"{key} eval")


@pytest.mark.parametrize("key", ["P1", "P3"])
def test_pnet2_stage_training(key):
    """P5 (the P1 shape) and P3: train(): output, every parameter's gradient and the coordinates'"""
    _pnet_check(key, f"{'P5' if key == 'P1' else key} ({key} shape) training", train=True)
