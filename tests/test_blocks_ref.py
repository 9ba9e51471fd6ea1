"""tests/blocks_ref.py (the float64 restatement test_sa_fp_blocks_gpu.py holds the HIP blocks to) against the CPU oracle
network's blocks, oracle/net_ref.py RefNet._sa_module / _fp_module / _global_pnet -- fp32 on the CPU, bit-equal to the imported
reference through the committed goldens. Same weights, and the index lists the oracle itself produced (its op_log). No GPU.

Gate: 1e-5 of max|ref| -- the fp32 rounding of a two- or three-layer chain of (1x1 conv, GroupNorm, Swish) at unit scale
(the float64 side contributes nothing at that level). Measured: set abstraction 2.7e-7, feature propagation 3.3e-7, Pnet2Stage 7.0e-7."""
import json
import os

import pytest
import torch

import blocks_ref as R

GATE = 1e-5
E = 16


def _refnet(sd, log):
    from oracle import net_ref

    cfg = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_cfg.json")))
    return net_ref.RefNet(cfg, sd, op_log=log)


def _cloud(B, N, gen):
    p = torch.randn(B, 3, N, generator=gen, dtype=torch.float64)
    return (p / p.norm(dim=1, keepdim=True) + 0.01 * torch.randn(B, 3, N, generator=gen, dtype=torch.float64)).float()


def _mlp_params(pre, widths, cin, dim, cond, gen):
    """SharedMLP parameters under `pre` with the reference's names; random affine norm parameters"""
    p = {}
    for i, co in enumerate(widths):
        p[f"{pre}.layers.{3 * i}.weight"] = torch.randn(co, cin, *([1] * dim), generator=gen) / cin ** 0.5
        p[f"{pre}.layers.{3 * i}.bias"] = 0.1 * torch.randn(co, generator=gen)
        n = f"{pre}.layers.{3 * i + 1}"
        gn = n + ".norm" if cond else n
        p[gn + ".weight"] = 1 + 0.3 * torch.randn(co, generator=gen)
        p[gn + ".bias"] = 0.3 * torch.randn(co, generator=gen)
        if cond:
            p[n + ".emd.weight"] = 0.3 * torch.randn(2 * co, E, generator=gen)
            p[n + ".emd.bias"] = torch.cat([torch.ones(co), torch.zeros(co)]) + 0.1 * torch.randn(2 * co, generator=gen)
        cin = co
    return p


def _d(t):
    return None if t is None else t.double()


def _err(out, ref):
    return ((out - ref.double()).abs().max() / ref.abs().max()).item()


@pytest.mark.parametrize("cond", [True, False], ids=["adagn", "gn"])
def test_sa_block_vs_oracle(cond):
    gen = torch.Generator().manual_seed(11)
    B, N, M, C = 2, 256, 64, 13
    coords, feats = _cloud(B, N, gen), torch.randn(B, C, N, generator=gen)
    temb = torch.randn(B, E, generator=gen)[:, :, None].expand(-1, -1, N)
    cd = torch.randn(B, E, generator=gen) if cond else None
    p = _mlp_params("mlps.0", [24, 40], C + 3, 2, cond, gen)
    log = []
    net = _refnet({"sa." + k: v for k, v in p.items()}, log)
    ref, ref_centers, ref_temb = net._sa_module(feats, coords, temb, cd, dict(centers=M, radius=0.3, sa="sa", nmlp=2))
    fps = next(o for n, _, o in log if n == "fps")[0]
    nidx = next(o for n, _, o in log if n == "ball")[0]
    assert nidx.shape == (B, M, 32)
    out, centers, t = R.sa_block(_d(feats), _d(coords), _d(temb), _d(cd), {k: v.double() for k, v in p.items()}, fps, nidx)
    assert torch.equal(centers.float(), ref_centers) and torch.equal(t.float(), ref_temb)
    err = _err(out, ref)
    print(f"MEASURED sa_block vs oracle {err:.2e}")
    assert out.shape == ref.shape == (B, 40, M) and err < GATE, err


def test_sa_block_xyz_only_vs_restated_grouping():
    """features = None: the grouped tensor is the relative coordinates alone (BallQuery.forward, models/pvcnn.py:119-121);
    the oracle's _sa_module always groups features, so the comparison is with its pieces: grouping, subtraction, MLP, max"""
    from oracle import cpu_ops as ops

    gen = torch.Generator().manual_seed(12)
    B, N, M = 2, 256, 64
    coords = _cloud(B, N, gen)
    p = _mlp_params("mlps.0", [24, 40], 3, 2, False, gen)
    net = _refnet({"sa." + k: v for k, v in p.items()}, None)
    fps = ops.furthest_point_sampling_forward(coords, M)
    centers = ops.gather_features_forward(coords, fps)
    nidx = ops.ball_query(centers, coords, 0.3, 16)
    rel = ops.grouping_forward(coords, nidx) - centers.unsqueeze(-1)
    ref = net._shared_mlp(rel, None, "sa.mlps.0", 2).max(dim=-1).values
    out, _, t = R.sa_block(None, _d(coords), None, None, {k: v.double() for k, v in p.items()}, fps, nidx)
    assert t is None and _err(out, ref) < GATE


@pytest.mark.parametrize("skip", [True, False], ids=["skip", "noskip"])
def test_fp_block_vs_oracle(skip):
    gen = torch.Generator().manual_seed(13)
    B, N, M, Cg, Cs = 2, 256, 64, 32, 19
    coords = _cloud(B, N, gen)
    lower = coords[:, :, torch.randperm(N, generator=gen)[:M]].contiguous()  # (a coarse level is a subset of the fine one)
    g, te = torch.randn(B, Cg, M, generator=gen), torch.randn(B, E, generator=gen)
    sk = torch.randn(B, Cs, N, generator=gen) if skip else None
    cd = torch.randn(B, E, generator=gen)
    p = _mlp_params("mlp", [40, 24], Cg + E + (Cs if skip else 0), 1, True, gen)
    log = []
    net = _refnet({"fp." + k: v for k, v in p.items()}, log)
    lower_feats = torch.cat([g, te[:, :, None].expand(-1, -1, M)], dim=1)
    ref, _ = net._fp_module(coords, sk, lower, lower_feats, None, cd, dict(fp="fp", nmlp=2))
    _, idx3, w3 = next(o for n, _, o in log if n == "3nn")
    assert (R.three_nn_weights(coords, lower, idx3) - w3.double()).abs().max().item() < 1e-6  # (the oracle's fp32 weights)
    out = R.fp_block(coords, _d(sk), lower, _d(g), _d(te), _d(cd), {k: v.double() for k, v in p.items()}, idx3)
    err = _err(out, ref)
    print(f"MEASURED fp_block vs oracle {err:.2e}")
    assert out.shape == ref.shape == (B, 24, N) and err < GATE, err


def test_gpu_cases_meet_their_input_conditions_on_the_cpu():
    """the cases of test_sa_fp_blocks_gpu.py, built here with the oracle's FPS / ball query and the restatement alone: every
    set-abstraction case has padded AND full neighbour lists (sa_decisions asserts it) and, like every Pnet2Stage case, at least
    MIN_SHARE of its pooled rows take their value from the row minimum; no Pnet2Stage winner sits at Swish's zero crossing"""
    import test_sa_fp_blocks_gpu as T
    from oracle import cpu_ops as ops

    for key, c in T.SA_CASES.items():
        mod, inp = T.sa_setup(key, "cpu")
        fps, nidx, padded = T.sa_decisions(inp["coords"], c, ops)
        keep = {}
        with torch.no_grad():
            R.sa_block(_d(inp["feats"]), _d(inp["coords"]), None, _d(inp["cond"]), T._params64(mod), fps, nidx,
                       groups=c.get("groups", 8), keep=keep)
        share = R.min_share(keep["pre_act"])
        print(f"MEASURED {key} padded {padded:.2f} full {1 - padded:.2f} min share {share:.2f}")
        assert share >= T.MIN_SHARE, (key, share)
    for key in T.PNET_CASES:
        mod, inp = T.pnet_setup(key, "cpu")
        keep = {}
        with torch.no_grad():
            R.pnet2_stage(_d(inp["coords"]), T._params64(mod), keep)
        assert min(R.min_share(v) for v in keep.values()) >= T.MIN_SHARE, key
        assert T.pnet_winners(mod, inp["coords"]).abs().min().item() >= T.PNET_MIN_WINNER, key


def _pnet_params(mlp1, mlp2, gen):
    p = {}
    for name, ch in (("mlp1", mlp1), ("mlp2", [2 * mlp1[-1]] + mlp2)):
        blocks = ["shared_mlp_0", "shared_mlp_1"] + [f"last_mlp_layers.{i}" for i in range(len(ch) - 3)]
        for blk, ci, co in zip(blocks, ch[:-1], ch[1:]):
            p[f"{name}.{blk}.mlp.0.weight"] = torch.randn(co, ci, 1, 1, generator=gen) / ci ** 0.5
            p[f"{name}.{blk}.mlp.0.bias"] = 0.1 * torch.randn(co, generator=gen)
            p[f"{name}.{blk}.mlp.1.group_norm.weight"] = 1 + 0.3 * torch.randn(co - co % 32, generator=gen)
            p[f"{name}.{blk}.mlp.1.group_norm.bias"] = 0.3 * torch.randn(co - co % 32, generator=gen)
    return p


@pytest.mark.parametrize("mlp1,mlp2", [([3, 32, 64], [128, 256]), ([3, 40, 72], [72, 96])], ids=["full-groups", "remainders"])
def test_pnet2_stage_vs_oracle(mlp1, mlp2):
    """the second case: widths 40 and 72 (MyGroupNorm normalises 32 and 64 channels and passes the other 8 through)"""
    gen = torch.Generator().manual_seed(14)
    coords = _cloud(2, 301, gen)
    p = _pnet_params(mlp1, mlp2, gen)
    ref = _refnet({"global_pnet." + k: v for k, v in p.items()}, None)._global_pnet(coords)
    out = R.pnet2_stage(coords.double(), {k: v.double() for k, v in p.items()})
    err = _err(out, ref)
    print(f"MEASURED pnet2_stage vs oracle {err:.2e}")
    assert out.shape == ref.shape == (2, mlp2[-1]) and err < GATE, err
