"""Product network + bridge sampler on the GPU vs the CPU oracle (vox_mode='tree': the build's
deterministic voxel normalisation on both sides) and vs the golden vectors captured from the
reference's own model. fp32 tolerance 1e-4 on predicted xyz / Chamfer-L2 (BASELINE.json north_star)."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import cpu_ops, net_ref

pytestmark = pytest.mark.gpu
TOL = 1e-4


def chamfer_l2(a, b):
    """CD-L2 (metrics/metrics.py:77-78 convention) between [B,3,N] clouds, on the oracle"""
    a, b = a.transpose(1, 2).contiguous(), b.transpose(1, 2).contiguous()
    B, N, _ = a.shape
    d1, d2 = torch.zeros(B, N), torch.zeros(B, N)
    i1, i2 = torch.zeros(B, N, dtype=torch.int32), torch.zeros(B, N, dtype=torch.int32)
    cpu_ops.chamfer_forward(a, b, d1, d2, i1, i2)
    return (d1.mean(1) + d2.mean(1)).max().item()


@pytest.fixture(scope="module")
def tiny():
    cfg = json.load(open(os.path.join(GOLDEN, "tiny_cfg.json")))
    w = np.load(os.path.join(GOLDEN, "tiny_weights.npz"))
    sd = {k: torch.from_numpy(w[k]).float() for k in w.files}
    return cfg, sd, np.load(os.path.join(GOLDEN, "tiny_run.npz"))


def test_tiny_net_forward(tiny):
    from p2p_bridge_amd import p2pb as product

    cfg, sd, run = tiny
    model = product.build_model(cfg, sd, device="cuda")
    model.eval()
    x, t = torch.from_numpy(run["x_start"]), torch.from_numpy(run["t"])
    with torch.no_grad():
        out = model.model(x.cuda(), t.cuda()).cpu()
        ref = net_ref.RefNet(cfg, sd, vox_mode="tree")(x, t)
    assert (out - ref).abs().max().item() < TOL
    assert np.abs(out.numpy() - run["net_out"]).max() < TOL  # the reference's own output


def chain_parity(model, orc, x, chain, T):
    """max |eps_hip - eps_oracle| over the network evaluations of a GIVEN chain of states x_t: both sides see
    identical inputs at every step ("teacher forcing"), so one flipped index decision cannot snowball."""
    _, table = model.step_tables(T)
    states = [x] + [chain[:, i] for i in range(T - 1, 0, -1)]  # x_t entering evaluation 0..T-1
    worst = 0.0
    model.eval()
    with torch.no_grad():
        for i, xt in enumerate(states):
            t = table[i, 0].expand(x.shape[0])
            worst = max(worst, (model.model(xt.cuda(), t).cpu() - orc(xt.cpu(), t.cpu())).abs().max().item())
    model.train()
    return worst


def check_sampler(model, orc, cfg, x, T, graph=False):
    """Parity contract for the T-step bridge sampler (DESIGN.md "parity"):
      1. along the ORACLE's chain and along the HIP chain, every network evaluation agrees to 1e-4;
      2. the free-running chains agree to 1e-4 while no index decision has flipped (checked at 2 steps).
    FPS / voxel rounding / ball query are discontinuous in x_t: after enough steps fp32 noise (~1e-6 per
    evaluation, dense-layer summation order) flips one of them and the two chains follow different, equally
    valid, centre sets -- with random (untrained, non-contractive) weights they then separate. The reference's
    own float-atomic voxelisation makes its CUDA runs diverge from each other the same way."""
    ref = net_ref.sample(orc, cfg, x, steps=T, log_count=T)
    assert chain_parity(model, orc, x, ref["x_chain"], T) < TOL
    out = model.sample(x_start=x.cuda(), steps=T, log_count=T, verbose=False, graph=graph)
    assert out["x_pred"].shape == ref["x_pred"].shape and out["x_chain"].shape == ref["x_chain"].shape
    assert chain_parity(model, orc, x, out["x_chain"].cpu(), T) < TOL
    for k in (1, 2):
        a = model.sample(x_start=x.cuda(), steps=k, log_count=k, verbose=False, graph=graph)["x_pred"].cpu()
        b = net_ref.sample(orc, cfg, x, steps=k, log_count=k)["x_pred"]
        assert (a - b).abs().max().item() < TOL, k
        assert chamfer_l2(a, b) < TOL
    return out, ref


@pytest.mark.parametrize("graph", [False, True])
def test_tiny_sampler(tiny, graph):
    from p2p_bridge_amd import p2pb as product

    cfg, sd, run = tiny
    model = product.build_model(cfg, sd, device="cuda")
    x = torch.from_numpy(run["x_start"])
    orc = net_ref.RefNet(cfg, sd, vox_mode="tree")
    out, ref = check_sampler(model, orc, cfg, x, 5, graph)
    assert model.model.training  # ddpm_sampling flips back to train() (models/p2pb.py:333)
    # golden (the reference's own sampler output): same function at the golden chain's states
    assert chain_parity(model, orc, x, torch.from_numpy(run["x_chain_T5"]), 5) < TOL
    if graph:  # replay determinism
        pred = out["x_pred"].cpu()
        again = model.sample(x_start=x.cuda(), steps=5, log_count=5, verbose=False, graph=True)["x_pred"].cpu()
        assert torch.equal(again, pred), f"replay differs: max {(again - pred).abs().max().item():.3e}, " \
                                         f"{(again != pred).sum().item()} of {pred.numel()} values"


def test_stock_pvds_config1():
    """BASELINE config 1: stock PVDS_PUNet, one 1024-point patch, 5 steps; seeded weights shared by both
    sides; parity contract of check_sampler."""
    from test_host_logic import PVDS
    from p2p_bridge_amd import p2pb as product
    from p2p_bridge_amd.pvcnn_unet import PVCNN2Unet

    torch.manual_seed(0)
    sd = {k: v.clone() for k, v in PVCNN2Unet(PVDS).state_dict().items()}
    x, _ = net_ref.synthetic_patches(1, 1024, seed=0)
    model = product.build_model(PVDS, sd, device="cuda")
    orc = net_ref.RefNet(PVDS, sd, vox_mode="tree")
    check_sampler(model, orc, PVDS, x, 5)


def test_pvdl_like_topology(tiny):
    """A PVDL-shaped network (extra input features, two PVConvs in SA stage 0, 2/2/3/2 feature-propagation blocks:
    models/pvcnn.py:615-618,78-95), tiny channel widths, seeded weights shared by both sides: the fused inference path
    (first-layer-before-grouping / -interpolation, shared voxel sorts per level, ...) vs the oracle network."""
    import copy

    from p2p_bridge_amd import p2pb as product
    from p2p_bridge_amd.pvcnn_unet import PVCNN2Unet

    cfg = copy.deepcopy(tiny[0])
    cfg["model"]["extra_feature_channels"] = 3
    cfg["model"]["PVD"]["n_sa_blocks"] = [2, 1, 1, 1]
    cfg["model"]["PVD"]["n_fp_blocks"] = [2, 2, 3, 2]
    cfg["gpu"] = "cpu"
    torch.manual_seed(0)
    sd = {k: v.clone() for k, v in PVCNN2Unet(cfg).state_dict().items()}
    torch.manual_seed(1)
    xyz, _ = net_ref.synthetic_patches(2, 1024, seed=3)
    x = torch.cat([xyz, torch.rand(2, 3, 1024)], dim=1)  # xyz + RGB-like features
    t = torch.tensor([10.0, 500.0])
    model = product.build_model(cfg, sd, device="cuda")
    model.eval()
    orc = net_ref.RefNet(cfg, sd, vox_mode="tree")
    with torch.no_grad():
        out = model.model(x.cuda(), t.cuda()).cpu()
        ref = orc(x, t)
    assert out.shape == ref.shape == (2, 3, 1024)
    assert (out - ref).abs().max().item() < TOL
    # the unfused (training-mode layers, autograd ops) path of the same module agrees as well
    model.model.train()
    out_train = model.model(x.cuda(), t.cuda()).detach().cpu()
    assert (out_train - ref).abs().max().item() < TOL


@pytest.mark.parametrize("vres", [[32, 16, 8, 4], [12, 6, 6, 2], [64, 32, 16, 8]], ids=lambda v: "r" + "-".join(map(str, v)))
def test_voxel_resolutions(tiny, vres):
    """The tiny network (8..128 channels) at other voxel resolutions, seeded weights shared by both sides, fused inference and
    training-mode forward vs the oracle. [32, 16, 8, 4]: the compact r = 16 and brick-list sparse r = 32 convolutions at narrow
    channel counts, through the geometry stream and the pre-split operands; [12, 6, 6, 2]: resolutions outside {4, 8, 16, 32}
    (PVConv's dense fallback, whose SE gate the fused point branch used to drop); [64, 32, 16, 8]: r = 64 (the reference's
    voxel_resolution_multiplier = 2 on PVDS), where the geometry stream used to ask for brick lists it has none for."""
    import copy

    from p2p_bridge_amd import p2pb as product
    from p2p_bridge_amd.pvcnn_unet import PVCNN2Unet

    cfg = copy.deepcopy(tiny[0])
    cfg["model"]["PVD"]["voxel_resolutions"] = list(vres)
    cfg["gpu"] = "cpu"
    torch.manual_seed(0)
    sd = {k: v.clone() for k, v in PVCNN2Unet(cfg).state_dict().items()}
    x, _ = net_ref.synthetic_patches(2, 1024, seed=3)
    t = torch.tensor([10.0, 500.0])
    model = product.build_model(cfg, sd, device="cuda")
    model.eval()
    orc = net_ref.RefNet(cfg, sd, vox_mode="tree")
    with torch.no_grad():
        out = model.model(x.cuda(), t.cuda()).cpu()
        ref = orc(x, t)
    assert out.shape == ref.shape == (2, 3, 1024)
    assert (out - ref).abs().max().item() < TOL
    model.model.train()
    out_train = model.model(x.cuda(), t.cuda()).detach().cpu()
    assert (out_train - ref).abs().max().item() < TOL


def test_odd_point_counts(tiny):
    """N = 1000 (centres 250 / 62 / 15 / 3): rows that are not 16-byte multiples take the fallback paths of the fused
    kernels (one-position-per-lane GEMM, two-pass pooling, channel-major gathers) -- same contract."""
    import copy

    from p2p_bridge_amd import p2pb as product

    cfg, sd, _ = tiny
    cfg = copy.deepcopy(cfg)
    cfg["data"]["npoints"] = 1000
    x, _ = net_ref.synthetic_patches(2, 1000, seed=5)
    t = torch.tensor([3.0, 700.0])
    model = product.build_model(cfg, sd, device="cuda")
    model.eval()
    orc = net_ref.RefNet(cfg, sd, vox_mode="tree")
    with torch.no_grad():
        out = model.model(x.cuda(), t.cuda()).cpu()
        ref = orc(x, t)
    assert out.shape == ref.shape == (2, 3, 1000)
    assert (out - ref).abs().max().item() < TOL


def test_large_cloud(tiny):
    """one 20000-point cloud (BASELINE configs 4/5 feed 50000-point room patches): the global-memory FPS variant
    (n > 16384), long rows in every kernel, stock radii -- network output vs the oracle"""
    import copy

    from p2p_bridge_amd import p2pb as product

    cfg, sd, _ = tiny
    cfg = copy.deepcopy(cfg)
    cfg["data"]["npoints"] = 20000
    x, _ = net_ref.synthetic_patches(1, 20000, seed=7)
    t = torch.tensor([250.0])
    model = product.build_model(cfg, sd, device="cuda")
    model.eval()
    orc = net_ref.RefNet(cfg, sd, vox_mode="tree")
    with torch.no_grad():
        out = model.model(x.cuda(), t.cuda()).cpu()
        ref = orc(x, t)
    assert out.shape == ref.shape == (1, 3, 20000)
    assert (out - ref).abs().max().item() < TOL


def test_training_step_grads(tiny):
    """forward+backward of the bridge loss on the GPU (HIP grad kernels) vs the golden loss/gradients
    the reference produced on CPU for the same fixed steps."""
    from p2p_bridge_amd import p2pb as product

    cfg, sd, run = tiny
    model = product.build_model(cfg, sd, device="cuda")
    model.train()
    steps = torch.from_numpy(run["loss_steps"])
    _randint = torch.randint
    torch.randint = lambda *a, **k: steps.clone()
    try:
        loss = model(torch.from_numpy(run["clean"]).cuda(), torch.from_numpy(run["x_start"]).cuda())
    finally:
        torch.randint = _randint
    loss.backward()
    assert abs(loss.item() - float(run["loss"])) <= 1e-4 * abs(float(run["loss"]))
    norms = json.load(open(os.path.join(GOLDEN, "tiny_gradnorms.json")))
    params = dict(model.model.named_parameters())
    bad = [(k, params[k].grad.norm().item(), v) for k, v in norms.items()
           if abs(params[k].grad.norm().item() - v) > 2e-3 * max(v, 1e-3)]
    assert not bad, bad[:5]
    for k in ("classifier.2.weight", "embedf.0.weight"):
        g, exp = params[k].grad.cpu().numpy(), run["grad_" + k]
        assert np.abs(g - exp).max() <= 1e-3 * max(1.0, np.abs(exp).max()), k


def test_full_size_pvdl_fused_vs_unfused():
    """PVDL at its real size (channels 64..1024, 13 PVConvs, 384 extra feature channels, 118.7 M parameters; BASELINE
    configs 4-5): the fused inference path (compact / sparse convolutions, split-operand GEMMs, folded norms) against
    the unfused autograd path of the same module on the same HIP ops -- one evaluation, B=2, N=4096"""
    import copy

    from p2p_bridge_amd import p2pb as product
    from p2p_bridge_amd.synthetic import synthetic_patches
    from test_host_logic import pvdl_cfg

    cfg = copy.deepcopy(pvdl_cfg())
    torch.manual_seed(0)
    model = product.build_model(cfg, device="cuda")
    assert abs(sum(p.numel() for p in model.model.parameters()) / 1e6 - 118.67) < 0.01
    x, _ = synthetic_patches(2, 4096, seed=1)
    xin = torch.cat([x, torch.randn(2, 384, 4096)], 1).cuda()
    t = torch.tensor([500.0, 20.0], device="cuda")
    model.model.eval()
    with torch.no_grad():
        y_fused = model.model(xin, t)
    with torch.enable_grad():
        y_ref = model.model(xin, t).detach()
    assert torch.isfinite(y_fused).all()
    assert (y_fused - y_ref).abs().max().item() < TOL
