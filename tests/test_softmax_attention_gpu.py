"""`attention_type: flash` / `none` on the GPU: the HIP softmax-attention core (csrc/attention.hip) against the fp64
restatement of tests/test_attention_types.py (which that file ties to the reference's own module), the `Attention` module
and the whole tiny network against what the reference computed (tests/golden/tiny_flash.npz, tiny_noattn.npz;
tools/make_golden_attention.py)."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import net_ref
from test_attention_types import attention64, core64, flash_record, tiny_cfg

pytestmark = pytest.mark.gpu
TOL = 1e-4  # the project's parity budget


def _weights(extra=None):
    w = np.load(os.path.join(GOLDEN, "tiny_weights.npz"))
    sd = {k: torch.from_numpy(w[k]).float() for k in w.files if not k.startswith("global_att.")}
    return {**sd, **(extra or {})}


@pytest.fixture(scope="module")
def flash():
    g, w = flash_record()
    return tiny_cfg("flash"), _weights(w), g


@pytest.mark.parametrize("b,heads,n", [(2, 4, 32), (3, 12, 195), (1, 4, 8), (2, 4, 1000), (1, 4, 1), (1, 4, 4096)])
def test_softmax_attention_core_fwd_bwd(b, heads, n):
    """forward and backward vs fp64, at the gates the linear core is held to (tests/test_sampler_features_gpu.py:170-172):
    forward 1e-5, gradients 2e-5, times max(1, |ref|max). fp32 torch (einsum + softmax) sits at <= 1.4e-6 / 2.1e-6 from
    fp64 on these inputs. Two backward passes on the same inputs give the same bits (no atomics)."""
    from p2p_bridge_amd.pvcnn_unet import _SoftmaxAttentionCore

    torch.manual_seed(b * 100 + n)
    q = (torch.randn(b, heads * 32, n, device="cuda") * 2).requires_grad_(True)
    kv = (torch.randn(b, 2 * heads * 32, n, device="cuda") * 2).requires_grad_(True)
    out = _SoftmaxAttentionCore.apply(q, kv, heads)
    gy = torch.randn_like(out)
    gq, gkv = torch.autograd.grad(out, (q, kv), gy, retain_graph=True)
    gq2, gkv2 = torch.autograd.grad(out, (q, kv), gy)
    q64 = q.detach().double().cpu().requires_grad_(True)
    kv64 = kv.detach().double().cpu().requires_grad_(True)
    ref = core64(q64, kv64, heads)
    rq, rkv = torch.autograd.grad(ref, (q64, kv64), gy.double().cpu())
    ref = ref.detach()
    e_out = (out.detach().cpu().double() - ref).abs().max().item()
    e_q, e_kv = (gq.cpu().double() - rq).abs().max().item(), (gkv.cpu().double() - rkv).abs().max().item()
    print(f"\n(b, heads, n) = {(b, heads, n)}: forward {e_out:.2e} (|ref| {ref.abs().max().item():.2f}), dq {e_q:.2e} "
          f"(|ref| {rq.abs().max().item():.2f}), dkv {e_kv:.2e} (|ref| {rkv.abs().max().item():.2f})")
    assert e_out < 1e-5 * max(1.0, ref.abs().max().item())
    assert e_q < 2e-5 * max(1.0, rq.abs().max().item())
    assert e_kv < 2e-5 * max(1.0, rkv.abs().max().item())
    assert torch.equal(gq, gq2) and torch.equal(gkv, gkv2)
    with torch.no_grad():  # the inference form (no log-sum-exp output) computes the same bits
        assert torch.equal(_SoftmaxAttentionCore.apply(q.detach(), kv.detach(), heads), out.detach())
    if n == 1:  # a single token attends to itself: out = v exactly
        assert torch.equal(out.detach(), kv.detach()[:, heads * 32:])


def test_softmax_attention_core_preconditions():
    """raw pointers go to the kernels: host tensors, non-fp32 tensors, a head width other than 32 and operands that do not
    fit each other are refused -- no fault, no reinterpreted halves"""
    from p2p_bridge_amd.pvcnn_unet import _SoftmaxAttentionCore

    q, kv = torch.randn(1, 128, 16, device="cuda"), torch.randn(1, 256, 16, device="cuda")
    with pytest.raises(RuntimeError, match="CUDA"):
        _SoftmaxAttentionCore.apply(q.cpu(), kv, 4)
    with pytest.raises(RuntimeError, match="CUDA"):
        _SoftmaxAttentionCore.apply(q, kv.cpu(), 4)
    with pytest.raises(RuntimeError, match="float"):
        _SoftmaxAttentionCore.apply(q.half(), kv.half(), 4)
    with pytest.raises(RuntimeError, match="float"):
        _SoftmaxAttentionCore.apply(q, kv.double(), 4)
    with pytest.raises(RuntimeError):  # dim_head = 64: P2PB_EINVAL from the library
        _SoftmaxAttentionCore.apply(q, kv, 2)
    with pytest.raises(RuntimeError):  # dim_head = 16
        _SoftmaxAttentionCore.apply(q, kv, 8)
    with pytest.raises(RuntimeError):  # kv of another length
        _SoftmaxAttentionCore.apply(q, kv[:, :, :8], 4)
    with pytest.raises(RuntimeError):
        _SoftmaxAttentionCore.apply(q, kv[:, :128], 4)
    torch.cuda.synchronize()
    assert torch.isfinite(_SoftmaxAttentionCore.apply(q, kv, 4)).all()


def _module(g, w):
    from p2p_bridge_amd.pvcnn_unet import Attention

    att = Attention(g["mod.x"].shape[1], heads=int(g["mod.heads"]))
    att.load_state_dict({k[len("global_att."):]: v for k, v in w.items()}, strict=True)
    return att.cuda()


def test_attention_module_vs_reference():
    """the module-level record: fused (eval, no_grad) and autograd outputs and the input gradient vs the reference's"""
    g, w = flash_record()
    att = _module(g, w)
    x = torch.from_numpy(g["mod.x"]).cuda().requires_grad_(True)
    y = att(x)
    assert y.shape == x.shape
    (gx,) = torch.autograd.grad(y, x, torch.from_numpy(g["mod.gy"]).cuda())
    att.eval()
    with torch.no_grad():
        y_fused = att(x.detach())
    e_t, e_f = np.abs(y.detach().cpu().numpy() - g["mod.y"]).max(), np.abs(y_fused.cpu().numpy() - g["mod.y"]).max()
    e_g = np.abs(gx.cpu().numpy() - g["mod.gx"]).max()
    e_tf = (y.detach() - y_fused).abs().max().item()
    print(f"\nmodule: autograd {e_t:.2e}, fused {e_f:.2e} (|y| {np.abs(g['mod.y']).max():.2f}); dx {e_g:.2e} "
          f"(|dx| {np.abs(g['mod.gx']).max():.2f}); fused vs autograd {e_tf:.2e}")
    assert e_t < TOL and e_f < TOL and e_g < TOL
    assert e_tf < 1e-5 * max(1.0, y.detach().abs().max().item())
    # the weights' gradients, against the fp64 restatement
    params = [att.to_q.weight, att.to_kv.weight, att.to_out.weight]
    att.train()
    gy = torch.from_numpy(g["mod.gy"]).cuda()
    got = torch.autograd.grad(att(x.detach()), params, gy)
    p64 = [p.detach().double().cpu().requires_grad_(True) for p in params]
    ref = torch.autograd.grad(attention64(x.detach().cpu(), *p64, att.heads), p64, gy.double().cpu())
    for a, r in zip(got, ref):
        assert (a.cpu().double() - r).abs().max().item() < TOL * max(1.0, r.abs().max().item())


def _forward_without_functional_linear():
    """both paths of Attention.forward with torch.nn.functional.linear (what calling a Linear does) made to raise"""
    import torch.nn.functional as F

    g, w = flash_record()
    att = _module(g, w)
    x = torch.from_numpy(g["mod.x"]).cuda()
    _linear = F.linear

    def refuse(*a, **k):
        raise AssertionError("torch.nn.functional.linear reached from Attention.forward")

    F.linear = refuse
    try:
        att(x.clone().requires_grad_(True)).sum().backward()
        att.eval()
        with torch.no_grad():
            att(x)
    finally:
        F.linear = _linear
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in att.parameters())


def test_attention_module_reaches_no_aten_gemm():
    """both paths of Attention.forward run their projections on the pointwise GEMM kernels (fused.pw_conv /
    dense.pointwise) and the core: torch.nn.functional.linear is never reached"""
    _forward_without_functional_linear()


def test_flash_network_vs_reference(flash):
    """strict load of the reference's state dict; eval (fused) and train-mode outputs vs the reference's net(x_start, t)"""
    from p2p_bridge_amd import p2pb as product
    from p2p_bridge_amd.pvcnn_unet import Attention

    cfg, sd, g = flash
    model = product.build_model(cfg, sd, device="cuda")
    assert isinstance(model.model.global_att, Attention)
    x, _ = net_ref.synthetic_patches(2, 1024, seed=0)
    t = torch.from_numpy(g["t"])
    model.eval()
    with torch.no_grad():
        out = model.model(x.cuda(), t.cuda()).cpu().numpy()
    model.train()
    out_t = model.model(x.cuda(), t.cuda()).detach().cpu().numpy()
    e, e_t = np.abs(out - g["net_out"]).max(), np.abs(out_t - g["net_out"]).max()
    print(f"\nflash network: eval {e:.2e}, train {e_t:.2e}")
    assert e < TOL and e_t < TOL


def test_flash_sampler_eager_and_graph(flash):
    """the 5-step sampler, eager and captured, vs the reference's x_pred; the two forms agree bit for bit (as
    tests/test_sampler_features_gpu.py::test_graph_recaptured_when_weights_change asks of replay vs eager)"""
    from p2p_bridge_amd import p2pb as product

    cfg, sd, g = flash
    model = product.build_model(cfg, sd, device="cuda")
    x, _ = net_ref.synthetic_patches(2, 1024, seed=0)
    eager = model.sample(x_start=x.cuda(), steps=5, log_count=5, verbose=False, graph=False)["x_pred"].clone()
    graph = model.sample(x_start=x.cuda(), steps=5, log_count=5, verbose=False, graph=True)["x_pred"].clone()
    replay = model.sample(x_start=x.cuda(), steps=5, log_count=5, verbose=False, graph=True)["x_pred"].clone()
    e_e, e_g = np.abs(eager.cpu().numpy() - g["x_pred"]).max(), np.abs(graph.cpu().numpy() - g["x_pred"]).max()
    print(f"\nflash sampler, 5 steps: eager {e_e:.2e}, graph {e_g:.2e}, eager vs graph {(eager - graph).abs().max().item():.2e}")
    assert e_e < TOL and e_g < TOL
    assert torch.equal(graph, eager) and torch.equal(replay, eager)


def test_flash_training_step_vs_reference(flash):
    """P2PB.forward + backward at the fixture's fixed steps: the loss within 1e-4 relative, the three attention weights'
    gradients within 2e-3 |fixture|max (the gates of tests/test_conditional_gpu.py:296-300)"""
    from p2p_bridge_amd import p2pb as product
    from p2p_bridge_amd import train

    cfg, sd, g = flash
    model = product.build_model(cfg, sd, device="cuda")
    x1, x0 = net_ref.synthetic_patches(2, 1024, seed=0)
    model.train()
    loss = model(x0.cuda(), x1.cuda(), steps=torch.from_numpy(g["loss_steps"]))
    loss.backward()
    print(f"\nflash loss {loss.item():.8f} vs {float(g['loss']):.8f}")
    assert abs(loss.item() - float(g["loss"])) <= 1e-4 * abs(float(g["loss"]))
    params = dict(model.model.named_parameters())
    for k in ("global_att.to_q.weight", "global_att.to_kv.weight", "global_att.to_out.weight"):
        ref = g["grad." + k]
        err = np.abs(params[k].grad.cpu().numpy() - ref).max()
        print(f"  {k}: {err:.2e} (|fixture|max {np.abs(ref).max():.2e})")
        assert err <= 2e-3 * np.abs(ref).max(), k
    # the decoder half of train.segmented_backward finds the new weights by their name prefix
    dec = {id(p) for p in train.decoder_parameters(model.model)}
    assert all(id(params[k]) in dec for k in params if k.startswith("global_att."))


def test_flash_projections_are_audited_and_pinnable(flash):
    """the three projections are split-operand launches like every other layer: fused.operand_audit sees them (so
    P2PB.calibrate_ranges can pin them), and a layer pinned to bf16x6 still computes the reference's output"""
    from p2p_bridge_amd import fused
    from p2p_bridge_amd import p2pb as product

    cfg, sd, g = flash
    model = product.build_model(cfg, sd, device="cuda")
    att = model.model.global_att
    x, _ = net_ref.synthetic_patches(2, 1024, seed=0)
    t = torch.from_numpy(g["t"]).cuda()
    model.eval()
    with torch.no_grad():
        with fused.operand_audit() as audit:
            model.model(x.cuda(), t)
        seen = {id(m) for m in audit.layers}
        assert {id(att.to_q), id(att.to_kv), id(att.to_out)} <= seen
        names = dict(model.model.named_modules())
        assert all(n in names for n, _kind, _amax in model.calibrate_ranges(x.cuda(), steps=5))
        for m in (att.to_q, att.to_kv, att.to_out):
            fused.pin_layer_math(m, "bf16x6")
        try:
            out = model.model(x.cuda(), t).cpu().numpy()
        finally:
            for m in (att.to_q, att.to_kv, att.to_out):
                fused.pin_layer_math(m, None)
    assert np.abs(out - g["net_out"]).max() < TOL


def test_no_attention_network_vs_reference():
    """attention_type = none: no global_att, the bottleneck passes through; eval / train outputs vs the reference's, and the
    sampler runs eager and captured with the same bits"""
    from p2p_bridge_amd import p2pb as product

    g = np.load(os.path.join(GOLDEN, "tiny_noattn.npz"))
    model = product.build_model(tiny_cfg("none"), _weights(), device="cuda")
    assert model.model.global_att is None
    x, _ = net_ref.synthetic_patches(2, 1024, seed=0)
    t = torch.from_numpy(g["t"])
    model.eval()
    with torch.no_grad():
        out = model.model(x.cuda(), t.cuda()).cpu().numpy()
    model.train()
    out_t = model.model(x.cuda(), t.cuda())
    e, e_t = np.abs(out - g["net_out"]).max(), np.abs(out_t.detach().cpu().numpy() - g["net_out"]).max()
    print(f"\nno-attention network: eval {e:.2e}, train {e_t:.2e}")
    assert e < TOL and e_t < TOL
    out_t.square().mean().backward()
    assert all(p.grad is not None for p in model.model.sa_layers.parameters())
    eager = model.sample(x_start=x.cuda(), steps=3, log_count=3, verbose=False, graph=False)["x_pred"].clone()
    graph = model.sample(x_start=x.cuda(), steps=3, log_count=3, verbose=False, graph=True)["x_pred"]
    assert torch.equal(graph, eager)


def test_captured_replay_launches_no_blas_gemm(flash):
    """one replay of the captured sampler step under torch.profiler: the softmax-attention kernel is in it and no BLAS
    GEMM (`Cijk_*` Tensile kernels, gemm / gemv kernels of ATen) is. Where the profiler records no device kernels inside a
    replay, the assertion is instead that Attention.forward never reaches torch.nn.functional.linear."""
    import re

    from torch.profiler import ProfilerActivity, profile

    from p2p_bridge_amd import p2pb as product

    cfg, sd, g = flash
    model = product.build_model(cfg, sd, device="cuda")
    x, _ = net_ref.synthetic_patches(2, 1024, seed=0)
    model.sample(x_start=x.cuda(), steps=2, log_count=2, verbose=False, graph=True)  # capture
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        model.sample(x_start=x.cuda(), steps=2, log_count=2, verbose=False, graph=True)  # replay
        torch.cuda.synchronize()
    names = sorted({e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")})
    print(f"\n{len(names)} distinct device kernels in the replay")
    if not any("_kernel" in n for n in names):
        print("torch.profiler recorded no device kernels inside the graph replay: checking the module's call path instead")
        return _forward_without_functional_linear()
    assert any("softmax_attention_fwd_kernel" in n for n in names), names
    bad = [n for n in names if n.startswith("Cijk_") or re.search(r"gemm|gemv", n, re.I)]
    assert not bad, bad
