"""model.PVD.attention_type = linear | flash | anything else (models/unet_pvc.py:96-101,124-125): module trees against the
reference's manifests, the two configurations with no behaviour to mirror, and the fp64 restatement of the softmax
attention contract (shared with tests/test_softmax_attention_gpu.py) against the reference's own module output."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN


def tiny_cfg(attention_type, attentions=None):
    cfg = copy.deepcopy(json.load(open(os.path.join(GOLDEN, "tiny_cfg.json"))))
    cfg["model"]["PVD"]["attention_type"] = attention_type
    if attentions is not None:
        cfg["model"]["PVD"]["attentions"] = attentions
    return cfg


def manifest(name):
    return {k: tuple(v) for k, v in json.load(open(os.path.join(GOLDEN, name))).items()}


def core64(q, kv, heads):
    """the core in the given precision on channel-major operands: q [B, heads*32, n], kv [B, 2*heads*32, n] (k | v) ->
    [B, heads*32, n]; channel index = head*32 + j, scale 32^-0.5, softmax over the keys, no mask"""
    b, c, n = q.shape
    k, v = kv[:, :c], kv[:, c:]
    q, k, v = (z.reshape(b, heads, 32, n) for z in (q, k, v))
    sim = torch.einsum("bhdi,bhdj->bhij", q, k) * 32 ** -0.5
    return torch.einsum("bhij,bhdj->bhdi", sim.softmax(dim=-1), v).reshape(b, c, n)


def attention64(x, w_q, w_kv, w_out, heads):
    """the contract on x [B, C, n] in fp64: q = x W_q^T, k | v = x W_kv^T (first half k), per-head softmax attention,
    y = concat_h(out_h) W_out^T; no bias, no norm, no residual -> [B, C, n]"""
    x, w_q, w_kv, w_out = (z.double() for z in (x, w_q, w_kv, w_out))
    xt = x.transpose(1, 2)  # [B, n, C]
    q, kv = xt @ w_q.T, xt @ w_kv.T
    out = core64(q.transpose(1, 2), kv.transpose(1, 2), heads)
    return (out.transpose(1, 2) @ w_out.T).transpose(1, 2)


def flash_record():
    g = np.load(os.path.join(GOLDEN, "tiny_flash.npz"))
    w = {k[2:]: torch.from_numpy(g[k]).float() for k in g.files if k.startswith("w.")}
    return g, w


def test_flash_module_tree_matches_reference():
    from p2p_bridge_amd.pvcnn_unet import Attention, PVCNN2Unet

    net = PVCNN2Unet(tiny_cfg("flash"))
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == manifest("manifest_tiny_flash.json")
    assert isinstance(net.global_att, Attention)
    assert [k for k, _ in net.global_att.named_parameters()] == ["to_q.weight", "to_kv.weight", "to_out.weight"]
    _, w = flash_record()
    missing, unexpected = net.load_state_dict(w, strict=False)
    assert not unexpected and not [k for k in missing if k.startswith("global_att.")]


@pytest.mark.parametrize("name", ["none", "None", "softmax"])
def test_no_attention_module_tree_matches_reference(name):
    from p2p_bridge_amd.pvcnn_unet import PVCNN2Unet

    net = PVCNN2Unet(tiny_cfg(name))
    assert net.global_att is None
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == manifest("manifest_tiny_noattn.json")
    assert not net._decoder_adagns() - {id(m) for m in net.modules()}  # (walks global_att: None is skipped)


def test_linear_stays_the_default():
    from test_host_logic import PVDS
    from p2p_bridge_amd.pvcnn_unet import LinearAttention, PVCNN2Unet

    net = PVCNN2Unet(PVDS)
    assert isinstance(net.global_att, LinearAttention)
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == manifest("manifest_PVDS.json")
    cfg = tiny_cfg("flash")
    del cfg["model"]["PVD"]["attention_type"]  # (models/unet_pvc.py:50: default "linear")
    assert isinstance(PVCNN2Unet(cfg).global_att, LinearAttention)


@pytest.mark.parametrize("name", ["flash", "none"])
def test_pvconv_level_attention_needs_linear(name):
    """attentions flags a stage that has a PVConv: the reference's Attention would run its Linear(C) along the point axis
    (models/pvcnn.py:329-330), and with no attention type it calls None(out_channels) -- refused at construction"""
    from p2p_bridge_amd.pvcnn_unet import PVCNN2Unet

    with pytest.raises(ValueError, match="attention"):
        PVCNN2Unet(tiny_cfg(name, attentions=[1, 1, 0, 1]))
    PVCNN2Unet(tiny_cfg("linear", attentions=[1, 1, 0, 1]))  # (the linear form of the same config still builds)


def test_fp64_restatement_reproduces_reference_module():
    """the yardstick of the GPU tests, tied to the reference: its Attention(128, norm=False, flash=True, heads=4) output and
    input gradient (tests/golden/tiny_flash.npz mod.*, tools/make_golden_attention.py) vs the restatement, 1e-6 relative"""
    g, w = flash_record()
    x = torch.from_numpy(g["mod.x"]).double().requires_grad_(True)
    y = attention64(x, w["global_att.to_q.weight"], w["global_att.to_kv.weight"], w["global_att.to_out.weight"],
                    int(g["mod.heads"]))
    y.backward(torch.from_numpy(g["mod.gy"]).double())
    for got, ref in ((y.detach(), g["mod.y"]), (x.grad, g["mod.gx"])):
        ref = torch.from_numpy(ref).double()
        assert got.shape == ref.shape
        assert (got - ref).abs().max().item() <= 1e-6 * ref.abs().max().item()


def test_attention_has_no_eager_form():
    """a host tensor is refused (no CPU / eager fallback, p2p_bridge_amd/_lib.py) instead of running the Linears along the
    wrong axis"""
    from p2p_bridge_amd.pvcnn_unet import Attention, _SoftmaxAttentionCore

    with pytest.raises(RuntimeError, match="CUDA"):
        Attention(64, heads=4)(torch.randn(1, 64, 8))
    with pytest.raises(RuntimeError, match="CUDA"):
        _SoftmaxAttentionCore.apply(torch.randn(1, 128, 8), torch.randn(1, 256, 8), 4)
