"""Fixtures of `attention_type: flash` / `none` under tests/golden/, generated like tools/make_golden_extra.py by running
the REFERENCE's own Python (imported through tools/ref_import on CPU, the C oracle standing in for its CUDA extension).
Build container only.

    python tools/make_golden_attention.py

  tiny_flash.npz    the tiny config with model.PVD.attention_type = "flash" (models/unet_pvc.py:98-99: global_att is
                    `Attention(dim, norm=False, flash=True, heads=...)`, models/modules.py:197-264):
                      w.global_att.*   its three Linear weights (torch.manual_seed(11), fp16-rounded); every other parameter
                                       is tiny_weights.npz's (whose linear global_att.to_qkv / to_out entries are dropped)
                      t, net_out       net(x_start, t) in eval mode, x_start = synthetic_patches(2, 1024, seed=0)
                      x_pred           the 5-step P2PB.sample(x_start)
                      loss_steps, loss, grad.global_att.*
                                       P2PB.forward(clean, x_start) (mse) at fixed steps with the gradients of the three weights
                      mod.*            one module-level record: the reference's Attention(128, norm=False, flash=True, heads=4)
                                       with these weights on a seeded x [2, 128, 37] (handed over as [B, n, C] and back, as
                                       unet_pvc.py:239-241 does) -> y, and dL/dx for a seeded upstream gradient gy
  tiny_noattn.npz   attention_type = "none" (unet_pvc.py:100-101,124-125: no global_att is built; the instance gets
                    `global_att = None`, which the reference's forward tests for but its constructor never sets): t, net_out
  manifest_tiny_flash.json, manifest_tiny_noattn.json   parameter name -> shape
"""
import json
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")
from tools import ref_import  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def main():
    unet, p2pb = ref_import.load_models()
    import importlib

    from oracle import net_ref

    modules = importlib.import_module("models.modules")
    raw = json.load(open(os.path.join(OUT, "tiny_cfg.json")))
    w = np.load(os.path.join(OUT, "tiny_weights.npz"))
    sd = {k: torch.from_numpy(w[k]).float() for k in w.files if not k.startswith("global_att.")}
    x_start, clean = net_ref.synthetic_patches(2, 1024, seed=0)
    t = torch.tensor([500.0, 123.0])
    steps = torch.tensor([10, 700])

    # ---- attention_type = flash -------------------------------------------------------------------------------------
    r = json.loads(json.dumps(raw))
    r["model"]["PVD"]["attention_type"] = "flash"
    cfg = ref_import.to_attr(r)
    cfg.gpu = "cpu"
    torch.manual_seed(11)
    net = unet.PVCNN2Unet(cfg)
    full = net.state_dict()
    extra = {k: v.half().float() for k, v in full.items() if k not in sd}
    assert sorted(extra) == ["global_att.to_kv.weight", "global_att.to_out.weight", "global_att.to_q.weight"], sorted(extra)
    net.load_state_dict({**sd, **extra})
    json.dump({k: list(v.shape) for k, v in full.items()}, open(os.path.join(OUT, "manifest_tiny_flash.json"), "w"), indent=0)
    out = {"t": t.numpy(), "loss_steps": steps.numpy()}
    net.eval()
    with torch.no_grad():
        out["net_out"] = net(x_start, t).numpy()
    model = p2pb.P2PB(cfg, net)
    out["x_pred"] = model.sample(x_start=x_start, steps=5, verbose=False, log_count=5)["x_pred"].numpy()
    _randint = torch.randint
    torch.randint = lambda *a, **k: steps.clone()
    try:
        model.model.train()
        for p in net.parameters():
            p.grad = None
        loss = model(clean.clone(), x_start.clone())
        loss.backward()
    finally:
        torch.randint = _randint
    out["loss"] = loss.detach().numpy()
    for k in extra:
        out["grad." + k] = dict(net.named_parameters())[k].grad.numpy()
        out["w." + k] = extra[k].half().numpy()

    # the module alone
    dim, heads, n = extra["global_att.to_q.weight"].shape[1], r["model"]["PVD"]["attention_heads"], 37
    att = modules.Attention(dim, norm=False, flash=True, heads=heads)
    att.load_state_dict({k[len("global_att."):]: v for k, v in extra.items()})
    g = torch.Generator().manual_seed(12)
    x = torch.randn(2, dim, n, generator=g).requires_grad_(True)
    gy = torch.randn(2, dim, n, generator=g)
    y = att(x.permute(0, 2, 1)).permute(0, 2, 1)
    y.backward(gy)
    out.update({"mod.x": x.detach().numpy(), "mod.gy": gy.numpy(), "mod.y": y.detach().numpy(), "mod.gx": x.grad.numpy(),
                "mod.heads": np.array(heads)})
    np.savez_compressed(os.path.join(OUT, "tiny_flash.npz"), **out)

    # ---- attention_type = none --------------------------------------------------------------------------------------
    r = json.loads(json.dumps(raw))
    r["model"]["PVD"]["attention_type"] = "none"
    cfg = ref_import.to_attr(r)
    cfg.gpu = "cpu"
    net = unet.PVCNN2Unet(cfg)
    full = net.state_dict()
    assert sorted(full) == sorted(sd), set(full) ^ set(sd)
    net.load_state_dict(sd)
    # The reference's constructor defines `global_att` only when there is an attention (unet_pvc.py:124-125) while its
    # forward asks `if self.global_att is not None` (:234): as it stands, forward() of such a network ends in an
    # AttributeError. The attribute the forward tests for is set here, on the instance; every value below is then computed
    # by the reference's own code along the branch it wrote for this case (the bottleneck features pass through).
    assert not hasattr(net, "global_att")
    net.global_att = None
    json.dump({k: list(v.shape) for k, v in full.items()}, open(os.path.join(OUT, "manifest_tiny_noattn.json"), "w"), indent=0)
    net.eval()
    with torch.no_grad():
        y = net(x_start, t)
    np.savez_compressed(os.path.join(OUT, "tiny_noattn.npz"), t=t.numpy(), net_out=y.numpy())
    print({f: os.path.getsize(os.path.join(OUT, f)) for f in ("tiny_flash.npz", "tiny_noattn.npz", "manifest_tiny_flash.json",
                                                              "manifest_tiny_noattn.json")}, float(out["loss"]))


if __name__ == "__main__":
    main()
