"""Times the DINOv2 feature path (p2p_bridge_amd/dinov2.py, csrc/vit.hip, csrc/imgfeat.hip) against plain torch on the same GPU.
Not part of bench.py.

  ViT-S/14 forward at 8 x 3 x 182 x 252 (the reference's default batch of 192 x 256 frames, cropped to patch multiples):
      hip            DinoV2.forward_features: 3 + 7 * depth launches, fp32
      hip fp16       the same weights in a DinoV2(precision="fp16"): fp16 matrix operands on the matrix pipe (csrc/vit_f16.hip),
                     the arithmetic of the autocast line below; same launch count
      torch fp32     the same weights through F.layer_norm / F.linear / F.scaled_dot_product_attention / F.gelu
      torch fp16 autocast   the same under torch.autocast(float16): what the reference runs (image_features.py:494)
  Feature fusion, 8 frames, 300 000 points, C = 384:
      from grid      update_features_from_grid on the f16[8,13,18,384] token grid: one launch
      via the map    F.interpolate to f16[8,384,192,256], channel-last copy, update_features: the default path of fuse_scene
    with the peak bytes each allocates on top of its inputs (the map is 8 * 192 * 256 * 384 * 2 = 302 MB, twice while it is
    being made channel-last).

    python tools/bench_dinov2.py [--batch 8] [--points 300000] [--repeats 7] [--window 0.25] [--out profiles/dinov2_half_timing.txt]

One process, seeded inputs, every variant warmed up, device events around back-to-back calls (as many as fill `window` seconds);
the variants of a comparison are ALTERNATED inside every repeat; median and minimum per call over the repeats. Needs a GPU."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from p2p_bridge_amd import dinov2, image_features as IF  # noqa: E402

F16, I32 = torch.float16, torch.int32
H, W = 192, 256


def per_call_ms(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def compare(variants, repeats, window):
    """variants: [(name, fn)] -> one result per variant; inside every repeat the variants run one after the other"""
    iters = {}
    for name, fn in variants:
        for _ in range(3):  # warm-up: code objects, allocator, clocks
            fn()
        torch.cuda.synchronize()
        iters[name] = max(3, min(2000, int(window * 1e3 / per_call_ms(fn, 3)) + 1))
    times = {name: [] for name, _ in variants}
    for _ in range(repeats):
        for name, fn in variants:
            times[name].append(per_call_ms(fn, iters[name]))
    return [{"what": name, "iters": iters[name], "ms_median": statistics.median(times[name]), "ms_min": min(times[name])}
            for name, _ in variants]


def torch_forward(model, x):
    """the model's definition in plain torch operators with the library's fused attention"""
    b, c, ps, heads = x.shape[0], model.embed_dim, model.patch_size, model.num_heads
    p = model.patch_embed.proj
    t = F.conv2d(x, p.weight, p.bias, stride=ps).flatten(2).transpose(1, 2)
    t = torch.cat([model.cls_token.expand(b, -1, -1).to(t.dtype), t], 1) + model.pos_table(x.shape[2] // ps, x.shape[3] // ps, x.device)
    n = t.shape[1]
    for blk in model.blocks:
        y = F.layer_norm(t, (c,), blk.norm1.weight, blk.norm1.bias, model.eps)
        q, k, v = F.linear(y, blk.attn.qkv.weight, blk.attn.qkv.bias).view(b, n, 3, heads, 64).permute(2, 0, 3, 1, 4)
        a = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(b, n, c)
        t = t + blk.ls1.gamma * F.linear(a, blk.attn.proj.weight, blk.attn.proj.bias)
        y = F.layer_norm(t, (c,), blk.norm2.weight, blk.norm2.bias, model.eps)
        t = t + blk.ls2.gamma * F.linear(F.gelu(F.linear(y, blk.mlp.fc1.weight, blk.mlp.fc1.bias)), blk.mlp.fc2.weight, blk.mlp.fc2.bias)
    return F.layer_norm(t, (c,), model.norm.weight, model.norm.bias, model.eps)


def random_vits(seed):
    """ViT-S/14 with the weight recipe of tools/make_golden_dinov2.py (visible attention rows and branches)"""
    g = torch.Generator().manual_seed(seed)
    model = dinov2.dinov2_vits14()
    sd = model.state_dict()
    for k, v in sd.items():
        if k.endswith("gamma") or (k.endswith("weight") and v.dim() == 1):
            v.copy_(torch.rand(v.shape, generator=g) + 0.5)
        elif v.dim() >= 2 and "weight" in k:
            v.copy_(torch.randn(v.shape, generator=g) / (v[0].numel() ** 0.5))
            if "qkv" in k:
                v[:2 * model.embed_dim] *= 2.0
        else:
            v.copy_(torch.randn(v.shape, generator=g) * 0.5)
    model.load_state_dict(sd)
    return model.cuda()


def half_twin(model):
    """the same weights in an fp16-mode model"""
    twin = dinov2.dinov2_vits14(precision="fp16")
    twin.load_state_dict(model.state_dict())
    return twin.cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--points", type=int, default=300000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dinov2 needs a GPU: nothing is timed on the CPU")
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    b = a.batch
    model = random_vits(0)
    model16 = half_twin(model)
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(b, 3, H - H % 14, W - W % 14, generator=gen, device="cuda")
    emit({"what": "setup", "model": "ViT-S/14", "input": list(x.shape), "tokens": 1 + (x.shape[2] // 14) * (x.shape[3] // 14),
          "hip_launches_per_forward": 3 + 7 * model.depth, "device": torch.cuda.get_device_name(0), "torch": torch.__version__})

    def hip():
        return model.forward_features(x)

    def hip16():
        return model16.forward_features(x)

    @torch.no_grad()
    def torch32():
        return torch_forward(model, x)

    @torch.no_grad()
    def torch16():
        with torch.autocast("cuda", dtype=F16):
            return torch_forward(model, x)

    ref = torch32()
    got = torch.cat([hip()["x_norm_clstoken"][:, None], hip()["x_norm_patchtokens"]], 1)
    got16 = torch.cat([hip16()["x_norm_clstoken"][:, None], hip16()["x_norm_patchtokens"]], 1)
    emit({"what": "agreement", "max_abs_hip_minus_torch_fp32": float((got - ref).abs().max()),
          "max_abs_autocast_minus_torch_fp32": float((torch16().float() - ref).abs().max()),
          "max_abs_hip_fp16_minus_torch_fp32": float((got16 - ref).abs().max()), "rms": float(ref.pow(2).mean().sqrt())})
    res = compare([("vit-s forward hip fp32", hip), ("vit-s forward torch fp32", torch32),
                   ("vit-s forward torch fp16 autocast", torch16), ("vit-s forward hip fp16", hip16)], a.repeats, a.window)
    for r in res:
        r["ms_per_frame_at_median"] = r["ms_median"] / b
        r["relative_to_hip"] = r["ms_median"] / res[0]["ms_median"]
    res[3]["relative_to_torch_fp16_autocast"] = res[3]["ms_median"] / res[2]["ms_median"]
    for r in res:
        emit(r)

    # ---- fusion ------------------------------------------------------------------------------------------------------
    n, c = a.points, model.embed_dim
    grid = hip()["x_norm_patchtokens"].half().reshape(b, x.shape[2] // 14, x.shape[3] // 14, c).contiguous()
    xy = torch.stack([torch.randint(0, W, (b, n), generator=gen, device="cuda"), torch.randint(0, H, (b, n), generator=gen, device="cuda")],
                     -1).to(I32)
    valid = torch.rand(b, n, generator=gen, device="cuda") < 0.5
    mean, count = torch.zeros(n, c, dtype=F16, device="cuda"), torch.zeros(n, dtype=I32, device="cuda")

    def from_grid():
        IF.update_features_from_grid(mean, count, grid, (H, W), valid, xy)

    def via_map():
        feat = F.interpolate(grid.permute(0, 3, 1, 2), size=(H, W), mode="bilinear", antialias=False)
        IF.update_features(mean, count, feat.permute(0, 2, 3, 1).contiguous(), valid, xy)

    peaks = {}
    for name, fn in (("from grid", from_grid), ("via the map", via_map)):
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated() - base
    res = compare([("fusion from grid (update_features_from_grid)", from_grid),
                   ("fusion via the map (F.interpolate + update_features)", via_map)], a.repeats, a.window)
    res[0]["peak_bytes_allocated"], res[1]["peak_bytes_allocated"] = peaks["from grid"], peaks["via the map"]
    for r in res:
        r.update({"frames": b, "points": n, "channels": c, "valid_pairs": int(valid.sum()), "relative_to_from_grid": r["ms_median"] / res[0]["ms_median"]})
        emit(r)
    emit({"what": "map bytes from shapes", "bytes": b * H * W * c * 2})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
