"""A plain-torch restatement of the DINOv2 ViT forward in the hub checkpoints' names, for the tests (a helper module, not a
conftest): dtype-generic, so the same code is the float64 reference and the fp32 yardstick of the gates. It shares no code
with p2p_bridge_amd/dinov2.py: explicit mean / variance LayerNorm, explicit erf GELU, explicit softmax.

Also here, because the tool and the tests both need them: the seeded weight recipe of tools/make_golden_dinov2.py (weights
under the hub names; default initialisations give near-uniform softmax rows and invisible branches, under which a wrong
attention scale or a missing LayerScale passes) and the gate `4 x the error of this forward in fp32 against its own float64`.
"""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dinov2_tiny.npz")
HEAD_DIM = 64
GATE_FACTOR = 4  # the margin the project gives its own arithmetic over an fp32 evaluation (test_full_size_parity_gpu.py)


def pos_table(pos_embed, grid, h, w, offset=0.0):
    """[1 + h*w, C] in the dtype of pos_embed; the interpolation itself runs in fp32 (as `transformers` does for any dtype)"""
    pos = pos_embed[0]
    if h == grid and w == grid:
        return pos
    c = pos.shape[-1]
    patch = pos[1:].float().reshape(1, grid, grid, c).permute(0, 3, 1, 2)
    if offset > 0:
        patch = F.interpolate(patch, scale_factor=((h + offset) / grid, (w + offset) / grid), mode="bicubic", antialias=False)
    else:
        patch = F.interpolate(patch, size=(h, w), mode="bicubic", antialias=False)
    assert tuple(patch.shape[-2:]) == (h, w)
    return torch.cat([pos[:1], patch.permute(0, 2, 3, 1).reshape(h * w, c).to(pos.dtype)])


def layer_norm(x, weight, bias, eps):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * weight + bias


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def attention(q, k, v):
    """q, k, v [B, heads, T, 64] -> [B, heads, T, 64]"""
    s = (q * HEAD_DIM ** -0.5) @ k.transpose(-1, -2)
    s = s - s.amax(-1, keepdim=True)
    p = torch.exp(s)
    return (p / p.sum(-1, keepdim=True)) @ v


def forward(sd, x, patch_size=14, eps=1e-6, offset=0.0, dtype=torch.float64, taps=None):
    """sd: weights under the hub names (any float dtype), x [B,3,H,W] -> (hidden states: the embeddings, then the stream after
    each block; normalised tokens [B, T, C]), everything in `dtype`. taps (a dict): receives max |post-GELU activation| per block"""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    x = x.to(dtype)
    b, _, hh, ww = x.shape
    h, w = hh // patch_size, ww // patch_size
    wt = sd["patch_embed.proj.weight"]
    c = wt.shape[0]
    heads = c // HEAD_DIM
    grid = int(round(math.sqrt(sd["pos_embed"].shape[1] - 1)))
    patches = x.reshape(b, 3, h, patch_size, w, patch_size).permute(0, 2, 4, 1, 3, 5).reshape(b, h * w, -1)
    t = patches @ wt.reshape(c, -1).t() + sd["patch_embed.proj.bias"]
    t = torch.cat([sd["cls_token"].expand(b, -1, -1), t], 1) + pos_table(sd["pos_embed"], grid, h, w, offset)
    n = t.shape[1]
    hidden = [t]  # (the embeddings first, as `transformers` lists them)
    i = 0
    while f"blocks.{i}.norm1.weight" in sd:
        p = f"blocks.{i}."
        y = layer_norm(t, sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
        qkv = (y @ sd[p + "attn.qkv.weight"].t() + sd[p + "attn.qkv.bias"]).reshape(b, n, 3, heads, HEAD_DIM).permute(2, 0, 3, 1, 4)
        a = attention(qkv[0], qkv[1], qkv[2]).transpose(1, 2).reshape(b, n, c)
        t = t + sd[p + "ls1.gamma"] * (a @ sd[p + "attn.proj.weight"].t() + sd[p + "attn.proj.bias"])
        y = layer_norm(t, sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
        y = gelu(y @ sd[p + "mlp.fc1.weight"].t() + sd[p + "mlp.fc1.bias"])
        if taps is not None:
            taps.setdefault("post_gelu_max", []).append(float(y.abs().max()))
        t = t + sd[p + "ls2.gamma"] * (y @ sd[p + "mlp.fc2.weight"].t() + sd[p + "mlp.fc2.bias"])
        hidden.append(t)
        i += 1
    return hidden, layer_norm(t, sd["norm.weight"], sd["norm.bias"], eps)


def gate(sd, x, **kw):
    """(float64 hidden states, float64 tokens, per-layer gates, token gate): a gate is GATE_FACTOR x max |fp32 - fp64| of this
    restatement on this case -- torch's fp32 on the CPU is the yardstick, never the code under test"""
    h64, t64 = forward(sd, x, dtype=torch.float64, **kw)
    h32, t32 = forward(sd, x, dtype=torch.float32, **kw)
    gates = [GATE_FACTOR * float((a.double() - b).abs().max()) for a, b in zip(h32, h64)]
    return h64, t64, gates, GATE_FACTOR * float((t32.double() - t64).abs().max())


# ---- the weight recipe -----------------------------------------------------------------------------------------------
def random_weights(embed_dim, depth, grid, seed, patch_size=14, mlp_ratio=4):
    """Weights under the hub names from a seeded CPU generator, rounded to fp16 (returned as fp32): matrices N(0, 1/fan_in)
    with the query and key rows x 2, LayerScale and norm weights U[0.5, 1.5], biases, cls_token and pos_embed N(0, 0.25)
    (standard deviation 0.5)."""
    g = torch.Generator().manual_seed(seed)
    c, hid = embed_dim, int(embed_dim * mlp_ratio)

    def mat(out, inp):
        return torch.randn(out, inp, generator=g) / math.sqrt(inp)

    def vec(*shape):
        return torch.randn(*shape, generator=g) * 0.5

    def scale(n):
        return torch.rand(n, generator=g) + 0.5

    sd = {"cls_token": vec(1, 1, c), "pos_embed": vec(1, 1 + grid * grid, c), "mask_token": vec(1, c),
          "patch_embed.proj.weight": mat(c, 3 * patch_size ** 2).reshape(c, 3, patch_size, patch_size),
          "patch_embed.proj.bias": vec(c)}
    for i in range(depth):
        p = f"blocks.{i}."
        qkv = mat(3 * c, c)
        qkv[:2 * c] *= 2.0
        sd.update({p + "norm1.weight": scale(c), p + "norm1.bias": vec(c), p + "attn.qkv.weight": qkv,
                   p + "attn.qkv.bias": vec(3 * c), p + "attn.proj.weight": mat(c, c), p + "attn.proj.bias": vec(c),
                   p + "ls1.gamma": scale(c), p + "norm2.weight": scale(c), p + "norm2.bias": vec(c),
                   p + "mlp.fc1.weight": mat(hid, c), p + "mlp.fc1.bias": vec(hid), p + "mlp.fc2.weight": mat(c, hid),
                   p + "mlp.fc2.bias": vec(c), p + "ls2.gamma": scale(c)})
    sd.update({"norm.weight": scale(c), "norm.bias": vec(c)})
    return {k: v.half().float() for k, v in sd.items()}


def images(b, h, w, seed):
    """normalised-looking inputs, rounded to fp16 (returned as fp32)"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(b, 3, h, w, generator=g).half().float()


def hub_from_transformers(sd):
    """the `transformers` names -> the hub names (query | key | value stacked to attn.qkv)"""
    out = {"cls_token": sd["embeddings.cls_token"], "mask_token": sd["embeddings.mask_token"],
           "pos_embed": sd["embeddings.position_embeddings"],
           "patch_embed.proj.weight": sd["embeddings.patch_embeddings.projection.weight"],
           "patch_embed.proj.bias": sd["embeddings.patch_embeddings.projection.bias"],
           "norm.weight": sd["layernorm.weight"], "norm.bias": sd["layernorm.bias"]}
    i = 0
    while f"encoder.layer.{i}.norm1.weight" in sd:
        s, d = f"encoder.layer.{i}.", f"blocks.{i}."
        for p in ("weight", "bias"):
            out[f"{d}norm1.{p}"], out[f"{d}norm2.{p}"] = sd[f"{s}norm1.{p}"], sd[f"{s}norm2.{p}"]
            out[f"{d}attn.qkv.{p}"] = torch.cat([sd[f"{s}attention.attention.{n}.{p}"] for n in ("query", "key", "value")])
            out[f"{d}attn.proj.{p}"] = sd[f"{s}attention.output.dense.{p}"]
            out[f"{d}mlp.fc1.{p}"], out[f"{d}mlp.fc2.{p}"] = sd[f"{s}mlp.fc1.{p}"], sd[f"{s}mlp.fc2.{p}"]
        out[f"{d}ls1.gamma"], out[f"{d}ls2.gamma"] = sd[f"{s}layer_scale1.lambda1"], sd[f"{s}layer_scale2.lambda1"]
        i += 1
    return out


def transformers_from_hub(sd):
    c = sd["norm.weight"].shape[0]
    out = {"embeddings.cls_token": sd["cls_token"], "embeddings.mask_token": sd["mask_token"],
           "embeddings.position_embeddings": sd["pos_embed"],
           "embeddings.patch_embeddings.projection.weight": sd["patch_embed.proj.weight"],
           "embeddings.patch_embeddings.projection.bias": sd["patch_embed.proj.bias"],
           "layernorm.weight": sd["norm.weight"], "layernorm.bias": sd["norm.bias"]}
    i = 0
    while f"blocks.{i}.norm1.weight" in sd:
        s, d = f"blocks.{i}.", f"encoder.layer.{i}."
        for p in ("weight", "bias"):
            out[f"{d}norm1.{p}"], out[f"{d}norm2.{p}"] = sd[f"{s}norm1.{p}"], sd[f"{s}norm2.{p}"]
            for j, n in enumerate(("query", "key", "value")):
                out[f"{d}attention.attention.{n}.{p}"] = sd[f"{s}attn.qkv.{p}"][j * c:(j + 1) * c]
            out[f"{d}attention.output.dense.{p}"] = sd[f"{s}attn.proj.{p}"]
            out[f"{d}mlp.fc1.{p}"], out[f"{d}mlp.fc2.{p}"] = sd[f"{s}mlp.fc1.{p}"], sd[f"{s}mlp.fc2.{p}"]
        out[f"{d}layer_scale1.lambda1"], out[f"{d}layer_scale2.lambda1"] = sd[f"{s}ls1.gamma"], sd[f"{s}ls2.gamma"]
        i += 1
    return out


# ---- the stored cases (tools/make_golden_dinov2.py) ------------------------------------------------------------------
CASES = {"a": (2, 182, 252), "b": (1, 70, 70), "c": (1, 14, 14)}  # 13 x 18 tokens from the 5 x 5 table; native grid; one patch
HIDDEN_ROWS = slice(0, None, 5)  # case a stores the hidden states of image 1 at every 5th token (file size)


def image_from_u8(u8):
    """stored uint8 pixels -> the (already normalised) model input: (p - 128) / 64, exact in fp16"""
    return (u8.float() - 128.0) / 64.0


def load_golden():
    """-> (weights under the `transformers` names as fp32 tensors, {case: {x, last_hidden_state, hidden_states}}, figures)"""
    z = np.load(GOLDEN)
    sd = {k[2:]: torch.from_numpy(z[k]).float() for k in z.files if k.startswith("w.")}
    figures = {k: z[k] for k in z.files if not k.startswith("w.")}
    cases = {}
    for name in CASES:
        f = np.load(GOLDEN.replace(".npz", f"_case_{name}.npz"))
        cases[name] = {k: torch.from_numpy(f[k]) for k in f.files}
        cases[name]["x"] = image_from_u8(cases[name].pop("x_u8"))
    return sd, cases, figures
