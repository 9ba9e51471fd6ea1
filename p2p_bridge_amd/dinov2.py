"""DINOv2 point features: the ViT whose patch tokens the reference's room pipeline fuses onto its scans
(data/processing/image_features.py:21-33 `load_dino`, :88-111 `get_dino_features`; configs/PVDL_*.yaml `point_features: dino`).
The reference fetches the model with torch.hub; here it is built from a checkpoint FILE:

    model = dinov2.dinov2_vits14()
    model.load_state_dict(torch.load("dinov2_vits14_pretrain.pth"))        # strict: the hub's names and shapes
    feats = image_features.fuse_scene(points, frames, "dino", feature_fn=dinov2.feature_fn(model.cuda()))
    image_features.save_features("scene_dino.npy", feats)                    # f16[384, N], what room_data reads

    DinoV2                    the module (parameters named as in the hub checkpoints), `forward_features`
    dinov2_vits14 / _vitb14 / _vitl14   the presets with an MLP block and no register tokens (head dimension 64)
    DinoV2.from_transformers_state_dict  the same weights under the `transformers` names
    get_dino_features         :88-111: normalise, crop to patch multiples, patch tokens .half(), reshape, bilinear upsample
    feature_fn                the callable `image_features.fuse_scene` expects

CUDA tensors run the kernels of csrc/vit.hip and csrc/vit_f16.hip (include/p2pb_hip.h, "vision transformer"): 3 + 7 * depth
launches per `forward_features`, tokens row-major [B*T, C]; there is no fallback from them. CPU tensors take a torch path under
the same definition (F.linear, F.layer_norm, exact-erf GELU, softmax attention with q scaled by 64^-0.5), which is what the CPU
tests hold against the stored float64 results of `transformers.Dinov2Model`.

Arithmetic, `precision="fp32"` (the default; README "Arithmetic"): fp32 operands and results. The reference runs the model under
fp16 autocast (:494) and then takes `.half()` of the tokens; here the forward is fp32 and the tokens are rounded to fp16 once,
where that `.half()` stands.
`precision="fp16"` is the reference's arithmetic on the matrix pipe (csrc/vit_f16.hip): ONLY the operands of the matrix products
are fp16, each rounded once to nearest-even -- the outputs of norm1 and norm2, the qkv rows, the softmax weights entering P.V,
the attention output, the post-GELU activations and the weights of attn.qkv, attn.proj, mlp.fc1 and mlp.fc2 (made by `.half()`
once per model and cached; `load_state_dict` and `.to()` / `.cuda()` drop the cache). The residual stream, LayerNorm statistics,
softmax, bias, GELU, LayerScale and every accumulation stay fp32, patch embedding and the final norm run the fp32 kernels, and
`forward_features` returns fp32 as before. The conversion is IEEE: a value beyond +-65504 becomes +-inf, as `Tensor.half()` and
the reference under autocast make it -- nothing saturates and the hot path checks nothing, so a checkpoint whose post-GELU
activations leave the fp16 range needs `precision="fp32"`. A CPU model in fp16 mode restates the same roundings in torch.

Position embedding: the [1 + grid^2, C] table is interpolated ON THE HOST in fp32 with F.interpolate(mode="bicubic",
antialias=False), once per (h, w), and cached (plumbing, not hot; the same table feeds both paths). `interpolate_offset == 0`
passes size=(h, w): what `transformers` does and what tests/golden/dinov2_tiny.npz pins. `interpolate_offset > 0` passes
scale_factor=((h + o) / grid, (w + o) / grid), the rule of the hub model (constructor default 0.1): that branch follows the
published code FROM MEMORY and is not pinned by any stored result (INTEGRATION.md lists it). h == w == grid: the table as it is.

The SwiGLU giant (vitg14) and the register-token variants (*_reg) are not supported and raise ValueError.
"""
import math

import torch
import torch.nn.functional as F
from torch import nn

from ._lib import ask, call, ptr, stream_ptr

F16, F32 = torch.float16, torch.float32
IMAGENET_DEFAULT_MEAN = (0.485, 0.456, 0.406)
IMAGENET_DEFAULT_STD = (0.229, 0.224, 0.225)
HEAD_DIM = 64
EPI_BIAS, EPI_GELU, EPI_RESIDUAL = 0, 1, 2  # P2PB_VIT_EPI_*

PRESETS = {
    "dinov2_vits14": dict(embed_dim=384, depth=12, num_heads=6),
    "dinov2_vitb14": dict(embed_dim=768, depth=12, num_heads=12),
    "dinov2_vitl14": dict(embed_dim=1024, depth=24, num_heads=16),
}


# ---- the operators of csrc/vit.hip, one launch each (CUDA tensors only: no fallback) ----------------------------------------
def _f32_cuda(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor (dinov2 operators have no CPU fallback; the model's CPU path is torch)")
    if t.dtype != F32 or not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous float32 tensor")
    return t


def layernorm(x, weight, bias, eps=1e-6, out_dtype=F32):
    """LayerNorm over the last axis of x f32[..., C] (two-pass, biased variance) -> a new tensor; out_dtype=torch.float16: the
    same fp32 result rounded once in the kernel (the bits of `layernorm(...).half()`)"""
    c = x.shape[-1]
    _f32_cuda(x, "x"), _f32_cuda(weight, "weight"), _f32_cuda(bias, "bias")
    if weight.shape != (c,) or bias.shape != (c,) or x.numel() == 0:
        raise ValueError(f"layernorm: x {list(x.shape)}, weight {list(weight.shape)}, bias {list(bias.shape)}")
    if out_dtype not in (F32, F16):
        raise ValueError(f"layernorm: out_dtype {out_dtype} is not float32 or float16")
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    call("p2pb_vit_layernorm" if out_dtype == F32 else "p2pb_vit_layernorm_f16", x.numel() // c, c,
         ptr(x), ptr(weight), ptr(bias), eps, ptr(y), stream_ptr())
    return y


def linear(x, weight, bias, gelu=False, residual=None, gamma=None):
    """x f32[M,K] @ weight[N,K]^T + bias -> f32[M,N]; gelu=True: the exact-erf GELU of it; residual (f32[M,N], updated IN
    PLACE and returned) with gamma f32[N]: residual += gamma * (x @ weight^T + bias)"""
    _f32_cuda(x, "x"), _f32_cuda(weight, "weight"), _f32_cuda(bias, "bias")
    if x.dim() != 2 or weight.dim() != 2 or x.shape[1] != weight.shape[1] or bias.shape != (weight.shape[0],) or x.shape[0] < 1:
        raise ValueError(f"linear: x {list(x.shape)}, weight {list(weight.shape)}, bias {list(bias.shape)}")
    m, k, n = x.shape[0], x.shape[1], weight.shape[0]
    if (residual is None) != (gamma is None) or (gelu and residual is not None):
        raise ValueError("linear: residual and gamma come together, and not with gelu")
    if residual is not None:
        _f32_cuda(residual, "residual"), _f32_cuda(gamma, "gamma")
        if residual.shape != (m, n) or gamma.shape != (n,):
            raise ValueError(f"linear: residual {list(residual.shape)}, gamma {list(gamma.shape)}")
    y = residual if residual is not None else torch.empty(m, n, dtype=F32, device=x.device)
    epi = EPI_RESIDUAL if residual is not None else EPI_GELU if gelu else EPI_BIAS
    call("p2pb_vit_linear", m, n, k, ptr(x), ptr(weight), ptr(bias), epi, ptr(gamma), ptr(y), stream_ptr())
    return y


def attention(qkv, heads, n_valid=None):
    """qkv f32[B, n, 3*heads*64] (channels (q | k | v) x heads x 64) -> f32[B, n, heads*64]: softmax((q 64^-0.5) k^T) v over the
    keys < n_valid (default n). Rows >= n_valid are padding: never read, their output rows are zeros."""
    _f32_cuda(qkv, "qkv")
    if qkv.dim() != 3 or qkv.shape[2] != 3 * heads * HEAD_DIM or qkv.shape[0] < 1 or qkv.shape[1] < 1:
        raise ValueError(f"attention: qkv {list(qkv.shape)} is not [B, n, {3 * heads * HEAD_DIM}]")
    b, n = qkv.shape[:2]
    n_valid = n if n_valid is None else int(n_valid)
    if not 1 <= n_valid <= n:
        raise ValueError(f"attention: n_valid {n_valid} outside [1, {n}]")
    out = torch.empty(b, n, heads * HEAD_DIM, dtype=F32, device=qkv.device)
    call("p2pb_vit_attention_forward", b, heads, n, n_valid, ptr(qkv), ptr(out), stream_ptr())
    return out


# ---- the operators of csrc/vit_f16.hip: fp16 matrix operands, fp32 everything else ------------------------------------------
def _f16_cuda(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor (dinov2 operators have no CPU fallback; the model's CPU path is torch)")
    if t.dtype != F16 or not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous float16 tensor")
    return t


def linear_half(x, weight, bias, gelu=False, residual=None, gamma=None):
    """x f16[M,K] @ weight f16[N,K]^T + bias f32[N], accumulated in fp32 -> f16[M,N] (rounded once, IEEE); gelu=True: the
    exact-erf GELU of the fp32 sum, then rounded; residual (f32[M,N], updated IN PLACE and returned) with gamma f32[N]:
    residual += gamma * (x @ weight^T + bias), all fp32. N % 64 == 0 and K % 32 == 0."""
    _f16_cuda(x, "x"), _f16_cuda(weight, "weight"), _f32_cuda(bias, "bias")
    if x.dim() != 2 or weight.dim() != 2 or x.shape[1] != weight.shape[1] or bias.shape != (weight.shape[0],) or x.shape[0] < 1:
        raise ValueError(f"linear_half: x {list(x.shape)}, weight {list(weight.shape)}, bias {list(bias.shape)}")
    m, k, n = x.shape[0], x.shape[1], weight.shape[0]
    if n % 64 or k % 32:
        raise ValueError(f"linear_half: N = {n} must be a multiple of 64 and K = {k} of 32")
    if (residual is None) != (gamma is None) or (gelu and residual is not None):
        raise ValueError("linear_half: residual and gamma come together, and not with gelu")
    if residual is not None:
        _f32_cuda(residual, "residual"), _f32_cuda(gamma, "gamma")
        if residual.shape != (m, n) or gamma.shape != (n,):
            raise ValueError(f"linear_half: residual {list(residual.shape)}, gamma {list(gamma.shape)}")
    y = residual if residual is not None else torch.empty(m, n, dtype=F16, device=x.device)
    epi = EPI_RESIDUAL if residual is not None else EPI_GELU if gelu else EPI_BIAS
    call("p2pb_vit_linear_f16", m, n, k, ptr(x), ptr(weight), ptr(bias), epi,
         ptr(gamma), ptr(y), stream_ptr())
    return y


def attention_half(qkv, heads, n_valid=None):
    """`attention` for qkv f16[B, n, 3*heads*64] -> f16[B, n, heads*64]: both products on the matrix pipe, softmax in fp32"""
    _f16_cuda(qkv, "qkv")
    if qkv.dim() != 3 or qkv.shape[2] != 3 * heads * HEAD_DIM or qkv.shape[0] < 1 or qkv.shape[1] < 1:
        raise ValueError(f"attention_half: qkv {list(qkv.shape)} is not [B, n, {3 * heads * HEAD_DIM}]")
    b, n = qkv.shape[:2]
    n_valid = n if n_valid is None else int(n_valid)
    if not 1 <= n_valid <= n:
        raise ValueError(f"attention_half: n_valid {n_valid} outside [1, {n}]")
    out = torch.empty(b, n, heads * HEAD_DIM, dtype=F16, device=qkv.device)
    call("p2pb_vit_attention_forward_f16", b, heads, n, n_valid, ptr(qkv),
         ptr(out), stream_ptr())
    return out


def _r16(t):
    """the fp16 rounding of a matrix operand, kept in fp32 (the CPU restatement of the fp16 mode)"""
    return t.half().float()


class _LayerScale(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.gamma = nn.Parameter(torch.ones(dim))


class _Attention(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)


class _Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)


class _Block(nn.Module):
    def __init__(self, dim, hidden, eps):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=eps)
        self.attn = _Attention(dim)
        self.ls1 = _LayerScale(dim)
        self.norm2 = nn.LayerNorm(dim, eps=eps)
        self.mlp = _Mlp(dim, hidden)
        self.ls2 = _LayerScale(dim)


class _PatchEmbed(nn.Module):
    def __init__(self, dim, patch):
        super().__init__()
        self.proj = nn.Conv2d(3, dim, kernel_size=patch, stride=patch)


class DinoV2(nn.Module):
    """DINOv2 ViT with an MLP block. Parameter names and shapes are those of the published hub checkpoints
    (dinov2_vit{s,b,l}14_pretrain.pth): cls_token [1,1,C], pos_embed [1,1+grid^2,C], mask_token [1,C] (held, unused),
    patch_embed.proj, blocks.{i}.{norm1, attn.qkv (rows (q|k|v) x heads x 64), attn.proj, ls1.gamma, norm2, mlp.fc1, mlp.fc2,
    ls2.gamma}, norm. Inference only. precision: "fp32" (default) or "fp16" (module docstring, "Arithmetic")."""

    HALF_WEIGHTS = ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2")  # the matrix operands of a block

    def __init__(self, embed_dim=384, depth=12, num_heads=6, mlp_ratio=4, patch_size=14, grid=37, layer_norm_eps=1e-6,
                 interpolate_offset=0.1, ffn_layer="mlp", num_register_tokens=0, precision="fp32"):
        super().__init__()
        if precision not in ("fp32", "fp16"):
            raise ValueError(f"DinoV2: precision {precision!r} is not 'fp32' or 'fp16'")
        self.precision = precision
        if ffn_layer != "mlp":
            raise ValueError(f"DinoV2: ffn_layer {ffn_layer!r} is not supported (the SwiGLU block of vitg14); only 'mlp'")
        if num_register_tokens != 0:
            raise ValueError("DinoV2: register tokens (the *_reg checkpoints) are not supported")
        if embed_dim != num_heads * HEAD_DIM:
            raise ValueError(f"DinoV2: embed_dim {embed_dim} / num_heads {num_heads} is not the head dimension {HEAD_DIM} of "
                             "the DINOv2 models (csrc/vit.hip attends over 64-wide heads)")
        if patch_size % 2 or patch_size < 2:
            raise ValueError(f"DinoV2: patch_size {patch_size} must be even")
        self.embed_dim, self.depth, self.num_heads = int(embed_dim), int(depth), int(num_heads)
        self.patch_size, self.grid, self.eps = int(patch_size), int(grid), float(layer_norm_eps)
        self.interpolate_offset = float(interpolate_offset)
        c = self.embed_dim
        if precision == "fp16" and int(c * mlp_ratio) % 64:
            raise ValueError(f"DinoV2: precision='fp16' needs an MLP width that is a multiple of 64, not {int(c * mlp_ratio)} "
                             "(csrc/vit_f16.hip tiles the output channels by 64)")
        self.cls_token = nn.Parameter(torch.zeros(1, 1, c))
        self.pos_embed = nn.Parameter(torch.zeros(1, 1 + self.grid ** 2, c))
        self.mask_token = nn.Parameter(torch.zeros(1, c))
        self.patch_embed = _PatchEmbed(c, self.patch_size)
        self.blocks = nn.ModuleList(_Block(c, int(c * mlp_ratio), self.eps) for _ in range(self.depth))
        self.norm = nn.LayerNorm(c, eps=self.eps)
        self._pos_cache = {}
        self._half_cache = None
        self.requires_grad_(False)
        self.eval()

    # ---- weights --------------------------------------------------------------------------------------------------------
    @classmethod
    def from_transformers_state_dict(cls, sd, **config):
        """A model from the state dict of `transformers.Dinov2Model` (with or without a leading "dinov2."): the config is
        read from the shapes unless given; query / key / value are concatenated to attn.qkv."""
        sd = {(k[len("dinov2."):] if k.startswith("dinov2.") else k): v for k, v in sd.items()}
        if any("register_tokens" in k for k in sd):
            raise ValueError("DinoV2: register tokens are not supported")
        if any(".mlp.weights_in." in k for k in sd):
            raise ValueError("DinoV2: the SwiGLU block (mlp.weights_in) is not supported")
        w = sd["embeddings.patch_embeddings.projection.weight"]
        c = w.shape[0]
        depth = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.layer."))
        cfg = dict(embed_dim=c, depth=depth, num_heads=c // HEAD_DIM, patch_size=w.shape[-1],
                   mlp_ratio=sd["encoder.layer.0.mlp.fc1.weight"].shape[0] / c,
                   grid=int(round(math.sqrt(sd["embeddings.position_embeddings"].shape[1] - 1))), interpolate_offset=0.0)
        cfg.update(config)
        model = cls(**cfg)
        out = {"cls_token": sd["embeddings.cls_token"], "mask_token": sd["embeddings.mask_token"],
               "pos_embed": sd["embeddings.position_embeddings"],
               "patch_embed.proj.weight": w, "patch_embed.proj.bias": sd["embeddings.patch_embeddings.projection.bias"],
               "norm.weight": sd["layernorm.weight"], "norm.bias": sd["layernorm.bias"]}
        for i in range(depth):
            src, dst = f"encoder.layer.{i}.", f"blocks.{i}."
            for p in ("weight", "bias"):
                out[f"{dst}norm1.{p}"], out[f"{dst}norm2.{p}"] = sd[f"{src}norm1.{p}"], sd[f"{src}norm2.{p}"]
                out[f"{dst}attn.qkv.{p}"] = torch.cat([sd[f"{src}attention.attention.{n}.{p}"] for n in ("query", "key", "value")])
                out[f"{dst}attn.proj.{p}"] = sd[f"{src}attention.output.dense.{p}"]
                out[f"{dst}mlp.fc1.{p}"], out[f"{dst}mlp.fc2.{p}"] = sd[f"{src}mlp.fc1.{p}"], sd[f"{src}mlp.fc2.{p}"]
            out[f"{dst}ls1.gamma"], out[f"{dst}ls2.gamma"] = sd[f"{src}layer_scale1.lambda1"], sd[f"{src}layer_scale2.lambda1"]
        model.load_state_dict({k: torch.as_tensor(v).to(F32) for k, v in out.items()}, strict=True)
        return model

    def load_state_dict(self, *args, **kwargs):
        self._pos_cache = {}
        self._half_cache = None
        return super().load_state_dict(*args, **kwargs)

    def _apply(self, *args, **kwargs):
        self._half_cache = None  # .to() / .cuda() / .float(): the fp16 weights follow the parameters
        return super()._apply(*args, **kwargs)

    def half_weights(self):
        """{"blocks.{i}.{attn.qkv | attn.proj | mlp.fc1 | mlp.fc2}": the weight's `.half()`}: the matrix operands of the fp16
        mode, made once per model on the parameters' device and kept until `load_state_dict` or `_apply`"""
        if self._half_cache is None:
            self._half_cache = {f"blocks.{i}.{name}": blk.get_submodule(name).weight.detach().half().contiguous()
                                for i, blk in enumerate(self.blocks) for name in self.HALF_WEIGHTS}
        return self._half_cache

    # ---- position embedding -----------------------------------------------------------------------------------------------
    def pos_table(self, h, w, device=None):
        """f32[1 + h*w, C]: the position embedding for an h x w patch grid (module docstring), interpolated on the host in fp32
        and cached per (h, w, device)"""
        device = self.pos_embed.device if device is None else torch.device(device)
        key = (int(h), int(w), str(device))
        if key not in self._pos_cache:
            pos = self.pos_embed.detach()[0].to("cpu", F32)
            if not (h == self.grid and w == self.grid):
                g, c = self.grid, self.embed_dim
                patch = pos[1:].reshape(1, g, g, c).permute(0, 3, 1, 2)
                if self.interpolate_offset > 0:
                    o = self.interpolate_offset
                    patch = F.interpolate(patch, scale_factor=((h + o) / g, (w + o) / g), mode="bicubic", antialias=False)
                else:
                    patch = F.interpolate(patch, size=(h, w), mode="bicubic", antialias=False)
                if tuple(patch.shape[-2:]) != (h, w):
                    raise RuntimeError(f"DinoV2: the position table came out {tuple(patch.shape[-2:])}, not {(h, w)}")
                pos = torch.cat([pos[:1], patch.permute(0, 2, 3, 1).reshape(h * w, c)])
            self._pos_cache[key] = pos.contiguous().to(device)
        return self._pos_cache[key]

    # ---- forward --------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward_features(self, x):
        """x f32 | f16 [B,3,H,W] (normalised; H, W multiples of the patch size) ->
        {"x_norm_clstoken": f32[B,C], "x_norm_patchtokens": f32[B, h*w, C]}, patch tokens row-major over (h, w)"""
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"forward_features: x must be [B,3,H,W], got {list(x.shape)}")
        if x.dtype not in (F32, F16):
            raise RuntimeError("forward_features: x must be float32 or float16")
        ps = self.patch_size
        if x.shape[2] % ps or x.shape[3] % ps or x.shape[2] < ps or x.shape[3] < ps or x.shape[0] < 1:
            raise ValueError(f"forward_features: H, W = {tuple(x.shape[2:])} must be positive multiples of {ps}")
        if x.device != self.pos_embed.device:
            raise RuntimeError(f"forward_features: x is on {x.device}, the model on {self.pos_embed.device}")
        x = x.to(F32).contiguous()
        tok = self._tokens_hip(x) if x.is_cuda else self._tokens_torch(x)
        return {"x_norm_clstoken": tok[:, 0], "x_norm_patchtokens": tok[:, 1:]}

    def _tokens_torch(self, x, hidden_states=None):
        if self.precision == "fp16":
            return self._tokens_torch_half(x, hidden_states)
        b, c, ps = x.shape[0], self.embed_dim, self.patch_size
        hp, wp = x.shape[2] // ps, x.shape[3] // ps
        p = self.patch_embed.proj
        t = F.conv2d(x, p.weight, p.bias, stride=ps).flatten(2).transpose(1, 2)
        t = torch.cat([self.cls_token.expand(b, -1, -1), t], 1) + self.pos_table(hp, wp, x.device)
        n = t.shape[1]
        if hidden_states is not None:
            hidden_states.append(t)
        for blk in self.blocks:
            y = F.layer_norm(t, (c,), blk.norm1.weight, blk.norm1.bias, self.eps)
            q, k, v = F.linear(y, blk.attn.qkv.weight, blk.attn.qkv.bias).view(b, n, 3, self.num_heads, HEAD_DIM).unbind(2)
            a = torch.softmax((q * HEAD_DIM ** -0.5).transpose(1, 2) @ k.permute(0, 2, 3, 1), -1) @ v.transpose(1, 2)
            a = a.transpose(1, 2).reshape(b, n, c)
            t = t + blk.ls1.gamma * F.linear(a, blk.attn.proj.weight, blk.attn.proj.bias)
            y = F.layer_norm(t, (c,), blk.norm2.weight, blk.norm2.bias, self.eps)
            y = F.gelu(F.linear(y, blk.mlp.fc1.weight, blk.mlp.fc1.bias))
            t = t + blk.ls2.gamma * F.linear(y, blk.mlp.fc2.weight, blk.mlp.fc2.bias)
            if hidden_states is not None:
                hidden_states.append(t)
        return F.layer_norm(t, (c,), self.norm.weight, self.norm.bias, self.eps)

    def _tokens_torch_half(self, x, hidden_states=None):
        """the fp16 mode restated in torch: every matrix operand through .half().float(), products and the rest in fp32"""
        b, c, ps = x.shape[0], self.embed_dim, self.patch_size
        hp, wp = x.shape[2] // ps, x.shape[3] // ps
        p = self.patch_embed.proj
        t = F.conv2d(x, p.weight, p.bias, stride=ps).flatten(2).transpose(1, 2)
        t = torch.cat([self.cls_token.expand(b, -1, -1), t], 1) + self.pos_table(hp, wp, x.device)
        n = t.shape[1]
        w16 = {k: v.float() for k, v in self.half_weights().items()}
        if hidden_states is not None:
            hidden_states.append(t)
        for i, blk in enumerate(self.blocks):
            y = _r16(F.layer_norm(t, (c,), blk.norm1.weight, blk.norm1.bias, self.eps))
            qkv = _r16(F.linear(y, w16[f"blocks.{i}.attn.qkv"], blk.attn.qkv.bias))
            q, k, v = qkv.view(b, n, 3, self.num_heads, HEAD_DIM).unbind(2)
            prob = torch.softmax((q * HEAD_DIM ** -0.5).transpose(1, 2) @ k.permute(0, 2, 3, 1), -1)
            a = _r16((_r16(prob) @ v.transpose(1, 2)).transpose(1, 2).reshape(b, n, c))
            t = t + blk.ls1.gamma * F.linear(a, w16[f"blocks.{i}.attn.proj"], blk.attn.proj.bias)
            y = _r16(F.layer_norm(t, (c,), blk.norm2.weight, blk.norm2.bias, self.eps))
            y = _r16(F.gelu(F.linear(y, w16[f"blocks.{i}.mlp.fc1"], blk.mlp.fc1.bias)))
            t = t + blk.ls2.gamma * F.linear(y, w16[f"blocks.{i}.mlp.fc2"], blk.mlp.fc2.bias)
            if hidden_states is not None:
                hidden_states.append(t)
        return F.layer_norm(t, (c,), self.norm.weight, self.norm.bias, self.eps)

    def _tokens_hip(self, x, hidden_states=None):
        dev = x.device
        b, c, ps = x.shape[0], self.embed_dim, self.patch_size
        hp, wp = x.shape[2] // ps, x.shape[3] // ps
        n = 1 + hp * wp
        rows = b * n
        if hp * wp > 65535 or rows * 4 * c >= 2 ** 31:
            raise ValueError(f"forward_features: {b} images of {hp} x {wp} patches are out of range")
        for prm in self.parameters():
            if prm.dtype != F32 or not prm.is_contiguous():
                raise RuntimeError("DinoV2: parameters must be contiguous float32 (precision='fp16' rounds the matrix "
                                   "operands itself)")
        pos = self.pos_table(hp, wp, dev)
        ws = torch.empty(int(ask("p2pb_vit_patch_embed_ws_floats", b, hp, wp, ps)), dtype=F32, device=dev)
        half = self.precision == "fp16"
        act = F16 if half else F32  # the operands of the matrix products: norm outputs, qkv, attention output, hidden
        if half:
            w16 = self.half_weights()
            if w16 and next(iter(w16.values())).device != dev:
                raise RuntimeError("DinoV2: the cached fp16 weights are not on the model's device")
        t = torch.empty(b, n, c, dtype=F32, device=dev)
        y = torch.empty(rows, c, dtype=act, device=dev)
        qkv = torch.empty(rows, 3 * c, dtype=act, device=dev)
        hid = torch.empty(rows, self.blocks[0].mlp.fc1.weight.shape[0], dtype=act, device=dev) if self.depth else None
        s = stream_ptr()
        p = self.patch_embed.proj
        call("p2pb_vit_patch_embed", b, hp, wp, ps, c, ptr(x), ptr(p.weight), ptr(p.bias),
             ptr(self.cls_token), ptr(pos), ptr(ws), ptr(t), s)

        def norm(src, ln, dst):
            call("p2pb_vit_layernorm_f16" if dst.dtype == F16 else "p2pb_vit_layernorm", rows, c, ptr(src),
                 ptr(ln.weight), ptr(ln.bias), self.eps, ptr(dst), s)

        matmul = "p2pb_vit_linear_f16" if half else "p2pb_vit_linear"
        attend = "p2pb_vit_attention_forward_f16" if half else "p2pb_vit_attention_forward"

        def linear(src, lin, weight, epi, gamma, dst):
            call(matmul, rows, weight.shape[0], weight.shape[1], ptr(src), ptr(weight), ptr(lin.bias), epi,
                 ptr(gamma), ptr(dst), s)

        if hidden_states is not None:
            hidden_states.append(t.clone())
        for i, blk in enumerate(self.blocks):
            attn, mlp = blk.attn, blk.mlp
            if half:
                wq, wp, w1, w2 = (w16[f"blocks.{i}.{name}"] for name in self.HALF_WEIGHTS)
            else:
                wq, wp, w1, w2 = attn.qkv.weight, attn.proj.weight, mlp.fc1.weight, mlp.fc2.weight
            norm(t, blk.norm1, y)
            linear(y, attn.qkv, wq, EPI_BIAS, None, qkv)
            call(attend, b, self.num_heads, n, n, ptr(qkv), ptr(y), s)
            linear(y, attn.proj, wp, EPI_RESIDUAL, blk.ls1.gamma, t)
            norm(t, blk.norm2, y)
            linear(y, mlp.fc1, w1, EPI_GELU, None, hid)
            linear(hid, mlp.fc2, w2, EPI_RESIDUAL, blk.ls2.gamma, t)
            if hidden_states is not None:
                hidden_states.append(t.clone())
        out = torch.empty(b, n, c, dtype=F32, device=dev)
        norm(t, self.norm, out)
        return out

    @torch.no_grad()
    def hidden_states(self, x):
        """([the embeddings, then the residual stream after every block], the normalised tokens), f32[B,T,C] each (for tests: a
        failure names its layer)"""
        hs = []
        x = x.to(F32).contiguous()
        out = (self._tokens_hip if x.is_cuda else self._tokens_torch)(x, hs)
        return hs, out


def create(name, **kwargs):
    """a preset by its hub name; vitg14 and the *_reg variants raise ValueError"""
    if name.endswith("_reg") or "_reg" in name:
        raise ValueError(f"{name}: register tokens are not supported")
    if name.startswith("dinov2_vitg14"):
        raise ValueError(f"{name}: the SwiGLU block of the giant model is not supported")
    if name not in PRESETS:
        raise ValueError(f"{name}: not one of {sorted(PRESETS)}")
    return DinoV2(**{**PRESETS[name], **kwargs})


def dinov2_vits14(**kwargs):
    return create("dinov2_vits14", **kwargs)


def dinov2_vitb14(**kwargs):
    return create("dinov2_vitb14", **kwargs)


def dinov2_vitl14(**kwargs):
    return create("dinov2_vitl14", **kwargs)


# ---- the reference's wrapper ---------------------------------------------------------------------------------------------
def normalize(image):
    """(image - mean) / std with the ImageNet constants, in fp32 (make_transform, :36-55; its Resize to the image's own
    smaller edge is the identity)"""
    mean = torch.tensor(IMAGENET_DEFAULT_MEAN, dtype=F32, device=image.device).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_DEFAULT_STD, dtype=F32, device=image.device).view(1, 3, 1, 1)
    return (image.to(F32) - mean) / std


def _patch_grid(model, image, patch_size):
    """image [B,3,H,W] in [0,1] -> the patch tokens rounded to fp16 once, f16[B,h,w,C] channel-last"""
    if patch_size != model.patch_size:
        raise ValueError(f"patch_size {patch_size} is not the model's {model.patch_size}")
    b, _, h, w = image.shape
    x = normalize(image)[:, :, :h - h % patch_size, :w - w % patch_size]  # (:76-81)
    t = model.forward_features(x)["x_norm_patchtokens"].half()
    return t.reshape(b, x.shape[2] // patch_size, x.shape[3] // patch_size, -1)


@torch.no_grad()
def get_dino_features(model, image, patch_size=14):
    """:88-111. image f32 | f16 [B,3,H,W] in [0,1] -> f16[B,C,H,W]: the patch tokens, bilinearly upsampled to the image"""
    feat = _patch_grid(model, image, patch_size).permute(0, 3, 1, 2)
    return F.interpolate(feat, size=tuple(image.shape[2:]), mode="bilinear", antialias=False)


def feature_fn(model, patch_size=14):
    """the `feature_fn` of image_features.fuse_scene: images f16[B,3,H,W] in [0,1] -> the fp16 patch grid f16[B,C,h,w] (a view
    of the channel-last tokens: `dino_from_grid=True` reads it without a copy)"""
    def fn(images):
        return _patch_grid(model, images, patch_size).permute(0, 3, 1, 2)
    return fn
