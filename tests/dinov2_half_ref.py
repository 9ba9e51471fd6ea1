"""The yardstick of DinoV2(precision="fp16"): the mode's contract written in plain torch on the CPU (a helper module, not a
conftest). It shares no code with p2p_bridge_amd/dinov2.py; LayerNorm, GELU, softmax and the weight names come from dinov2_ref.

The contract: only the OPERANDS of the matrix products are fp16, each rounded once to nearest-even (`.half()`, IEEE: beyond
+-65504 it is +-inf) -- the outputs of norm1 and norm2, the qkv rows, the softmax weights entering P.V, the attention output,
the post-GELU activations and the weights of attn.qkv, attn.proj, mlp.fc1 and mlp.fc2. The residual stream, LayerNorm
statistics, softmax, bias, GELU, LayerScale and the accumulation of every product are fp32; patch embedding and the final norm
are the fp32 forward's.

A gate is GATE_FACTOR (4, dinov2_ref) x the error of THIS restatement against float64 on the same inputs, for the model and for
a single operator alike: never the code under test. An independent evaluation of the same contract (float64 accumulation,
un-normalised softmax weights) stays within 1.52 x this restatement's error on the worst layer of the golden cases, the range
case and ViT-S at 2 x 182 x 252, so 4 x has room and still fails on any indexing error.
"""
import math

import torch

import dinov2_ref as R

F32, F64 = torch.float32, torch.float64
GATE_FACTOR = R.GATE_FACTOR
HEAD_DIM = R.HEAD_DIM


def r16(t):
    """one fp16 rounding of a matrix operand, the value kept in fp32"""
    return t.to(torch.float16).to(F32)


def linear_half(x16, w16, bias, gelu=False):
    """the linear operator's contract: fp16 operands (given as fp16 numbers in any dtype), fp32 sum + bias (+ GELU) -> fp32, NOT
    yet rounded to the output's fp16"""
    y = x16.to(F32) @ w16.to(F32).t() + bias.to(F32)
    return R.gelu(y) if gelu else y


def attention_half(qkv16, heads):
    """qkv [B, n, 3*heads*64] of fp16 numbers -> the attention output in fp32 BEFORE its rounding to fp16: fp32 logits and
    softmax, the normalised weights rounded to fp16 where they enter P.V"""
    b, n, _ = qkv16.shape
    q, k, v = qkv16.to(F32).reshape(b, n, 3, heads, HEAD_DIM).permute(2, 0, 3, 1, 4)
    s = (q * HEAD_DIM ** -0.5) @ k.transpose(-1, -2)
    s = s - s.amax(-1, keepdim=True)
    p = torch.exp(s)
    p = p / p.sum(-1, keepdim=True)
    return (r16(p) @ v).transpose(1, 2).reshape(b, n, heads * HEAD_DIM)


def forward_half(sd, x, patch_size=14, eps=1e-6, offset=0.0):
    """sd: weights under the hub names, x [B,3,H,W] -> (hidden states: the embeddings, then the stream after each block;
    normalised tokens [B, T, C]), fp32"""
    sd = {k: v.to(F32) for k, v in sd.items()}
    x = x.to(F32)
    b, _, hh, ww = x.shape
    h, w = hh // patch_size, ww // patch_size
    wt = sd["patch_embed.proj.weight"]
    c = wt.shape[0]
    heads = c // HEAD_DIM
    grid = int(round(math.sqrt(sd["pos_embed"].shape[1] - 1)))
    patches = x.reshape(b, 3, h, patch_size, w, patch_size).permute(0, 2, 4, 1, 3, 5).reshape(b, h * w, -1)
    t = patches @ wt.reshape(c, -1).t() + sd["patch_embed.proj.bias"]  # fp32: the patch projection is not part of the mode
    t = torch.cat([sd["cls_token"].expand(b, -1, -1), t], 1) + R.pos_table(sd["pos_embed"], grid, h, w, offset)
    n = t.shape[1]
    hidden = [t]
    i = 0
    while f"blocks.{i}.norm1.weight" in sd:
        p = f"blocks.{i}."
        y = r16(R.layer_norm(t, sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps))
        qkv = r16(linear_half(y, r16(sd[p + "attn.qkv.weight"]), sd[p + "attn.qkv.bias"]))
        a = r16(attention_half(qkv, heads))
        t = t + sd[p + "ls1.gamma"] * linear_half(a, r16(sd[p + "attn.proj.weight"]), sd[p + "attn.proj.bias"])
        y = r16(R.layer_norm(t, sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps))
        y = r16(linear_half(y, r16(sd[p + "mlp.fc1.weight"]), sd[p + "mlp.fc1.bias"], gelu=True))
        t = t + sd[p + "ls2.gamma"] * linear_half(y, r16(sd[p + "mlp.fc2.weight"]), sd[p + "mlp.fc2.bias"])
        hidden.append(t)
        i += 1
    return hidden, R.layer_norm(t, sd["norm.weight"], sd["norm.bias"], eps)


def gate_half(sd, x, **kw):
    """(float64 hidden states, float64 tokens, per-layer gates, token gate): a gate is GATE_FACTOR x max |forward_half - float64|"""
    h64, t64 = R.forward(sd, x, dtype=F64, **kw)
    h16, t16 = forward_half(sd, x, **kw)
    gates = [GATE_FACTOR * float((a.double() - b).abs().max()) for a, b in zip(h16, h64)]
    return h64, t64, gates, GATE_FACTOR * float((t16.double() - t64).abs().max())
