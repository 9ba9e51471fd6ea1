"""Fixtures of p2p_bridge_amd/dinov2.py under tests/golden/, computed by an independent implementation:
`transformers.models.dinov2.Dinov2Model` in float64 on the CPU, built from a config with seeded random weights (no download).
Build container only; nothing that runs on a GPU machine imports `transformers`.

    python tools/make_golden_dinov2.py

Model: Dinov2Config(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, mlp_ratio=4, patch_size=14, image_size=70,
layerscale_value=1.0, qkv_bias=True, layer_norm_eps=1e-6, hidden_act="gelu", use_swiglu_ffn=False): two 64-wide heads, a 5 x 5
position table.

Weights: tests/dinov2_ref.py `random_weights` (seed 1234), stored rounded to fp16 and upcast on both sides. The library's own
initialisation (std 0.02) gives near-uniform softmax rows and residual branches too small to see, under which a wrong attention
scale or a missing LayerScale passes; so this tool ASSERTS, on case a, in every layer: standard deviation of the attention
logits along a row >= 1, and RMS of each residual branch after LayerScale >= 0.25 of the stream's RMS. Both figures are stored.

  dinov2_tiny.npz            w.<transformers name>  f16   the weights
                             logit_row_std, logit_abs_max, branch_rms_ratio   f64[layers] / [layers] / [layers, 2]
  dinov2_tiny_case_a.npz     2 x 3 x 182 x 252: 13 x 18 tokens, the table interpolated to a non-square grid
  dinov2_tiny_case_b.npz     1 x 3 x 70 x 70: the native grid, no interpolation
  dinov2_tiny_case_c.npz     1 x 3 x 14 x 14: one patch, T = 2
      x_u8 u8[B,3,H,W] (the model input is (x_u8 - 128) / 64), last_hidden_state f64[B,T,C], hidden_states f64[L+1,...]: the
      embeddings and the stream after every layer -- whole for b and c, image 1 at every 5th token for a (dinov2_ref.HIDDEN_ROWS)

Four files, not one: no committed file may exceed 1 MiB and the fp16 weights alone are 0.95 MB. The archives are written with
fixed member dates, so a rerun on the same software reproduces them byte for byte.
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dinov2_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SEED = 1234
LIMIT = 1 << 20


def save_npz(path, arrays):
    """np.savez with fixed member dates and order (np.savez stamps the members with the current time)"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    size = os.path.getsize(path)
    assert size <= LIMIT, (path, size)
    print(f"{os.path.relpath(path, ROOT)}: {size} bytes")


def figures(sd, x):
    """(row std of the attention logits, max |logit|, RMS(branch) / RMS(stream) for both branches) per layer, float64, from a
    replay of the forward with the primitives of tests/dinov2_ref.py"""
    sd = {k: v.double() for k, v in sd.items()}
    hidden, _ = R.forward(sd, x)
    c = sd["norm.weight"].shape[0]
    heads = c // R.HEAD_DIM
    rows, peak, ratio = [], [], []
    for i, t in enumerate(hidden[:-1]):
        p = f"blocks.{i}."
        b, n = t.shape[:2]
        y = R.layer_norm(t, sd[p + "norm1.weight"], sd[p + "norm1.bias"], 1e-6)
        qkv = (y @ sd[p + "attn.qkv.weight"].t() + sd[p + "attn.qkv.bias"]).reshape(b, n, 3, heads, R.HEAD_DIM).permute(2, 0, 3, 1, 4)
        logits = (qkv[0] * R.HEAD_DIM ** -0.5) @ qkv[1].transpose(-1, -2)
        rows.append(float(logits.std(-1).mean()))
        peak.append(float(logits.abs().max()))
        a = R.attention(qkv[0], qkv[1], qkv[2]).transpose(1, 2).reshape(b, n, c)
        br1 = sd[p + "ls1.gamma"] * (a @ sd[p + "attn.proj.weight"].t() + sd[p + "attn.proj.bias"])
        t1 = t + br1
        y = R.gelu(R.layer_norm(t1, sd[p + "norm2.weight"], sd[p + "norm2.bias"], 1e-6) @ sd[p + "mlp.fc1.weight"].t()
                   + sd[p + "mlp.fc1.bias"])
        br2 = sd[p + "ls2.gamma"] * (y @ sd[p + "mlp.fc2.weight"].t() + sd[p + "mlp.fc2.bias"])
        rms = lambda v: float(v.pow(2).mean().sqrt())  # noqa: E731
        ratio.append([rms(br1) / rms(t), rms(br2) / rms(t1)])
    return np.array(rows), np.array(peak), np.array(ratio)


def main():
    from transformers.models.dinov2 import Dinov2Config, Dinov2Model

    torch.set_num_threads(1)  # (one summation order)
    cfg = Dinov2Config(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, mlp_ratio=4, patch_size=14, image_size=70,
                       layerscale_value=1.0, qkv_bias=True, layer_norm_eps=1e-6, hidden_act="gelu", use_swiglu_ffn=False,
                       attn_implementation="eager")
    hub = R.random_weights(128, 2, 5, SEED)
    tsd = R.transformers_from_hub(hub)
    model = Dinov2Model(cfg).double().eval()
    missing = model.load_state_dict({k: v.double() for k, v in tsd.items()}, strict=True)
    print("load_state_dict:", missing)

    g = torch.Generator().manual_seed(SEED + 1)
    xs = {name: torch.randint(0, 256, (b, 3, h, w), generator=g, dtype=torch.uint8) for name, (b, h, w) in R.CASES.items()}

    row_std, peak, ratio = figures(hub, R.image_from_u8(xs["a"]))
    print("attention-logit row std per layer:", row_std, " max |logit|:", peak)
    print("RMS(branch) / RMS(stream) per layer (attention, MLP):", ratio.tolist())
    assert (row_std >= 1.0).all(), row_std
    assert (ratio >= 0.25).all(), ratio
    arrays = {"w." + k: v.half().numpy() for k, v in tsd.items()}
    for k, v in tsd.items():
        assert torch.equal(v.half().float(), v), k  # (the recipe rounds to fp16: nothing is lost here)
    arrays.update(logit_row_std=row_std, logit_abs_max=peak, branch_rms_ratio=ratio)
    save_npz(os.path.join(OUT, "dinov2_tiny.npz"), arrays)

    for name, x8 in xs.items():
        with torch.no_grad():
            out = model(pixel_values=R.image_from_u8(x8).double(), output_hidden_states=True)
        hidden = torch.stack(list(out.hidden_states))  # [L+1, B, T, C]
        if name == "a":
            hidden = hidden[:, 1, R.HIDDEN_ROWS]
        print(f"case {name}: x {tuple(x8.shape)}, last_hidden_state {tuple(out.last_hidden_state.shape)}, "
              f"RMS {float(out.last_hidden_state.pow(2).mean().sqrt()):.3f}")
        save_npz(os.path.join(OUT, f"dinov2_tiny_case_{name}.npz"),
                 {"x_u8": x8.numpy(), "last_hidden_state": out.last_hidden_state.numpy(), "hidden_states": hidden.numpy()})


if __name__ == "__main__":
    main()
