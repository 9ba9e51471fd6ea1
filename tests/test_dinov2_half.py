"""DinoV2(precision="fp16") on its CPU path (no GPU): the keyword, the torch restatement of the mode against the yardstick of
tests/dinov2_half_ref.py, the untouched fp32 mode and the cache of fp16 weights."""
import pytest
import torch

import dinov2_half_ref as H
import dinov2_ref as R


@pytest.fixture(scope="module")
def dinov2():
    from p2p_bridge_amd import dinov2 as d

    return d


@pytest.fixture(scope="module")
def gold():
    tsd, cases, _ = R.load_golden()
    return {"tsd": tsd, "hub": R.hub_from_transformers(tsd), "cases": cases}


def test_precision_keyword(dinov2, gold):
    assert dinov2.DinoV2(embed_dim=128, depth=1, num_heads=2, grid=5).precision == "fp32"
    assert dinov2.DinoV2(embed_dim=128, depth=1, num_heads=2, grid=5, precision="fp16").precision == "fp16"
    for bad in ("bf16", "half", "FP16", None, 16):
        with pytest.raises(ValueError):
            dinov2.DinoV2(embed_dim=128, depth=1, num_heads=2, grid=5, precision=bad)
    with pytest.raises(ValueError):  # an MLP width the 64-channel tiles of the fp16 kernels cannot take
        dinov2.DinoV2(embed_dim=128, depth=1, num_heads=2, grid=5, mlp_ratio=0.75, precision="fp16")
    assert dinov2.DinoV2(embed_dim=128, depth=1, num_heads=2, grid=5, mlp_ratio=0.75).precision == "fp32"
    assert dinov2.create("dinov2_vits14", depth=1, precision="fp16").precision == "fp16"
    for preset in (dinov2.dinov2_vits14, dinov2.dinov2_vitb14, dinov2.dinov2_vitl14):
        assert preset(depth=1, precision="fp16").precision == "fp16" and preset(depth=1).precision == "fp32"
    with pytest.raises(ValueError):
        dinov2.dinov2_vits14(depth=1, precision="bf16")
    assert dinov2.DinoV2.from_transformers_state_dict(gold["tsd"], precision="fp16").precision == "fp16"
    assert dinov2.DinoV2.from_transformers_state_dict(gold["tsd"]).precision == "fp32"


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_cpu_fp16_mode_inside_the_half_gate(dinov2, gold, name):
    x = gold["cases"][name]["x"]
    model = dinov2.DinoV2.from_transformers_state_dict(gold["tsd"], precision="fp16")
    h64, t64, gates, gate = H.gate_half(gold["hub"], x)
    hs, tokens = model.hidden_states(x)
    assert len(hs) == len(h64) == 3
    for i, (a, b, g) in enumerate(zip(hs, h64, gates)):
        err = float((a.double() - b).abs().max())
        print(f"case {name} hidden {i}: err {err:.3e} gate {g:.3e}")
        assert torch.isfinite(a).all() and err <= g, (i, err, g)
    err = float((tokens.double() - t64).abs().max())
    print(f"case {name} tokens: err {err:.3e} gate {gate:.3e}")
    assert tokens.dtype == torch.float32 and err <= gate
    out = model.forward_features(x)
    assert out["x_norm_patchtokens"].dtype == torch.float32
    assert torch.equal(out["x_norm_clstoken"], tokens[:, 0]) and torch.equal(out["x_norm_patchtokens"], tokens[:, 1:])
    # a CPU model in fp16 mode does not silently run fp32: the bits differ, by about the yardstick's own distance from fp32
    plain = dinov2.DinoV2.from_transformers_state_dict(gold["tsd"]).hidden_states(x)[1]
    assert not torch.equal(tokens, plain)
    assert float((tokens - plain).abs().max()) > 1e-5


@pytest.mark.parametrize("name", ["a", "c"])
def test_fp32_mode_is_unchanged_by_the_keyword(dinov2, gold, name):
    x = gold["cases"][name]["x"]
    without = dinov2.DinoV2.from_transformers_state_dict(gold["tsd"])
    given = dinov2.DinoV2.from_transformers_state_dict(gold["tsd"], precision="fp32")
    (ha, ta), (hb, tb) = without.hidden_states(x), given.hidden_states(x)
    assert torch.equal(ta, tb) and all(torch.equal(a, b) for a, b in zip(ha, hb))
    assert given._half_cache is None  # the fp32 mode makes no fp16 copies


def test_half_weights_follow_the_parameters(dinov2, gold):
    x = gold["cases"]["c"]["x"]
    model = dinov2.DinoV2.from_transformers_state_dict(gold["tsd"], precision="fp16")
    first = model.hidden_states(x)[1]
    cache = model.half_weights()
    assert sorted(cache) == sorted(f"blocks.{i}.{n}" for i in range(2) for n in ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2"))
    assert all(v.dtype == torch.float16 for v in cache.values()) and model.half_weights() is cache
    assert torch.equal(cache["blocks.1.mlp.fc2"], model.blocks[1].mlp.fc2.weight.half())
    other = {k: v.clone() for k, v in model.state_dict().items()}
    for k in other:
        if k.endswith("qkv.weight") or k.endswith("fc1.weight"):
            other[k] = (other[k] * 1.25).half().float()
    model.load_state_dict(other, strict=True)
    assert model._half_cache is None
    fresh = dinov2.DinoV2(embed_dim=128, depth=2, num_heads=2, grid=5, interpolate_offset=0.0, precision="fp16")
    fresh.load_state_dict(other, strict=True)
    again = model.hidden_states(x)[1]
    assert torch.equal(again, fresh.hidden_states(x)[1]) and not torch.equal(again, first)
    model.half_weights()
    model.to(torch.float32)  # _apply: the copies are dropped with whatever moved the parameters
    assert model._half_cache is None
