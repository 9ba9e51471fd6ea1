"""p2p_bridge_amd.dinov2 and the token-grid sampling of p2p_bridge_amd.image_features on their CPU paths (no GPU).

The yardstick of the model is tests/golden/dinov2_tiny*.npz: `transformers.Dinov2Model` in float64 with seeded weights
(tools/make_golden_dinov2.py), under which tests/dinov2_ref.py (float64) is first pinned at rtol 1e-9 -- two float64
evaluations of the same sums -- and then serves as the reference everywhere else. The fp32 gate is 4 x the error of
dinov2_ref run in fp32 against its own float64 run on the same case: torch's fp32, never the code under test.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dinov2_ref as R

HUB_NAMES = ["cls_token", "pos_embed", "mask_token", "patch_embed.proj.weight", "patch_embed.proj.bias"]
BLOCK_NAMES = ["norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias", "ls1.gamma",
               "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias", "ls2.gamma"]


@pytest.fixture(scope="module")
def gold():
    tsd, cases, figures = R.load_golden()
    return {"tsd": tsd, "hub": R.hub_from_transformers(tsd), "cases": cases, "figures": figures}


@pytest.fixture(scope="module")
def model(gold):
    from p2p_bridge_amd import dinov2

    return dinov2.DinoV2.from_transformers_state_dict(gold["tsd"])


def stored_hidden(name, hidden):
    """the part of a hidden-state stack [L+1, B, T, C] that the fixture of this case stores"""
    return hidden[:, 1, R.HIDDEN_ROWS] if name == "a" else hidden


def test_fixture_conditions(gold):
    f = gold["figures"]
    assert (f["logit_row_std"] >= 1.0).all() and (f["branch_rms_ratio"] >= 0.25).all()
    assert gold["cases"]["a"]["x"].shape == (2, 3, 182, 252) and gold["cases"]["a"]["last_hidden_state"].shape == (2, 235, 128)
    assert gold["cases"]["b"]["last_hidden_state"].shape == (1, 26, 128) and gold["cases"]["c"]["last_hidden_state"].shape == (1, 2, 128)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_ref_float64_matches_transformers(gold, name):
    case = gold["cases"][name]
    hidden, tokens = R.forward(gold["hub"], case["x"], dtype=torch.float64)
    np.testing.assert_allclose(tokens.numpy(), case["last_hidden_state"].numpy(), rtol=1e-9, atol=0)
    np.testing.assert_allclose(stored_hidden(name, torch.stack(hidden)).numpy(), case["hidden_states"].numpy(), rtol=1e-9, atol=0)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_cpu_path_inside_the_fp32_gate(gold, model, name):
    case = gold["cases"][name]
    h64, t64, gates, gate = R.gate(gold["hub"], case["x"])
    hs, tokens = model.hidden_states(case["x"])
    assert len(hs) == len(h64) == 3
    for i, (a, b, g) in enumerate(zip(hs, h64, gates)):
        err = float((a.double() - b).abs().max())
        print(f"case {name} hidden {i}: err {err:.3e} gate {g:.3e}")
        assert err <= g, (i, err, g)
    err = float((tokens.double() - case["last_hidden_state"]).abs().max())
    print(f"case {name} tokens: err {err:.3e} gate {gate:.3e}")
    assert err <= gate
    out = model.forward_features(case["x"])
    assert out["x_norm_clstoken"].dtype == torch.float32 and out["x_norm_clstoken"].shape == (case["x"].shape[0], 128)
    assert torch.equal(out["x_norm_clstoken"], tokens[:, 0]) and torch.equal(out["x_norm_patchtokens"], tokens[:, 1:])
    assert torch.equal(model.forward_features(case["x"].half())["x_norm_patchtokens"], tokens[:, 1:])  # (the inputs are fp16 numbers)


@pytest.mark.parametrize("preset, c, depth", [("dinov2_vits14", 384, 12), ("dinov2_vitb14", 768, 12), ("dinov2_vitl14", 1024, 24)])
def test_preset_state_dict_names_and_shapes(preset, c, depth):
    from p2p_bridge_amd import dinov2

    m = getattr(dinov2, preset)()
    sd = m.state_dict()
    assert list(sd) == HUB_NAMES + [f"blocks.{i}.{n}" for i in range(depth) for n in BLOCK_NAMES] + ["norm.weight", "norm.bias"]
    shapes = {"cls_token": (1, 1, c), "pos_embed": (1, 1 + 37 * 37, c), "mask_token": (1, c),
              "patch_embed.proj.weight": (c, 3, 14, 14), "patch_embed.proj.bias": (c,), "norm.weight": (c,), "norm.bias": (c,),
              "blocks.0.attn.qkv.weight": (3 * c, c), "blocks.0.attn.qkv.bias": (3 * c,), "blocks.0.attn.proj.weight": (c, c),
              "blocks.0.ls1.gamma": (c,), "blocks.0.mlp.fc1.weight": (4 * c, c), "blocks.0.mlp.fc2.weight": (c, 4 * c),
              f"blocks.{depth - 1}.ls2.gamma": (c,)}
    for k, s in shapes.items():
        assert tuple(sd[k].shape) == s, k
    assert m.num_heads * 64 == c and m.interpolate_offset == 0.1 and not any(p.requires_grad for p in m.parameters())
    # strict both ways: a checkpoint with exactly these names loads, one name more or less does not
    m.load_state_dict({k: torch.zeros_like(v) for k, v in sd.items()}, strict=True)
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != "mask_token"}, strict=True)
    with pytest.raises(RuntimeError):
        m.load_state_dict({**sd, "register_tokens": torch.zeros(1, 4, c)}, strict=True)


def test_transformers_round_trip(gold, model):
    from p2p_bridge_amd import dinov2

    assert model.embed_dim == 128 and model.depth == 2 and model.num_heads == 2 and model.grid == 5 and model.interpolate_offset == 0
    sd = model.state_dict()
    assert set(sd) == set(gold["hub"]) and all(torch.equal(sd[k], gold["hub"][k]) for k in sd)
    back = R.transformers_from_hub(sd)
    assert set(back) == set(gold["tsd"]) and all(torch.equal(back[k], gold["tsd"][k]) for k in back)
    again = dinov2.DinoV2.from_transformers_state_dict({"dinov2." + k: v for k, v in back.items()})
    assert all(torch.equal(v, again.state_dict()[k]) for k, v in sd.items())
    q = gold["tsd"]["encoder.layer.1.attention.attention.key.weight"]
    assert torch.equal(sd["blocks.1.attn.qkv.weight"][128:256], q)  # rows (q | k | v)


def test_unsupported_variants_raise(gold):
    from p2p_bridge_amd import dinov2

    for name in ("dinov2_vitg14", "dinov2_vits14_reg", "dinov2_vitg14_reg", "dinov2_vitx14"):
        with pytest.raises(ValueError):
            dinov2.create(name)
    with pytest.raises(ValueError, match="SwiGLU"):
        dinov2.DinoV2(ffn_layer="swiglufused")
    with pytest.raises(ValueError, match="register"):
        dinov2.DinoV2(num_register_tokens=4)
    with pytest.raises(ValueError):
        dinov2.DinoV2(embed_dim=384, num_heads=12)  # 32-wide heads
    with pytest.raises(ValueError, match="register"):
        dinov2.DinoV2.from_transformers_state_dict({**gold["tsd"], "embeddings.register_tokens": torch.zeros(1, 4, 128)})
    with pytest.raises(ValueError, match="SwiGLU"):
        dinov2.DinoV2.from_transformers_state_dict({**gold["tsd"], "encoder.layer.0.mlp.weights_in.weight": torch.zeros(1, 1)})
    m = dinov2.DinoV2.from_transformers_state_dict(gold["tsd"])
    with pytest.raises(ValueError):
        m.forward_features(torch.zeros(1, 3, 15, 14))


def test_position_table_rules(gold, model):
    from p2p_bridge_amd import dinov2

    assert torch.equal(model.pos_table(5, 5), gold["hub"]["pos_embed"][0])  # the native grid: no interpolation
    assert torch.equal(model.pos_table(13, 18), R.pos_table(gold["hub"]["pos_embed"], 5, 13, 18))
    off = dinov2.DinoV2.from_transformers_state_dict(gold["tsd"], interpolate_offset=0.1)
    t = off.pos_table(13, 18)
    assert torch.equal(t, R.pos_table(gold["hub"]["pos_embed"], 5, 13, 18, 0.1)) and not torch.equal(t, model.pos_table(13, 18))
    assert torch.equal(off.pos_table(5, 5), gold["hub"]["pos_embed"][0])


def test_get_dino_features_mirrors_the_reference(gold, model):
    from p2p_bridge_amd import dinov2

    assert dinov2.IMAGENET_DEFAULT_MEAN == (0.485, 0.456, 0.406) and dinov2.IMAGENET_DEFAULT_STD == (0.229, 0.224, 0.225)
    g = torch.Generator().manual_seed(3)
    image = torch.rand(2, 3, 75, 100, generator=g).half()  # neither side a multiple of 14: cropped to 70 x 98
    out = dinov2.get_dino_features(model, image)
    assert out.shape == (2, 128, 75, 100) and out.dtype == torch.float16
    mean = torch.tensor(dinov2.IMAGENET_DEFAULT_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(dinov2.IMAGENET_DEFAULT_STD).view(1, 3, 1, 1)
    x = ((image.float() - mean) / std)[:, :, :70, :98]
    assert torch.equal(dinov2.normalize(image)[:, :, :70, :98], x)
    tok = model.forward_features(x)["x_norm_patchtokens"].half().reshape(2, 5, 7, 128).permute(0, 3, 1, 2)
    assert torch.equal(out, F.interpolate(tok, size=(75, 100), mode="bilinear", antialias=False))
    grid = dinov2.feature_fn(model)(image)
    assert grid.shape == (2, 128, 5, 7) and grid.dtype == torch.float16 and torch.equal(grid, tok)
    assert grid.permute(0, 2, 3, 1).is_contiguous()
    _, t64 = R.forward(gold["hub"], x, dtype=torch.float64)  # and the tokens are the model's
    assert float((tok.permute(0, 2, 3, 1).reshape(2, 35, 128).double() - t64[:, 1:]).abs().max()) < 2e-3  # one fp16 rounding at |x| < 4


# ---- sample_grid -----------------------------------------------------------------------------------------------------
def f16_order(t):
    """fp16 -> integers in which adjacent fp16 numbers differ by one"""
    i = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def all_pixels(b, h, w):
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    return torch.stack([xs.flatten(), ys.flatten()], -1).to(torch.int32)[None].repeat(b, 1, 1).contiguous()


def test_sample_grid_within_one_ulp_of_interpolate():
    from p2p_bridge_amd import image_features as IF

    # A grid of ONE sign (uniform in [0, 1)): every value is a convex combination of same-sign operands, so any fp32 evaluation
    # order is within a few fp32 ulps of the exact value and two of them round to fp16 numbers at most one apart. Torch's CPU
    # kernel is not bit-equal to the written contract (it contracts multiply-adds), hence "one ulp" and not equality.
    g = torch.Generator().manual_seed(0)
    grid = torch.rand(2, 13, 18, 48, generator=g).half()
    out = IF.sample_grid(grid, (192, 256), all_pixels(2, 192, 256))
    assert out.shape == (2, 192 * 256, 48) and out.dtype == torch.float16
    full = F.interpolate(grid.float().permute(0, 3, 1, 2).contiguous(), size=(192, 256), mode="bilinear", antialias=False).half()
    full = full.permute(0, 2, 3, 1).reshape(2, 192 * 256, 48)
    diff = (f16_order(out) - f16_order(full)).abs()
    print(f"{int((diff > 0).sum())} of {diff.numel()} values differ, max {int(diff.max())} ulp")
    assert int(diff.max()) <= 1
    assert float((diff > 0).float().mean()) < 0.01


def test_sample_grid_signed_grid_against_float64():
    """A signed grid (what DINO tokens are): where the four operands cancel, an fp16 ulp OF THE RESULT is smaller than the fp32
    rounding of the operands, so no two fp32 evaluation orders agree to one result-ulp there (torch's own kernel differs from
    the written contract by up to 15 such ulps on this grid). The bound that does hold, against bilinear weights in float64:
    half an fp16 ulp of the exact value (the one rounding) + the fp32 error of the 7 operations on operands <= max |grid|,
    8 * 2^-24 * max |grid|, + the fp32 error of the weights: src = (dst + 0.5) * scale - 0.5 < 16 carries the rounding of scale
    (src * 2^-24 <= 2^-20) and two roundings of 2^-21 each, so |dl| <= 2^-19 per axis, moving the value by |dl| * |a - b| <=
    2^-19 * 2 max |grid| per axis: 2^-17 * max |grid| for both."""
    from p2p_bridge_amd import image_features as IF

    g = torch.Generator().manual_seed(0)
    grid = torch.randn(2, 13, 18, 48, generator=g).half()
    out = IF.sample_grid(grid, (192, 256), all_pixels(2, 192, 256))
    exact = F.interpolate(grid.double().permute(0, 3, 1, 2).contiguous(), size=(192, 256), mode="bilinear", antialias=False)
    exact = exact.permute(0, 2, 3, 1).reshape(2, 192 * 256, 48)
    half_ulp = torch.maximum(2.0 ** (torch.floor(torch.log2(exact.abs().clamp_min(2.0 ** -14))) - 11), torch.tensor(2.0 ** -25, dtype=torch.float64))
    bound = half_ulp + (2.0 ** -17 + 8 * 2.0 ** -24) * float(grid.abs().max())
    err = (out.double() - exact).abs()
    print(f"max err / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


def test_sample_grid_corners_and_clamp():
    from p2p_bridge_amd import image_features as IF

    g = torch.Generator().manual_seed(1)
    grid = torch.randn(1, 13, 18, 5, generator=g).half()
    h, w = 192, 256
    xy = torch.tensor([[[0, 0], [w - 1, h - 1], [-7, -1], [w + 40, h], [-1, h + 5], [w, -3], [100, 77]]], dtype=torch.int32)
    out = IF.sample_grid(grid, (h, w), xy)[0]
    assert torch.equal(out[0], grid[0, 0, 0]) and torch.equal(out[1], grid[0, 12, 17])  # the corners are grid values
    assert torch.equal(out[2], out[0]) and torch.equal(out[3], out[1])
    assert torch.equal(out[4], grid[0, 12, 0]) and torch.equal(out[5], grid[0, 0, 17])
    inside = IF.sample_grid(grid.numpy(), (h, w), xy.numpy())  # numpy in, numpy out
    assert isinstance(inside, np.ndarray) and np.array_equal(inside[0].view(np.uint16), out.numpy().view(np.uint16))
    # the written formula at an interior pixel, by hand
    sx, sy = (100 + 0.5) * (18 / 256) - 0.5, (77 + 0.5) * (13 / 192) - 0.5
    x0, y0 = int(sx), int(sy)
    lx, ly = sx - x0, sy - y0
    gd = grid[0].double()
    want = (1 - ly) * ((1 - lx) * gd[y0, x0] + lx * gd[y0, x0 + 1]) + ly * ((1 - lx) * gd[y0 + 1, x0] + lx * gd[y0 + 1, x0 + 1])
    assert float((out[6].double() - want).abs().max()) < 2e-3
    with pytest.raises(RuntimeError):
        IF.sample_grid(grid.float(), (h, w), xy)
    with pytest.raises(ValueError):
        IF.sample_grid(grid, (h, w), xy.repeat(2, 1, 1))


def test_update_features_from_grid_is_sample_then_mean():
    from p2p_bridge_amd import image_features as IF

    g = torch.Generator().manual_seed(2)
    b, n, c, h, w = 3, 400, 8, 48, 64
    grid = torch.randn(b, 5, 7, c, generator=g).half()
    xy = torch.stack([torch.randint(-3, w + 3, (b, n), generator=g), torch.randint(-3, h + 3, (b, n), generator=g)], -1).to(torch.int32)
    valid = torch.rand(b, n, generator=g) < 0.6
    mean, count = torch.randn(n, c, generator=g).half(), torch.randint(0, 3, (n,), generator=g, dtype=torch.int32)
    rows = IF.sample_grid(grid, (h, w), xy)
    want_m, want_c = mean.clone(), count.clone()
    for f in range(b):  # update_features on a one-pixel-per-point "map" made of the sampled rows
        maps = rows[f].reshape(1, 1, n, c).contiguous()
        at = torch.stack([torch.arange(n), torch.zeros(n, dtype=torch.long)], -1).to(torch.int32)[None]
        IF.update_features(want_m, want_c, maps, valid[f:f + 1], at)
    got = IF.update_features_from_grid(mean, count, grid, (h, w), valid, xy)
    assert got[0] is mean and got[1] is count
    assert torch.equal(count, want_c) and torch.equal(mean.view(torch.int16), want_m.view(torch.int16))


def test_fuse_scene_from_grid_against_a_hand_rolled_loop():
    import os

    from p2p_bridge_amd import image_features as IF

    gold = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_features.npz")))
    w, h = (int(v) for v in gold["size"])
    nf, c = gold["rotation"].shape[0], 16
    g = torch.Generator().manual_seed(4)
    grids = torch.randn(nf, c, 5, 7, generator=g).half()
    frames = []
    for f in range(nf):
        w2c = np.eye(4)
        w2c[:3, :3], w2c[:3, 3] = gold["rotation"][f], gold["translation"][f]
        frames.append({"image": np.full((h, w, 3), f / 8.0, dtype=np.float32), "intrinsic": gold["camera"][f], "world_to_camera": w2c})

    def feature_fn(images):
        first = int(round(float(images[0, 0, 0, 0]) * 8))
        return grids[first:first + images.shape[0]]

    kw = dict(feature_type="dino", feature_fn=feature_fn, batch_size=2, mask_size=(h, w), intrinsic_scale=1.0, sampling_rate=1)
    out = IF.fuse_scene(gold["points"], frames, dino_from_grid=True, **kw)
    pts = torch.from_numpy(gold["points"].astype(np.float64))
    n = pts.shape[0]
    mean, count = torch.zeros(n, c, dtype=torch.float16), torch.zeros(n, dtype=torch.int32)
    for f in range(nf):  # frame by frame: sample_grid rows, then the running mean with its three roundings
        valid, xy = IF.visible_points(pts, torch.from_numpy(gold["rotation"][f:f + 1]), torch.from_numpy(gold["translation"][f:f + 1]),
                                      torch.from_numpy(gold["camera"][f:f + 1]), w, h)
        rows = IF.sample_grid(grids[f:f + 1].permute(0, 2, 3, 1).contiguous(), (h, w), xy)[0]
        for i in torch.nonzero(valid[0]).flatten().tolist():
            count[i] += 1
            d = (rows[i].float() - mean[i].float()).half()
            q = (d.float() / float(count[i])).half()
            mean[i] = (mean[i].float() + q.float()).half()
    IF.interpolate_missing_features(mean, count, torch.from_numpy(gold["points"]))
    assert out.shape == (c, n) and out.dtype == torch.float16
    assert torch.equal(out.view(torch.int16), torch.nan_to_num(mean).t().contiguous().view(torch.int16))
    # the default path is untouched by the keyword and differs only in the last place (fp16 map against fp32 evaluation)
    default = IF.fuse_scene(gold["points"], frames, **kw)
    assert torch.equal(default, IF.fuse_scene(gold["points"], frames, dino_from_grid=False, **kw))
    assert float((default.float() - out.float()).abs().max()) < 0.05 and (count > 0).sum() > 100
