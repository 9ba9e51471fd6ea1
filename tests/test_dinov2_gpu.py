"""The kernels of csrc/vit.hip and the token-grid sampling of csrc/imgfeat.hip on the GPU.

References run no HIP: float64 torch on the CPU (tests/dinov2_ref.py, itself pinned to `transformers` by tests/test_dinov2.py),
or the CPU twin where the contract is bit-exactness. Every tolerance is 4 x the error of the same computation in torch's fp32
on the CPU against float64 ON THE SAME INPUTS, computed in the test (never the code under test): the margin this project gives
its own arithmetic over an fp32 evaluation (test_full_size_parity_gpu.py). Each case prints its error next to its gate.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dinov2_ref as R
from oracle.poison_arena import PoisonArena

pytestmark = pytest.mark.gpu

F64 = torch.float64
DEV = "cuda"


def held(name, got, ref64, yard32):
    """got inside 4 x max |yard32 - ref64| of ref64"""
    gate = R.GATE_FACTOR * float((yard32.double() - ref64).abs().max())
    err = float((got.double().cpu() - ref64).abs().max())
    print(f"[{name}] err {err:.3e} gate {gate:.3e}")
    assert torch.isfinite(got).all(), name
    assert err <= gate, (name, err, gate)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu()


@pytest.fixture(scope="module")
def dinov2():
    from p2p_bridge_amd import dinov2 as d

    return d


@pytest.fixture(scope="module")
def IF():
    from p2p_bridge_amd import image_features

    return image_features


@pytest.fixture(scope="module")
def gold():
    tsd, cases, _ = R.load_golden()
    return {"tsd": tsd, "hub": R.hub_from_transformers(tsd), "cases": cases}


# ---- LayerNorm -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [128, 384])
@pytest.mark.parametrize("t", [1, 2, 65, 235])
def test_layernorm_far_from_zero_mean(dinov2, c, t):
    """mean 50, std 0.5 per token: E[x^2] - E[x]^2 in fp32 has no correct digit here"""
    g = torch.Generator().manual_seed(c + t)
    x = 50.0 + 0.5 * torch.randn(2, t, c, generator=g)
    w, b = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    ref = R.layer_norm(x.double(), w.double(), b.double(), 1e-6)
    y = dinov2.layernorm(x.to(DEV), w.to(DEV), b.to(DEV), 1e-6)
    assert y.shape == x.shape
    held(f"layernorm C={c} T={t}", y, ref, F.layer_norm(x, (c,), w, b, 1e-6))


# ---- attention -------------------------------------------------------------------------------------------------------
def attention_ref(qkv, heads, dtype):
    b, n, _ = qkv.shape
    q, k, v = qkv.to(dtype).reshape(b, n, 3, heads, 64).permute(2, 0, 3, 1, 4)
    return R.attention(q, k, v).transpose(1, 2).reshape(b, n, heads * 64)


def qkv_case(heads, t, seed):
    """q, k ~ N(0, 5): logits (q . k) / 8 with a row standard deviation of about 5"""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(2, t, 3, heads, 64, generator=g)
    qkv[:, :, :2] *= 5.0 ** 0.5
    return qkv.reshape(2, t, 3 * heads * 64).contiguous()


@pytest.mark.parametrize("heads", [2, 6])
@pytest.mark.parametrize("t", [1, 2, 63, 64, 65, 235, 1370])
def test_attention_against_float64(dinov2, heads, t):
    qkv = qkv_case(heads, t, 100 * heads + t)
    ref = attention_ref(qkv, heads, F64)
    if t > 2:
        q, k = qkv.double().reshape(2, t, 3, heads, 64)[:, :, 0], qkv.double().reshape(2, t, 3, heads, 64)[:, :, 1]
        row_std = float((torch.einsum("bihd,bjhd->bhij", q, k) / 8).std(-1).mean())
        assert 3.5 < row_std < 6.5, row_std
    dq = qkv.to(DEV)
    out = dinov2.attention(dq, heads)
    held(f"attention heads={heads} T={t}", out, ref, attention_ref(qkv, heads, torch.float32))
    assert torch.equal(bits(out), bits(dinov2.attention(dq, heads)))  # no atomics: the same bits on every run


@pytest.mark.parametrize("heads, t", [(2, 65), (6, 235), (2, 2), (2, 1)])
@pytest.mark.parametrize("fill", [float("nan"), 1e30])
def test_attention_padding_has_no_weight(dinov2, heads, t, fill):
    """rows >= n_valid of q, k and v hold NaN / 1e30: the valid outputs keep their bits, the padded output rows are zeros"""
    pad = 7
    qkv = qkv_case(heads, t, 7 * heads + t)
    padded = torch.full((2, t + pad, qkv.shape[2]), fill)
    padded[:, :t] = qkv
    plain = dinov2.attention(qkv.to(DEV), heads)
    out = dinov2.attention(padded.to(DEV), heads, n_valid=t)
    assert out.shape == (2, t + pad, heads * 64)
    assert torch.equal(bits(out[:, :t]), bits(plain))
    assert torch.equal(out[:, t:].cpu(), torch.zeros(2, pad, heads * 64))


def test_attention_peaked_and_flat_rows(dinov2):
    """a key 80 above the rest takes the whole weight without overflow; equal keys give the plain mean of v"""
    heads, t = 2, 65
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(2, t, 3, heads, 64, generator=g)
    # image 0: q = 8 e_0 for every query, so logit_j = k_j[0]: zero except key 40 (80) -- placed in the second key tile
    qkv[0, :, 0] = 0.0
    qkv[0, :, 0, :, 0] = 8.0
    qkv[0, :, 1, :, 0] = 0.0
    qkv[0, 40, 1, :, 0] = 80.0
    # image 1: every key the same vector
    qkv[1, :, 1] = qkv[1, 0, 1].clone()
    qkv = qkv.reshape(2, t, -1).contiguous()
    ref = attention_ref(qkv, heads, F64)
    out = dinov2.attention(qkv.to(DEV), heads)
    held("attention peaked / flat", out, ref, attention_ref(qkv, heads, torch.float32))
    v = qkv.reshape(2, t, 3, heads, 64)[:, :, 2]
    assert torch.equal(out[0].cpu(), v[0, 40].reshape(1, -1).expand(t, -1))  # exp(-80) vanishes against 1 in fp32
    assert float((out[1].cpu().double() - v[1].double().mean(0).reshape(1, -1)).abs().max()) < 1e-6


def test_attention_refuses_bad_arguments(dinov2):
    qkv = torch.zeros(1, 4, 3 * 2 * 64, device=DEV)
    with pytest.raises(ValueError):
        dinov2.attention(qkv, 3)
    with pytest.raises(ValueError):
        dinov2.attention(qkv, 2, n_valid=5)
    with pytest.raises(RuntimeError):
        dinov2.attention(qkv.cpu(), 2)


# ---- linear layers with their epilogues ---------------------------------------------------------------------------------
@pytest.mark.parametrize("m, n, k", [(1, 128, 128), (2, 384, 128), (65, 128, 588), (470, 512, 128), (470, 128, 512), (130, 1152, 384)])
def test_linear_epilogues_against_float64(dinov2, m, n, k):
    g = torch.Generator().manual_seed(m + n + k)
    x, w, b = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g) / k ** 0.5, torch.randn(n, generator=g)
    gamma, res = torch.rand(n, generator=g) + 0.5, torch.randn(m, n, generator=g)
    dx, dw, db = x.to(DEV), w.to(DEV), b.to(DEV)
    y64 = x.double() @ w.double().t() + b.double()
    y32 = F.linear(x, w, b)
    held(f"linear {m}x{n}x{k} bias", dinov2.linear(dx, dw, db), y64, y32)
    held(f"linear {m}x{n}x{k} gelu", dinov2.linear(dx, dw, db, gelu=True), R.gelu(y64), F.gelu(y32))
    dres = res.to(DEV)
    out = dinov2.linear(dx, dw, db, residual=dres, gamma=gamma.to(DEV))
    assert out is dres
    held(f"linear {m}x{n}x{k} residual", out, res.double() + gamma.double() * y64, res + gamma * y32)


# ---- the whole model -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(dinov2, gold):
    return dinov2.DinoV2.from_transformers_state_dict(gold["tsd"]).to(DEV)


def model_held(name, model, x, h64, t64, gates, gate):
    hs, tokens = model.hidden_states(x.to(DEV))
    assert len(hs) == len(h64)
    for i, (a, b, g) in enumerate(zip(hs, h64, gates)):
        err = float((a.double().cpu() - b).abs().max())
        print(f"[{name}] hidden {i} (0 = embeddings): err {err:.3e} gate {g:.3e}")
        assert torch.isfinite(a).all() and err <= g, (name, "hidden state", i, err, g)
    err = float((tokens.double().cpu() - t64).abs().max())
    print(f"[{name}] tokens: err {err:.3e} gate {gate:.3e}, RMS {float(t64.pow(2).mean().sqrt()):.3f}")
    assert torch.isfinite(tokens).all() and err <= gate, (name, err, gate)
    return tokens


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_tiny_model_against_transformers(tiny, gold, name):
    case = gold["cases"][name]
    h64, t64, gates, gate = R.gate(gold["hub"], case["x"])
    tokens = model_held(f"tiny {name}", tiny, case["x"], h64, t64, gates, gate)
    err = float((tokens.double().cpu() - case["last_hidden_state"]).abs().max())  # the stored result itself
    assert err <= gate, (err, gate)
    out = tiny.forward_features(case["x"].to(DEV))
    assert torch.equal(bits(out["x_norm_patchtokens"]), bits(tokens[:, 1:])) and torch.equal(bits(out["x_norm_clstoken"]), bits(tokens[:, 0]))


@pytest.fixture(scope="module")
def vits():
    return R.random_weights(384, 12, 37, seed=77), R.images(2, 182, 252, seed=78)


@pytest.mark.parametrize("offset", [0.0, 0.1])
def test_vit_small_against_float64(dinov2, vits, offset):
    """ViT-S/14 (384 wide, 12 blocks, 6 heads) with weights of the fixture's recipe at 2 x 182 x 252. offset 0.1 runs the hub's
    scale_factor rule with the same host-side table on both sides: that tests the kernels, not the rule."""
    sd, x = vits
    model = dinov2.dinov2_vits14(interpolate_offset=offset)
    model.load_state_dict(sd, strict=True)
    model.to(DEV)
    h64, t64, gates, gate = R.gate(sd, x, offset=offset)
    assert torch.equal(model.pos_table(13, 18).cpu(), R.pos_table(sd["pos_embed"], 37, 13, 18, offset))
    model_held(f"vit-s offset={offset}", model, x, h64, t64, gates, gate)


def test_range_outlier_channel_and_large_activations(dinov2, gold):
    """post-GELU activations above 4095 and a residual channel at 3000 (outside the exact range of the f16x3 split arithmetic,
    DESIGN 3.1): finite and inside the same gate"""
    sd = {k: v.clone() for k, v in gold["hub"].items()}
    sd["blocks.0.mlp.fc1.weight"] *= 4000.0
    sd["blocks.0.mlp.fc1.bias"] *= 4000.0
    sd["blocks.0.mlp.fc2.weight"] /= 4000.0
    sd["cls_token"][0, 0, 7] += 3000.0
    sd["patch_embed.proj.bias"][7] += 3000.0
    x = gold["cases"]["a"]["x"]
    taps = {}
    hidden, _ = R.forward(sd, x, taps=taps)
    assert taps["post_gelu_max"][0] > 4095 and float(hidden[0][..., 7].abs().min()) > 2900
    model = dinov2.DinoV2(embed_dim=128, depth=2, num_heads=2, grid=5, interpolate_offset=0.0)
    model.load_state_dict(sd, strict=True)
    model_held("range", model.to(DEV), x, *R.gate(sd, x))


# ---- sample_grid / update_features_from_grid -----------------------------------------------------------------------------
def grid_case(c, seed):
    g = torch.Generator().manual_seed(seed)
    b, n, h, w = 2, 1000, 192, 256
    grid = torch.randn(b, 13, 18, c, generator=g).half()
    xy = torch.stack([torch.randint(0, w, (b, n), generator=g), torch.randint(0, h, (b, n), generator=g)], -1).to(torch.int32)
    special = torch.tensor([[0, 0], [w - 1, h - 1], [0, h - 1], [w - 1, 0], [-1, -1], [-500, 3], [w, h], [w + 9, -2], [17, h + 100]],
                           dtype=torch.int32)
    xy[:, :len(special)] = special
    valid = torch.rand(b, n, generator=g) < 0.6
    valid[:, :len(special)] = True  # corners and out-of-range pixels in both frames
    valid[:, 100:200] = True  # points seen by both frames
    valid[:, 200:250] = False  # and by none
    mean, count = torch.randn(n, c, generator=g).half(), torch.randint(0, 4, (n,), generator=g, dtype=torch.int32)
    return grid, xy, valid, mean, count, (h, w)


@pytest.mark.parametrize("c", [5, 384])
def test_sample_and_fuse_from_grid_bit_equal_to_cpu_twin(IF, c):
    grid, xy, valid, mean, count, size = grid_case(c, c)
    want = IF.sample_grid(grid, size, xy)
    got = IF.sample_grid(grid.to(DEV), size, xy.to(DEV))
    assert got.dtype == torch.float16 and torch.equal(bits(got), bits(want))
    want_m, want_c = IF.update_features_from_grid(mean.clone(), count.clone(), grid, size, valid, xy)
    dm, dc = mean.to(DEV), count.to(DEV)
    IF.update_features_from_grid(dm, dc, grid.to(DEV), size, valid.to(DEV), xy.to(DEV))
    assert torch.equal(dc.cpu(), want_c) and torch.equal(bits(dm), bits(want_m))
    assert torch.equal(want_c, count + valid.sum(0).to(torch.int32)) and not torch.equal(want_m, mean)
    assert torch.equal(bits(dm[200:250]), bits(mean[200:250]))  # unseen points keep their rows


def test_fuse_scene_from_grid_with_the_model(IF, dinov2, tiny, gold):
    """fuse_scene(dino_from_grid=True) with feature_fn(model) on the GPU == the same call on the CPU path given the same token
    grid (the scene of tests/golden/image_features.npz: 6000 points, 6 frames of 24 x 32, so a 1 x 2 token grid per frame)"""
    scene = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_features.npz")))
    w, h = (int(v) for v in scene["size"])
    rng = np.random.default_rng(0)
    frames = []
    for f in range(scene["rotation"].shape[0]):
        w2c = np.eye(4)
        w2c[:3, :3], w2c[:3, 3] = scene["rotation"][f], scene["translation"][f]
        frames.append({"image": rng.uniform(0, 1, (h, w, 3)).astype(np.float32), "intrinsic": scene["camera"][f], "world_to_camera": w2c})
    seen = []
    fn = dinov2.feature_fn(tiny)

    def recording(images):
        out = fn(images)
        seen.append(out.cpu())
        return out

    kw = dict(feature_type="dino", batch_size=2, mask_size=(h, w), intrinsic_scale=1.0, sampling_rate=1, dino_from_grid=True)
    out = IF.fuse_scene(torch.from_numpy(scene["points"]).to(DEV), frames, feature_fn=recording, **kw)
    assert len(seen) == 3 and seen[0].shape == (2, 128, 1, 2) and seen[0].dtype == torch.float16
    replay = iter(seen)
    want = IF.fuse_scene(scene["points"], frames, feature_fn=lambda images: next(replay), **kw)
    assert out.is_cuda and out.shape == (128, scene["points"].shape[0]) and torch.equal(bits(out), bits(want))
    assert float(want.float().abs().max()) > 0.5


# ---- poisoned arena --------------------------------------------------------------------------------------------------
ARENA_BYTES = 64 << 20


@pytest.fixture
def arena():
    with PoisonArena(DEV, ARENA_BYTES) as a:
        yield a


def checked(arena, what, fn, *args, **kwargs):
    """one wrapper call inside the arena: it allocated through the patch, the guards are intact, every result element was
    written and none is NaN"""
    n0 = arena.n_allocations
    out = fn(*args, **kwargs)
    assert arena.n_allocations > n0, f"{what} did not allocate through the arena"
    arena.check_guards()
    for i, t in enumerate(out if isinstance(out, (tuple, list)) else [out]):
        arena.assert_written(t, f"{what} result {i}")
    return out


@pytest.mark.parametrize("t", [235, 2])
def test_operators_inside_the_poisoned_arena(arena, dinov2, t):
    g = torch.Generator().manual_seed(t)
    c, heads, rows = 128, 2, 2 * t
    x = torch.randn(2, t, c, generator=g)
    w, b = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    y = checked(arena, "layernorm", dinov2.layernorm, arena.put(x), arena.put(w), arena.put(b), 1e-6)
    held(f"arena layernorm T={t}", y, R.layer_norm(x.double(), w.double(), b.double(), 1e-6), F.layer_norm(x, (c,), w, b, 1e-6))

    qkv = qkv_case(heads, t, t)
    out = checked(arena, "attention", dinov2.attention, arena.put(qkv), heads)
    held(f"arena attention T={t}", out, attention_ref(qkv, heads, F64), attention_ref(qkv, heads, torch.float32))
    padded = torch.cat([qkv, torch.full((2, 3, qkv.shape[2]), float("nan"))], 1)  # 3 padded rows: their outputs are zeros
    outp = checked(arena, "attention (padded)", dinov2.attention, arena.put(padded), heads, n_valid=t)
    assert torch.equal(bits(outp[:, :t]), bits(out)) and not outp[:, t:].any()

    xm, wm, bm = torch.randn(rows, c, generator=g), torch.randn(4 * c, c, generator=g) / c ** 0.5, torch.randn(4 * c, generator=g)
    y64, y32 = xm.double() @ wm.double().t() + bm.double(), F.linear(xm, wm, bm)
    dx, dw, db = arena.put(xm), arena.put(wm), arena.put(bm)
    held(f"arena linear bias T={t}", checked(arena, "linear", dinov2.linear, dx, dw, db), y64, y32)
    hid = checked(arena, "linear gelu", dinov2.linear, dx, dw, db, gelu=True)
    held(f"arena linear gelu T={t}", hid, R.gelu(y64), F.gelu(y32))
    w2, b2 = torch.randn(c, 4 * c, generator=g) / (4 * c) ** 0.5, torch.randn(c, generator=g)
    gamma, res = torch.rand(c, generator=g) + 0.5, torch.randn(rows, c, generator=g)
    dres = arena.put(res)
    h32 = F.gelu(y32)
    dinov2.linear(hid, arena.put(w2), arena.put(b2), residual=dres, gamma=arena.put(gamma))  # in place: nothing to allocate
    arena.check_guards()
    arena.assert_written(dres, "linear residual")
    held(f"arena linear residual T={t}", dres, res.double() + gamma.double() * (R.gelu(y64) @ w2.double().t() + b2.double()),
         res + gamma * F.linear(h32, w2, b2))


@pytest.mark.parametrize("name", ["a", "c"])  # T = 235 and T = 2
def test_forward_features_inside_the_poisoned_arena(arena, dinov2, gold, name):
    model = dinov2.DinoV2.from_transformers_state_dict(gold["tsd"])
    for prm in model.parameters():  # every weight between guards
        prm.data = arena.put(prm.data)
    case = gold["cases"][name]
    out = checked(arena, "forward_features", lambda x: tuple(model.forward_features(x).values()), arena.put(case["x"]))
    tokens = torch.cat([out[0][:, None], out[1]], 1)
    h64, t64, gates, gate = R.gate(gold["hub"], case["x"])
    err = float((tokens.double().cpu() - t64).abs().max())
    print(f"[arena forward {name}] err {err:.3e} gate {gate:.3e}")
    assert err <= gate


@pytest.mark.parametrize("c", [5, 384])
def test_grid_sampling_inside_the_poisoned_arena(arena, IF, c):
    grid, xy, valid, mean, count, size = grid_case(c, 10 + c)
    dgrid, dxy = arena.put(grid), arena.put(xy)
    got = checked(arena, "sample_grid", IF.sample_grid, dgrid, size, dxy)
    assert torch.equal(bits(got), bits(IF.sample_grid(grid, size, xy)))
    dm, dc = arena.put(mean), arena.put(count)
    IF.update_features_from_grid(dm, dc, dgrid, size, arena.put(valid), dxy)  # in place: nothing to allocate
    arena.check_guards()
    arena.assert_written(dm, "mean")
    want_m, want_c = IF.update_features_from_grid(mean.clone(), count.clone(), grid, size, valid, xy)
    assert torch.equal(dc.cpu(), want_c) and torch.equal(bits(dm), bits(want_m))
