"""The kernels of csrc/vit_f16.hip and DinoV2(precision="fp16") on the GPU.

References run no HIP. Where the contract is exactness (integer data through the matrix pipe, a softmax that selects one key,
the LayerNorm's rounding) the test asks for the bits. Everywhere else the gate is 4 x the error, against float64 on the same
inputs, of the contract restated in plain torch on the CPU (tests/dinov2_half_ref.py), computed in the test: never the code
under test. Each case prints its error next to its gate.
"""
import ctypes

import pytest
import torch

import dinov2_half_ref as H
import dinov2_ref as R
from oracle.poison_arena import PoisonArena

pytestmark = pytest.mark.gpu

F16, F32, F64 = torch.float16, torch.float32, torch.float64
DEV = "cuda"
T_LIST = [1, 2, 63, 64, 65, 235, 1370]


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16).cpu()


def held(name, got, ref64, yard):
    """got (fp16 or fp32) inside 4 x max |yard - ref64| of ref64; yard is in got's format"""
    assert yard.dtype == got.dtype, (yard.dtype, got.dtype)
    gate = H.GATE_FACTOR * float((yard.double() - ref64).abs().max())
    err = float((got.double().cpu() - ref64).abs().max())
    print(f"[{name}] err {err:.3e} gate {gate:.3e}")
    assert torch.isfinite(got).all(), name
    assert err <= gate, (name, err, gate)


@pytest.fixture(scope="module")
def dinov2():
    from p2p_bridge_amd import dinov2 as d

    return d


@pytest.fixture(scope="module")
def gold():
    tsd, cases, _ = R.load_golden()
    return {"tsd": tsd, "hub": R.hub_from_transformers(tsd), "cases": cases}


# ---- linear layers: exact integer data -----------------------------------------------------------------------------------
# the last shape is not one of a ViT layer at test sizes: it is the smallest that takes the 64-row tiles (m / 64 * n / 64 >= 512)
# with a K loop of more than one tile and a 32-wide K tail
@pytest.mark.parametrize("m, n, k", [(1, 128, 128), (2, 384, 128), (65, 128, 512), (130, 1152, 384), (470, 512, 128), (33, 64, 32),
                                     (1880, 1152, 96)])
def test_linear_half_exact_on_integer_data(dinov2, m, n, k):
    """x, w integers in [-4, 4] (products and sums exact in fp32), integer bias that puts the results into +-[2048, 8192) where
    fp16 spacing is 2 and 4: RESIDUAL must be the integer result, BIAS its round-to-nearest-even fp16 -- ties included. A wrong
    lane map, a dropped K tail or a row of the m edge changes integers; a convert that rounds toward zero changes the ties."""
    g = torch.Generator().manual_seed(1000 * m + n + k)
    x = torch.randint(-4, 5, (m, k), generator=g)
    w = torch.randint(-4, 5, (n, k), generator=g)
    bias = torch.randint(2048, 8192, (n,), generator=g) * (2 * torch.randint(0, 2, (n,), generator=g) - 1)
    gamma = 2 ** torch.randint(0, 3, (n,), generator=g)
    res = torch.randint(-1000, 1001, (m, n), generator=g)
    y = (x.double() @ w.double().t()).to(torch.int64) + bias  # (fp64 sums of these integers are exact)
    assert torch.equal(y[:2, :3], (x[:2] @ w[:3].t()) + bias[:3])
    mag = y.abs()
    ties = ((mag >= 2048) & (mag < 4096) & (mag % 2 == 1)) | ((mag >= 4096) & (mag < 8192) & (mag % 4 == 2))
    in_range = (mag >= 2048) & (mag < 8192)
    print(f"[linear_half {m}x{n}x{k}] {int(in_range.sum())} of {y.numel()} results in [2048, 8192), {int(ties.sum())} ties")
    assert int(in_range.sum()) * 2 > y.numel() and int(ties.sum()) > 0 and int(mag.max()) < 16384
    want = y.to(F32).half()
    assert bool((want.double().abs() > mag)[ties].any())  # some ties round AWAY from zero: a truncating convert would differ
    dx, dw, db = x.to(F16).to(DEV), w.to(F16).to(DEV), bias.to(F32).to(DEV)
    out = dinov2.linear_half(dx, dw, db)
    assert out.dtype == F16 and out.shape == (m, n)
    assert torch.equal(bits(out), bits(want))
    dres = res.to(F32).to(DEV)
    got = dinov2.linear_half(dx, dw, db, residual=dres, gamma=gamma.to(F32).to(DEV))
    assert got is dres and got.dtype == F32
    assert torch.equal(got.cpu().double(), (res + gamma * y).double())


def test_linear_half_gelu_inside_the_gate_and_overflow_is_inf(dinov2):
    m, n, k = 130, 512, 128
    g = torch.Generator().manual_seed(3)
    x, w, b = torch.randn(m, k, generator=g).half(), (torch.randn(n, k, generator=g) / k ** 0.5).half(), torch.randn(n, generator=g)
    y64 = x.double() @ w.double().t() + b.double()
    dx, dw, db = x.to(DEV), w.to(DEV), b.to(DEV)
    held("linear_half bias", dinov2.linear_half(dx, dw, db), y64, H.linear_half(x, w, b).half())
    held("linear_half gelu", dinov2.linear_half(dx, dw, db, gelu=True), R.gelu(y64), H.linear_half(x, w, b, gelu=True).half())
    gamma, res = torch.rand(n, generator=g) + 0.5, torch.randn(m, n, generator=g)
    out = dinov2.linear_half(dx, dw, db, residual=res.clone().to(DEV), gamma=gamma.to(DEV))
    held("linear_half residual", out, res.double() + gamma.double() * y64, res + gamma * H.linear_half(x, w, b))
    # 250 * 400 = 1e5 is beyond fp16: +inf, as torch's conversion makes it (no saturation to 65504)
    x = torch.zeros(2, 32, dtype=F16)
    w = torch.zeros(64, 32, dtype=F16)
    x[0, 0], x[1, 0], w[5, 0] = 250.0, -250.0, 400.0
    zero = torch.zeros(64, device=DEV)
    want = (x.float() @ w.float().t()).half()
    assert want[0, 5] == torch.tensor(1e5).half() == float("inf") and want[1, 5] == float("-inf")
    assert torch.equal(bits(dinov2.linear_half(x.to(DEV), w.to(DEV), zero)), bits(want))
    got = dinov2.linear_half(x.to(DEV), w.to(DEV), zero, gelu=True).cpu()
    assert got[0, 5] == float("inf") and got[1, 5] == 0 and int(torch.isinf(got).sum()) == 1 and not torch.isnan(got).any()


def test_linear_half_refuses_bad_arguments(dinov2):
    from p2p_bridge_amd import _lib

    x, w, b = torch.zeros(4, 64, dtype=F16, device=DEV), torch.zeros(64, 64, dtype=F16, device=DEV), torch.zeros(64, device=DEV)
    with pytest.raises(RuntimeError):
        dinov2.linear_half(x.float(), w, b)
    with pytest.raises(RuntimeError):
        dinov2.linear_half(x.cpu(), w.cpu(), b.cpu())
    with pytest.raises(ValueError):
        dinov2.linear_half(x, w[:32], b[:32])  # n % 64
    with pytest.raises(ValueError):
        dinov2.linear_half(x[:, :16].contiguous(), w[:, :16].contiguous(), b)  # k % 32
    with pytest.raises(ValueError):
        dinov2.linear_half(x, w, b, gelu=True, residual=torch.zeros(4, 64, device=DEV), gamma=b)
    # the library itself answers with its argument-error status
    ci, y = ctypes.c_int, torch.zeros(4, 64, dtype=F16, device=DEV)
    fn = _lib.lib().p2pb_vit_linear_f16
    for n, k, epi in ((32, 64, 0), (64, 16, 0), (64, 64, 7), (64, 64, 2)):  # (epilogue 2 without gamma)
        assert fn(ci(4), ci(n), ci(k), _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), ci(epi), _lib.ptr(None), _lib.ptr(y), _lib.stream_ptr()) == -22
    torch.cuda.synchronize()
    assert not y.any()


# ---- LayerNorm -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [128, 384])
@pytest.mark.parametrize("t", [1, 2, 65, 235])
def test_layernorm_half_is_the_fp32_result_rounded_once(dinov2, c, t):
    """the mean-50 input of test_layernorm_far_from_zero_mean"""
    g = torch.Generator().manual_seed(c + t)
    x = 50.0 + 0.5 * torch.randn(2, t, c, generator=g)
    w, b = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    dx, dw, db = x.to(DEV), w.to(DEV), b.to(DEV)
    y32 = dinov2.layernorm(dx, dw, db, 1e-6)
    y16 = dinov2.layernorm(dx, dw, db, 1e-6, out_dtype=F16)
    assert y16.dtype == F16 and y16.shape == x.shape
    assert torch.equal(bits(y16), bits(y32.half()))
    assert not torch.equal(y16.float(), y32)
    with pytest.raises(ValueError):
        dinov2.layernorm(dx, dw, db, 1e-6, out_dtype=torch.bfloat16)


# ---- attention -------------------------------------------------------------------------------------------------------
def attention_ref64(qkv, heads):
    b, n, _ = qkv.shape
    q, k, v = qkv.double().reshape(b, n, 3, heads, 64).permute(2, 0, 3, 1, 4)
    return R.attention(q, k, v).transpose(1, 2).reshape(b, n, heads * 64)


def qkv_case(heads, t, seed):
    """q, k ~ N(0, 5): logits (q . k) / 8 with a row standard deviation of about 5 (test_dinov2_gpu.py), as fp16 numbers"""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(2, t, 3, heads, 64, generator=g)
    qkv[:, :, :2] *= 5.0 ** 0.5
    return qkv.reshape(2, t, 3 * heads * 64).contiguous().half()


def key_codes(t):
    """code(j) f32[t, 64]: the 11 bits of j, each five times, as +-8 over 55 channels, zeros in the other 9. Two codes differ in
    at least 5 channels, so (code(a) . code(b)) / 8 = 440 - 80 * (bits in which a and b differ)"""
    j = torch.arange(t)
    code = torch.zeros(t, 64)
    for bit in range(11):
        code[:, 5 * bit:5 * bit + 5] = (((j >> bit) & 1).float() * 16.0 - 8.0)[:, None]
    return code


@pytest.mark.parametrize("heads", [2, 6])
@pytest.mark.parametrize("t", T_LIST)
def test_attention_half_selects_the_coded_key(dinov2, heads, t):
    """k_j = code(j) and q_i = code(perm(i)): the true key's logit is 440, every other at most 360, so its weight is 1 and
    exp(-80) of the rest vanishes in fp32 and is 0 in fp16: output row i is v[perm(i)] BIT FOR BIT. Every lane map of both
    products, the key order of the weights' fragments, the transposed values and the tile edges are in this."""
    assert t <= 2048
    g = torch.Generator().manual_seed(17 * heads + t)
    code = key_codes(t)
    logits = code @ code.t() / 8
    assert float(logits.diagonal().min()) == 440.0 and (t == 1 or float((logits - 1e4 * torch.eye(t)).max()) <= 360.0)
    qkv = torch.zeros(2, t, 3, heads, 64)
    perms = torch.stack([torch.stack([torch.randperm(t, generator=g) for _ in range(heads)]) for _ in range(2)])  # [2, heads, t]
    v = torch.randn(2, t, heads, 64, generator=g).half()
    for b in range(2):
        for h in range(heads):
            qkv[b, :, 0, h] = code[perms[b, h]]
            qkv[b, :, 1, h] = code
    qkv[:, :, 2] = v.float()
    out = dinov2.attention_half(qkv.reshape(2, t, -1).half().to(DEV), heads)
    assert out.dtype == F16 and out.shape == (2, t, heads * 64)
    want = torch.stack([torch.stack([v[b, perms[b, h], h] for h in range(heads)], 1) for b in range(2)])  # [2, t, heads, 64]
    assert torch.equal(bits(out), bits(want.reshape(2, t, heads * 64)))


@pytest.mark.parametrize("heads", [2, 6])
@pytest.mark.parametrize("t", T_LIST)
def test_attention_half_against_float64(dinov2, heads, t):
    qkv = qkv_case(heads, t, 100 * heads + t)
    dq = qkv.to(DEV)
    out = dinov2.attention_half(dq, heads)
    held(f"attention_half heads={heads} T={t}", out, attention_ref64(qkv, heads), H.attention_half(qkv, heads).half())
    assert torch.equal(bits(out), bits(dinov2.attention_half(dq, heads)))  # no atomics: the same bits on every run


@pytest.mark.parametrize("heads, t", [(2, 65), (6, 235), (2, 2), (2, 1)])
@pytest.mark.parametrize("fill", [float("nan"), 1e30])
def test_attention_half_padding_has_no_weight(dinov2, heads, t, fill):
    """rows >= n_valid of q, k and v hold NaN / 1e30 (inf in fp16): the valid outputs keep their bits, padded output rows are zeros"""
    pad = 7
    qkv = qkv_case(heads, t, 7 * heads + t)
    padded = torch.full((2, t + pad, qkv.shape[2]), fill).half()
    padded[:, :t] = qkv
    plain = dinov2.attention_half(qkv.to(DEV), heads)
    out = dinov2.attention_half(padded.to(DEV), heads, n_valid=t)
    assert out.shape == (2, t + pad, heads * 64)
    assert torch.equal(bits(out[:, :t]), bits(plain))
    assert torch.equal(bits(out[:, t:]), torch.zeros(2, pad, heads * 64, dtype=torch.int16))


def test_attention_half_peaked_and_flat_rows(dinov2):
    """a key 80 above the rest takes the whole weight without overflow; equal keys give the plain mean of v"""
    heads, t = 2, 65
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(2, t, 3, heads, 64, generator=g)
    qkv[0, :, 0] = 0.0
    qkv[0, :, 0, :, 0] = 8.0
    qkv[0, :, 1, :, 0] = 0.0
    qkv[0, 40, 1, :, 0] = 80.0  # in the second key tile
    qkv[1, :, 1] = qkv[1, 0, 1].clone()
    qkv = qkv.reshape(2, t, -1).contiguous().half()
    out = dinov2.attention_half(qkv.to(DEV), heads)
    held("attention_half peaked / flat", out, attention_ref64(qkv, heads), H.attention_half(qkv, heads).half())
    v = qkv.reshape(2, t, 3, heads, 64)[:, :, 2]
    assert torch.equal(bits(out[0]), bits(v[0, 40].reshape(1, -1).expand(t, -1)))


def test_attention_half_refuses_bad_arguments(dinov2):
    qkv = torch.zeros(1, 4, 3 * 2 * 64, dtype=F16, device=DEV)
    with pytest.raises(ValueError):
        dinov2.attention_half(qkv, 3)
    with pytest.raises(ValueError):
        dinov2.attention_half(qkv, 2, n_valid=5)
    with pytest.raises(ValueError):
        dinov2.attention_half(qkv, 2, n_valid=0)
    with pytest.raises(RuntimeError):
        dinov2.attention_half(qkv.cpu(), 2)
    with pytest.raises(RuntimeError):
        dinov2.attention_half(qkv.float(), 2)


# ---- the whole model -------------------------------------------------------------------------------------------------
def model_held(name, model, x, h64, t64, gates, gate):
    hs, tokens = model.hidden_states(x.to(DEV))
    assert len(hs) == len(h64)
    for i, (a, b, g) in enumerate(zip(hs, h64, gates)):
        err = float((a.double().cpu() - b).abs().max())
        print(f"[{name}] hidden {i} (0 = embeddings): err {err:.3e} gate {g:.3e}")
        assert torch.isfinite(a).all() and err <= g, (name, "hidden state", i, err, g)
    err = float((tokens.double().cpu() - t64).abs().max())
    print(f"[{name}] tokens: err {err:.3e} gate {gate:.3e}, RMS {float(t64.pow(2).mean().sqrt()):.3f}")
    assert tokens.dtype == F32 and torch.isfinite(tokens).all() and err <= gate, (name, err, gate)
    return tokens


@pytest.fixture(scope="module")
def tiny_half(dinov2, gold):
    return dinov2.DinoV2.from_transformers_state_dict(gold["tsd"], precision="fp16").to(DEV)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_tiny_model_half_per_layer(dinov2, tiny_half, gold, name):
    x = gold["cases"][name]["x"]
    tokens = model_held(f"tiny fp16 {name}", tiny_half, x, *H.gate_half(gold["hub"], x))
    out = tiny_half.forward_features(x.to(DEV))
    assert torch.equal(bits(out["x_norm_patchtokens"]), bits(tokens[:, 1:])) and torch.equal(bits(out["x_norm_clstoken"]), bits(tokens[:, 0]))
    assert torch.equal(bits(tiny_half.hidden_states(x.to(DEV))[1]), bits(tokens))
    fp32 = dinov2.DinoV2.from_transformers_state_dict(gold["tsd"]).to(DEV)
    assert not torch.equal(bits(fp32.hidden_states(x.to(DEV))[1]), bits(tokens))  # the mode is not the fp32 path
    # the wrapper that the room pipeline calls: the fp16 grid is these tokens rounded once
    grid = dinov2.feature_fn(tiny_half)(((x * 64.0 + 128.0) / 255.0).to(DEV))
    assert grid.dtype == F16 and grid.shape == (x.shape[0], 128, x.shape[2] // 14, x.shape[3] // 14)


def test_vit_small_half_per_layer(dinov2):
    """ViT-S/14 (384 wide, 12 blocks, 6 heads) with the fixture's weight recipe at 2 x 182 x 252"""
    sd, x = R.random_weights(384, 12, 37, seed=77), R.images(2, 182, 252, seed=78)
    model = dinov2.dinov2_vits14(interpolate_offset=0.0, precision="fp16")
    model.load_state_dict(sd, strict=True)
    model_held("vit-s fp16", model.to(DEV), x, *H.gate_half(sd, x))


def test_range_case_half_is_finite_and_reload_gives_fresh_bits(dinov2, gold):
    """the case of test_range_outlier_channel_and_large_activations: post-GELU reaches about 10 770 (inside fp16) and a residual
    channel sits at 3000 -- the fp32 stream carries it. Then the same model object reloaded with the plain weights gives the
    bits of a fresh model: the fp16 weights follow load_state_dict."""
    sd = {k: v.clone() for k, v in gold["hub"].items()}
    sd["blocks.0.mlp.fc1.weight"] *= 4000.0
    sd["blocks.0.mlp.fc1.bias"] *= 4000.0
    sd["blocks.0.mlp.fc2.weight"] /= 4000.0
    sd["cls_token"][0, 0, 7] += 3000.0
    sd["patch_embed.proj.bias"][7] += 3000.0
    x = gold["cases"]["a"]["x"]
    taps = {}
    hidden, _ = R.forward(sd, x, taps=taps)
    assert 4095 < taps["post_gelu_max"][0] < 65504 and float(hidden[0][..., 7].abs().min()) > 2900
    model = dinov2.DinoV2(embed_dim=128, depth=2, num_heads=2, grid=5, interpolate_offset=0.0, precision="fp16")
    model.load_state_dict(sd, strict=True)
    model.to(DEV)
    ranged = model_held("range fp16", model, x, *H.gate_half(sd, x))
    model.load_state_dict(gold["hub"], strict=True)
    fresh = dinov2.DinoV2(embed_dim=128, depth=2, num_heads=2, grid=5, interpolate_offset=0.0, precision="fp16")
    fresh.load_state_dict(gold["hub"], strict=True)
    again = model.hidden_states(x.to(DEV))[1]
    assert torch.equal(bits(again), bits(fresh.to(DEV).hidden_states(x.to(DEV))[1])) and not torch.equal(bits(again), bits(ranged))


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
def test_half_operators_inside_the_poisoned_arena(arena, dinov2, t):
    g = torch.Generator().manual_seed(t)
    c, heads, rows = 128, 2, 2 * t
    x = 50.0 + 0.5 * torch.randn(2, t, c, generator=g)
    w, b = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    dx, dw, db = arena.put(x), arena.put(w), arena.put(b)
    y = checked(arena, "layernorm fp16", dinov2.layernorm, dx, dw, db, 1e-6, out_dtype=F16)
    assert torch.equal(bits(y), bits(dinov2.layernorm(dx, dw, db, 1e-6).half()))

    qkv = qkv_case(heads, t, t)
    out = checked(arena, "attention_half", dinov2.attention_half, arena.put(qkv), heads)
    held(f"arena attention_half T={t}", out, attention_ref64(qkv, heads), H.attention_half(qkv, heads).half())
    padded = torch.cat([qkv, torch.full((2, 3, qkv.shape[2]), float("nan")).half()], 1)  # 3 padded rows: their outputs are zeros
    outp = checked(arena, "attention_half (padded)", dinov2.attention_half, arena.put(padded), heads, n_valid=t)
    assert torch.equal(bits(outp[:, :t]), bits(out)) and not outp[:, t:].any()

    xm, wm, bm = torch.randn(rows, c, generator=g).half(), (torch.randn(4 * c, c, generator=g) / c ** 0.5).half(), torch.randn(4 * c, generator=g)
    y64 = xm.double() @ wm.double().t() + bm.double()
    dxm, dwm, dbm = arena.put(xm), arena.put(wm), arena.put(bm)
    held(f"arena linear_half bias T={t}", checked(arena, "linear_half", dinov2.linear_half, dxm, dwm, dbm), y64, H.linear_half(xm, wm, bm).half())
    hid = checked(arena, "linear_half gelu", dinov2.linear_half, dxm, dwm, dbm, gelu=True)
    yard_hid = H.linear_half(xm, wm, bm, gelu=True).half()
    held(f"arena linear_half gelu T={t}", hid, R.gelu(y64), yard_hid)
    w2, b2 = (torch.randn(c, 4 * c, generator=g) / (4 * c) ** 0.5).half(), torch.randn(c, generator=g)
    gamma, res = torch.rand(c, generator=g) + 0.5, torch.randn(rows, c, generator=g)
    dres = arena.put(res)
    dinov2.linear_half(hid, arena.put(w2), arena.put(b2), residual=dres, gamma=arena.put(gamma))  # in place: nothing to allocate
    arena.check_guards()
    arena.assert_written(dres, "linear_half residual")
    h16 = hid.cpu()  # (the second layer's own operand: its gate measures this layer alone)
    held(f"arena linear_half residual T={t}", dres, res.double() + gamma.double() * (h16.double() @ w2.double().t() + b2.double()),
         res + gamma * H.linear_half(h16, w2, b2))


@pytest.mark.parametrize("name", ["a", "c"])  # T = 235 and T = 2
def test_forward_features_half_inside_the_poisoned_arena(arena, dinov2, gold, name):
    model = dinov2.DinoV2.from_transformers_state_dict(gold["tsd"], precision="fp16")
    for prm in model.parameters():  # every weight between guards
        prm.data = arena.put(prm.data)
    cache = model.half_weights()  # and every fp16 copy of one
    for key in list(cache):
        cache[key] = arena.put(cache[key])
    assert len(cache) == 8 and model.half_weights() is cache
    x = gold["cases"][name]["x"]
    out = checked(arena, "forward_features fp16", lambda v: tuple(model.forward_features(v).values()), arena.put(x))
    tokens = torch.cat([out[0][:, None], out[1]], 1)
    h64, t64, gates, gate = H.gate_half(gold["hub"], x)
    err = float((tokens.double().cpu() - t64).abs().max())
    print(f"[arena forward fp16 {name}] err {err:.3e} gate {gate:.3e}")
    assert err <= gate
