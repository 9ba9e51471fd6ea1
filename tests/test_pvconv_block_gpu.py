"""One PVConv block (pvcnn_unet.PVConv, models/pvcnn.py:237-334) on every dispatch path of its forward, against a float64
restatement of the block written here: voxelise (mean) -> conv3d -> AdaGN | GroupNorm(8) -> Swish -> conv3d -> AdaGN |
GroupNorm(8) -> [SE3d] -> trilinear devoxelisation, plus the point branch 1x1 conv -> AdaGN | GroupNorm(8) -> Swish.

Paths: the fused inference branch (compact / brick-list sparse / dense convolutions, far-field and plain form, pre-split
operands from the geometry stream and fp32 operands, the three arithmetics of fused.set_conv_math, the joined point branch),
the dense fallback of the resolutions outside {4, 8, 16, 32} (6, 12, 64), and training (forward + every gradient).

The discrete decisions -- the voxel of every point and the eight devoxelisation corners -- come from the product's integer ops
(layers.voxel_coords, avg_voxelize_forward, trilinear_devoxelize_forward), which test_ops_parity_gpu.py and
test_oracle_bruteforce.py pin to the oracle. Every value is then computed in float64 (the corner weights included), so a
rounding flip cannot make a case flaky.

Tolerances: outputs within TOL = 1e-4 of max|ref| AND every output channel within TOL of its own max|ref| (an error confined
to one channel group cannot hide behind the loud channels); gradients by relative L2 per tensor. Every case prints what it
measured (`pytest -rP`).

Measured on an MI355X (worst over the cases; under P2PB_CONV_MATH=f16x3 and =bf16x6 alike), error / max|ref| and worst
per-channel error / that channel's max|ref|:
    inference   r = 4: 7.3e-7 / 1.8e-6   r = 8: 5.4e-6 / 1.4e-5   r = 16: 9.2e-6 / 2.3e-5   r = 32: 4.1e-6 / 1.4e-5
                r = 6: 5.3e-7 / 1.6e-6   r = 12: 1.9e-6 / 2.7e-6  r = 64: 5.1e-6 / 1.3e-5
    training    output <= 1.2e-6 / 1.7e-6; gradients (relative L2): r = 8, 16, 32: <= 6.0e-6 (bf16x6: the same), r = 12: 1.4e-5,
                r = 64: 3.9e-5 except the second convolution's weight, 2.0e-3 (7.7e-5 of the sum of |terms|, see ABS_SUM_TOL).
    "cube" clouds (CUBE_CASES: all 8 corner voxels of the grid occupied), r = 8 / 16 / 32: <= 1.4e-6 / 2.9e-6
Wall time of the 55 tests before CUBE_CASES on an MI355X: 11 s (the 12 cube cases add 3 s) with torch's convolution kernels already compiled, about 30 s when the r = 64
training case has to compile them first."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
TOL = 1e-4
GRAD_TOL = 5e-4  # relative L2 per gradient tensor (measured worst: 3.9e-5)

MATHS = ("f16x3", "bf16x6", "fp32")
CHANNELS = ((3, 8), (19, 40), (64, 64), (35, 128))  # not multiples of 16; both sides of the cout > 32 wide tiling
CLOUDS = ("surface", "one_voxel", "plane")
COMPACT = (None, "", "32,16:16")  # P2PB_EXPERIMENT compact=: default, off, both resolutions


# r = 16 / 32: (arithmetic, SE, compact plan, sparse_conv, geometry stream) per case. Each compact plan meets sparse_conv under a
# split arithmetic; the compact form runs with (f16x3 + geometry stream: pre-split operands) and without pre-split operands at both
# resolutions (r = 32: plan "32,16:16" -- compact first convolution, plain second one); sparse_conv off meets a split arithmetic
WIDE_SLOTS = (("f16x3", True, "32,16:16", True, True), ("f16x3", False, None, True, False), ("bf16x6", True, "32,16:16", True, False),
              ("bf16x6", False, "", True, True), ("fp32", True, None, True, True), ("fp32", False, "32,16:16", False, False),
              ("f16x3", True, "", False, True), ("f16x3", False, None, True, True), ("f16x3", True, "32,16:16", True, False))


def _cases():
    """every r x arithmetic x SE combination at least once; at r = 16 / 32 the WIDE_SLOTS, elsewhere the other axes cycle; the
    remaining axes cycle so that each of their values meets r = 16 and r = 32"""
    out = []
    for r in (4, 8, 16, 32, 6, 12, 64):
        if r in (16, 32):
            for j, (math, se, compact, sparse, geo) in enumerate(WIDE_SLOTS):
                ch = CHANNELS[(j + r // 16) % 4]
                out.append(dict(r=r, math=math, se=se, cin=ch[0], cout=ch[1], cond=(j + 1) % 3 != 0, sparse=sparse, compact=compact,
                                B=(1, 3)[j // 2 % 2], N=(1000, 2048)[j % 2], cloud=CLOUDS[(j + r) % 3], geo=geo))
            continue
        for j in range(6):
            math, se = MATHS[j // 2], j % 2 == 0
            # (the fp64 reference of the big grids stays cheap: narrow layers only)
            ch = CHANNELS[j % 2] if r >= 12 else CHANNELS[(j + 2) % 4]
            out.append(dict(r=r, math=math, se=se, cin=ch[0], cout=ch[1], cond=(j + 1) % 3 != 0,
                            sparse=(j // 2 + j) % 2 == 0, compact=COMPACT[j % 3], B=(1, 3)[(j // 3 + j) % 2],
                            N=(1000, 2048)[(j + 1) // 2 % 2], cloud=CLOUDS[(j + r) % 3], geo=j % 3 != 1))
    return out


def _compact_runs(c):
    """does the case's block take the compact (voxel-level sparse) convolutions (pvcnn_unet.compact_plan)?"""
    plan = {None: "16:16", "": "", "32,16:16": "32,16:16"}[c["compact"]]
    first, second = ({int(t) for t in q.split(",") if t} for q in (plan.split(":") + [""])[:2])
    return c["sparse"] and c["math"] != "fp32" and (c["r"] in first or c["r"] in second)


CASES = _cases()
assert {(c["r"], c["math"], c["se"]) for c in CASES} == {(r, m, se) for r in (4, 8, 16, 32, 6, 12, 64) for m in MATHS for se in (True, False)}
for _r in (16, 32):  # every value of every other axis meets r = 16 and r = 32: checked where the list is made
    _sub = [c for c in CASES if c["r"] == _r]
    for _k, _vals in (("cond", (True, False)), ("sparse", (True, False)), ("compact", COMPACT), ("B", (1, 3)), ("N", (1000, 2048)),
                      ("cloud", CLOUDS), ("geo", (True, False))):
        assert {c[_k] for c in _sub} == set(_vals), (_r, _k)
    assert {(c["cin"], c["cout"]) for c in _sub} == set(CHANNELS), _r
    for _v in COMPACT:  # each compact plan changes what runs: it meets sparse_conv under a split arithmetic
        assert any(c["compact"] == _v and c["sparse"] and c["math"] != "fp32" for c in _sub), (_r, _v)
    assert any(not c["sparse"] and c["math"] != "fp32" for c in _sub), _r
    # the compact form itself, with pre-split operands (f16x3 + geometry stream) and without
    assert any(_compact_runs(c) and c["math"] == "f16x3" and c["geo"] for c in _sub), _r
    assert any(_compact_runs(c) and not (c["math"] == "f16x3" and c["geo"]) for c in _sub), _r
    assert any(_compact_runs(c) and c["math"] == "bf16x6" for c in _sub), _r


# Appended: a cloud that fills the grid out to its 8 corner voxels (`_cloud` "cube": uniform in [-1, 1]^3, normalize=False, plus
# four points at every corner). A normalised cloud lies inside the inscribed sphere, so the cases above never occupy an edge or a
# corner voxel and their compact convolutions compute outputs of the interior and the face boundary classes only. Compact plan
# at the case's own r for both convolutions; f16x3 with the geometry stream (pre-split operands), bf16x6 without; SE on and off.
CUBE_CASES = [dict(r=r, math=math, se=se, cin=CHANNELS[(j + r // 8) % 4][0], cout=CHANNELS[(j + r // 8) % 4][1], cond=j % 2 == 0,
                   sparse=True, compact=f"{r}:{r}", B=(3, 1)[j // 2 % 2], N=2048, cloud="cube", geo=math == "f16x3")
              for r in (8, 16, 32) for j, (math, se) in enumerate((m, s) for m in ("f16x3", "bf16x6") for s in (True, False))]


def _cid(c):
    return (f"r{c['r']}-{c['math']}-{'se' if c['se'] else 'nose'}-{c['cin']}x{c['cout']}-{'adagn' if c['cond'] else 'gn'}"
            f"-{'sparse' if c['sparse'] else 'dense'}-compact{'default' if c['compact'] is None else (c['compact'] or 'off')}"
            f"-B{c['B']}N{c['N']}-{c['cloud']}{'-geo' if c['geo'] else ''}")


# ------------------------------------------------------------------------------------------------- inputs and the block

E = 16  # cond_dim of the AdaGN cases


def _cloud(kind, B, N, gen):
    """(coords f32[B,3,N], normalize): a noisy sphere, every point in the centre voxel (normalize=False: centred, not
    rescaled), a flat plane"""
    if kind == "surface":
        p = torch.randn(B, 3, N, generator=gen, dtype=torch.float64)
        p = p / p.norm(dim=1, keepdim=True) + 0.01 * torch.randn(B, 3, N, generator=gen, dtype=torch.float64)
        return p.float(), True
    if kind == "one_voxel":
        return (0.3 + 1e-3 * torch.rand(B, 3, N, generator=gen, dtype=torch.float64)).float(), False
    if kind == "cube":  # the whole grid, its 8 corner voxels included: 4 points at +-(1 - 1e-3) per axis each
        p = torch.rand(B, 3, N, generator=gen, dtype=torch.float64) * 2 - 1
        signs = torch.tensor([[1.0 if (q >> a) & 1 else -1.0 for q in range(8)] for a in range(3)], dtype=torch.float64)
        p[:, :, :32] = (signs * (1 - 1e-3)).repeat(1, 4)
        return p.float(), False
    p = torch.rand(B, 3, N, generator=gen, dtype=torch.float64) * 2 - 1
    p[:, 2] = 0.25
    return p.float(), True


def _block(cin, cout, r, se, cond, normalize, dropout, seed):
    from p2p_bridge_amd.pvcnn_unet import PVConv

    torch.manual_seed(seed)
    blk = PVConv(cin, cout, r, with_se=se, dropout=dropout, cond_dim=E if cond else 0, normalize=normalize)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():  # the norms' affine parameters away from (1, 0), so that a swapped / dropped one shows
        for name, p in blk.named_parameters():
            if name.endswith(("norm.weight", "norm.bias")) or (name.split(".")[-2] in ("1", "5") and "emd" not in name):
                p.add_(0.3 * torch.randn(p.shape, generator=gen))
    return blk.cuda()


def _inputs(c, gen):
    coords, normalize = _cloud(c["cloud"], c["B"], c["N"], gen)
    feats = torch.randn(c["B"], c["cin"], c["N"], generator=gen)
    cond = torch.randn(c["B"], E, generator=gen) if c["cond"] else None
    return coords.cuda(), normalize, feats.cuda(), None if cond is None else cond.cuda()


# ------------------------------------------------------------------------------------------------- the float64 restatement


def _decisions(coords, r, normalize):
    """the discrete part, from the product's integer ops: (norm coords f32[B,3,N], ind i64[B,N], cnt i64[B,r^3],
    corner ids i64[B,8,N])"""
    from p2p_bridge_amd import layers as L
    from p2p_bridge_amd import pointnet2_batch_cuda as ext

    B, _, N = coords.shape
    vc, vox = L.voxel_coords(coords.contiguous(), r, normalize, 0.0)
    _, ind, cnt = ext.avg_voxelize_forward(torch.zeros(B, 1, N, device=coords.device), vox.contiguous(), r)
    _, inds, wgts = ext.trilinear_devoxelize_forward(r, True, vc.contiguous(), torch.zeros(B, 1, r ** 3, device=coords.device))
    return vc, ind.long(), cnt.long(), inds.long(), wgts


def _corner_weights(vc):
    """f64[B,8,N] trilinear weights of the corners in the order of the corner ids (x major, z minor; 0 = low side)"""
    x = vc.double()
    d1 = x - torch.floor(x)
    d0 = 1.0 - d1
    w = []
    for q in range(8):
        ax = [(d1 if (q >> (2 - a)) & 1 else d0)[:, a] for a in range(3)]
        w.append(ax[0] * ax[1] * ax[2])
    return torch.stack(w, 1)


def _conv3d(x, w, b):
    """3x3x3 correlation, zero padding 1, as 27 shifted channel products"""
    r = x.shape[2]
    xp = F.pad(x, (1, 1, 1, 1, 1, 1))
    y = b.view(1, -1, 1, 1, 1).expand(x.shape[0], -1, r, r, r)
    for i in range(3):
        for j in range(3):
            for k in range(3):
                y = y + torch.einsum("oc,bcxyz->boxyz", w[:, :, i, j, k], xp[:, :, i:i + r, j:j + r, k:k + r])
    return y


def _group_norm(x, w, b, groups=8, eps=1e-5):
    B, C = x.shape[:2]
    g = x.reshape(B, groups, -1)
    mu = g.mean(-1, keepdim=True)
    var = ((g - mu) ** 2).mean(-1, keepdim=True)
    y = ((g - mu) / torch.sqrt(var + eps)).reshape(x.shape)
    shape = (1, C) + (1,) * (x.dim() - 2)
    return y * w.view(shape) + b.view(shape)


def _norm(p, pre, x, cond):
    B, C = x.shape[:2]
    shape = (B, C) + (1,) * (x.dim() - 2)
    if pre + ".emd.weight" in p:  # AdaGN: GroupNorm, then the per-sample factor / bias of a Linear on cond
        y = _group_norm(x, p[pre + ".norm.weight"], p[pre + ".norm.bias"])
        style = cond @ p[pre + ".emd.weight"].t() + p[pre + ".emd.bias"]
        return y * style[:, :C].reshape(shape) + style[:, C:].reshape(shape)
    return _group_norm(x, p[pre + ".weight"], p[pre + ".bias"])


def _swish(x):
    return x * torch.sigmoid(x)


def _reference(p, feats, cond, dec, r, keep=None):
    """PVConv forward from the parameters `p` (name -> tensor) in the dtype of `feats` (float64; float32 for comparison, printed
    by _train_case)"""
    vc, ind, cnt, inds, _ = dec
    B, C, N = feats.shape
    grid = torch.zeros(B, C, r ** 3, dtype=feats.dtype, device=feats.device)
    grid = grid.scatter_add(2, ind[:, None, :].expand(B, C, N), feats)
    grid = (grid / cnt.clamp(min=1)[:, None, :].to(feats.dtype)).view(B, C, r, r, r)
    v = _conv3d(grid, p["voxel_layers.0.weight"], p["voxel_layers.0.bias"])
    if keep is not None:  # (the convolutions' operands and outputs, for _wgrad_scale)
        keep["voxel_layers.0.weight"] = (grid, v)
        v.retain_grad()
    v = _swish(_norm(p, "voxel_layers.1", v, cond))
    x4 = v
    v = _conv3d(v, p["voxel_layers.4.weight"], p["voxel_layers.4.bias"])
    if keep is not None:
        keep["voxel_layers.4.weight"] = (x4, v)
        v.retain_grad()
    v = _norm(p, "voxel_layers.5", v, cond)
    if "voxel_layers.6.fc.0.weight" in p:
        s = v.mean((2, 3, 4))
        s = torch.sigmoid(torch.relu(s @ p["voxel_layers.6.fc.0.weight"].t()) @ p["voxel_layers.6.fc.2.weight"].t())
        v = v * s[:, :, None, None, None]
    flat = v.reshape(B, -1, r ** 3)
    Co = flat.shape[1]
    w = _corner_weights(vc).to(feats.dtype)
    dv = 0
    for q in range(8):
        dv = dv + w[:, q][:, None, :] * flat.gather(2, inds[:, q][:, None, :].expand(B, Co, N))
    pt = torch.einsum("oc,bcn->bon", p["point_features.layers.0.weight"][:, :, 0], feats) + p["point_features.layers.0.bias"][None, :, None]
    pt = _swish(_norm(p, "point_features.layers.1", pt, cond))
    return dv + pt


def _params64(blk, grad=False, dtype=torch.float64):
    return {k: v.detach().to(dtype).requires_grad_(grad) for k, v in blk.named_parameters()}


def _check_out(out, ref, what):
    """-> (error / max|ref|, worst per-channel error / that channel's max|ref|), asserted below TOL"""
    out, ref = out.double(), ref.detach()
    assert torch.isfinite(out).all(), what
    err = (out - ref).abs()
    glob = err.max().item() / ref.abs().max().item()
    per = (err.amax((0, 2)) / ref.abs().amax((0, 2)).clamp(min=1e-30)).max().item()
    assert glob < TOL, (what, glob)
    assert per < TOL, (what, per)
    return glob, per


def _rel_l2(a, b, scale=None):
    """||a - b|| / ||b|| (or / max(||b||, ||scale||))"""
    den = b.double().norm() if scale is None else torch.maximum(b.double().norm(), scale.double().norm())
    return ((a.double() - b.double()).norm() / den.clamp(min=1e-30)).item()


# a convolution's bias in front of a GroupNorm only moves its group's mean: with 8 channels (one per group) its exact gradient
# is 0 and a relative error has no meaning -- it is measured against the gradient of the same layer's weight there
# r = 64 trains on the dense fallback, whose weight gradients come from torch's convolution, not from the project's kernels:
# fp32 sums over every voxel of every sample, B r^3 = 262144 terms, whose rounding error grows with the number and the absolute
# values of the terms (the restatement's own fp32 evaluation is 1e-5 of sum |terms| away from fp64 there, 1e-8 at r <= 32).
# THERE ONLY (r outside FUSED_RESOLUTIONS) a weight gradient beyond GRAD_TOL is measured against sum |terms| (_wgrad_scale);
# measured worst 7.7e-5 (r = 64, second convolution). Every weight gradient of the HIP kernels (r <= 32) is held to GRAD_TOL.
ABS_SUM_TOL = 2e-4
PRE_NORM_BIAS = ("voxel_layers.0.bias", "voxel_layers.4.bias", "point_features.layers.0.bias")


def _wgrad_scale(x, dy):
    """sum over samples and voxels of |dy[o]| |x[c] shifted by the tap|: the sum of the absolute values of the terms of the
    convolution's weight gradient -- the scale of the rounding error of any fp32 evaluation of that sum (|fl(s) - s| grows
    with sum |terms|, not with |s|)"""
    r = x.shape[2]
    xp = F.pad(x.abs(), (1, 1, 1, 1, 1, 1))
    dy = dy.abs()
    out = torch.empty(dy.shape[1], x.shape[1], 3, 3, 3, dtype=x.dtype, device=x.device)
    for i in range(3):
        for j in range(3):
            for k in range(3):
                out[:, :, i, j, k] = torch.einsum("boxyz,bcxyz->oc", dy, xp[:, :, i:i + r, j:j + r, k:k + r])
    return out


def _restatement(blk, feats, cond, dec, r, gy, dtype):
    """-> (output, {name: gradient}) of the restatement in `dtype`, autograd"""
    p = _params64(blk, grad=True, dtype=dtype)
    f = feats.detach().to(dtype).requires_grad_(True)
    cd = None if cond is None else cond.detach().to(dtype).requires_grad_(True)
    keep = {}
    out = _reference(p, f, cd, dec, r, keep)
    out.backward(gy.to(dtype))
    grads = {"features": f.grad}
    for name, (x, y) in keep.items():
        grads[name + ":scale"] = _wgrad_scale(x.detach(), y.grad)
    if cd is not None:
        grads["cond"] = cd.grad
    grads.update({k: v.grad for k, v in p.items()})
    return out.detach(), grads


# ------------------------------------------------------------------------------------------------- inference


def _geometry(coords, r, normalize):
    """the coordinate-only preparation of the network's geometry stream for this one block at level 0"""
    from p2p_bridge_amd.pvcnn_unet import Geometry

    return Geometry({"voxel": [(0, r, normalize, 0.0)], "sa": [], "fp": []}, coords, torch.cuda.Stream())


@pytest.mark.parametrize("c", CASES + CUBE_CASES, ids=_cid)
def test_pvconv_block_inference(c, monkeypatch):
    """eval() + no_grad: the fused branch for r in {4, 8, 16, 32}, the dense fallback for the others -- vs float64"""
    from p2p_bridge_amd import _experiment, fused
    from p2p_bridge_amd.pvcnn_unet import PVCData

    if c["compact"] is not None:
        monkeypatch.setenv("P2PB_EXPERIMENT", _experiment.setting(compact=c["compact"]))
    gen = torch.Generator().manual_seed(1000 + c["r"] * 7 + c["cout"])
    coords, normalize, feats, cond = _inputs(c, gen)
    blk = _block(c["cin"], c["cout"], c["r"], c["se"], c["cond"], normalize, 0.1, seed=c["r"] + c["cin"])
    blk.sparse_conv = c["sparse"]
    blk.eval()
    prev = fused._conv_math_override  # (set_conv_math returns the resolved name: restoring that would pin it process-wide)
    fused.set_conv_math(c["math"])
    try:
        with torch.no_grad():
            data = PVCData(features=feats, coords=coords, cond=cond)
            if c["geo"]:
                blk.level = 0
                data.geo = _geometry(coords, c["r"], normalize)
            out = blk(data).features
            if c["geo"]:
                torch.cuda.current_stream().wait_event(data.geo.join)
            torch.cuda.synchronize()
    finally:
        fused.set_conv_math(prev)
    dec = _decisions(coords, c["r"], normalize)
    assert (_corner_weights(dec[0]) - dec[4].double()).abs().max().item() < 1e-6  # (the kernel's own fp32 weights)
    if c["cloud"] == "cube":
        r = c["r"]
        corners = [(d * r + h) * r + w for d in (0, r - 1) for h in (0, r - 1) for w in (0, r - 1)]
        assert (dec[2][:, corners] > 0).all(), "a corner voxel of the grid is empty"
    with torch.no_grad():
        ref = _reference(_params64(blk), feats.double(), None if cond is None else cond.double(), dec, c["r"])
    assert out.shape == ref.shape == (c["B"], c["cout"], c["N"])
    glob, per = _check_out(out, ref, _cid(c))
    print(f"MEASURED {_cid(c)} out {glob:.2e} per-channel {per:.2e}")


# ------------------------------------------------------------------------------------------------- training

TRAIN_CASES = [dict(r=8, cin=19, cout=40, B=3, N=2048, cloud="surface", cond=True),
               dict(r=16, cin=35, cout=128, B=2, N=1000, cloud="plane", cond=True),
               dict(r=32, cin=64, cout=64, B=3, N=2048, cloud="surface", cond=False),
               dict(r=12, cin=3, cout=8, B=3, N=1000, cloud="one_voxel", cond=True),
               dict(r=64, cin=19, cout=40, B=1, N=2048, cloud="surface", cond=True)]


def _train_run(c, train_math=None, monkeypatch=None):
    """-> (block, feats, cond, product output, upstream gradient) after forward + backward in train() mode, dropout p = 0"""
    from p2p_bridge_amd.pvcnn_unet import PVCData

    if train_math is not None:
        monkeypatch.setenv("P2PB_TRAIN_MATH", train_math)
    gen = torch.Generator().manual_seed(2000 + c["r"])
    coords, normalize, feats, cond = _inputs(dict(c), gen)
    blk = _block(c["cin"], c["cout"], c["r"], True, c["cond"], normalize, 0.0, seed=50 + c["r"])
    blk.train()
    feats.requires_grad_(True)
    if cond is not None:
        cond.requires_grad_(True)
    gy = torch.randn(c["B"], c["cout"], c["N"], generator=gen).cuda()
    out = blk(PVCData(features=feats, coords=coords, cond=cond)).features
    out.backward(gy)
    torch.cuda.synchronize()
    return blk, coords, normalize, feats, cond, out.detach(), gy


def _train_case(c, train_math=None, monkeypatch=None, grad_tol=GRAD_TOL):
    from p2p_bridge_amd.pvcnn_unet import FUSED_RESOLUTIONS

    blk, coords, normalize, feats, cond, out, gy = _train_run(c, train_math, monkeypatch)
    dec = _decisions(coords, c["r"], normalize)
    ref, g64 = _restatement(blk, feats, cond, dec, c["r"], gy, torch.float64)
    _, g32 = _restatement(blk, feats, cond, dec, c["r"], gy, torch.float32)
    worst = {"out": _check_out(out, ref, c)}
    mine = {"features": feats.grad, "cond": None if cond is None else cond.grad}
    mine.update({k: v.grad for k, v in blk.named_parameters()})
    bad, rows = {}, []
    for name, ref_g in g64.items():
        if name.endswith(":scale"):
            continue
        g = mine[name]
        assert g is not None and ref_g is not None, name
        scale = g64[name[:-len("bias")] + "weight"] if (name in PRE_NORM_BIAS and c["cout"] == 8) else None
        err, err32 = _rel_l2(g, ref_g, scale), _rel_l2(g32[name], ref_g, scale)
        rows.append((err, err32, name))
        if not err < grad_tol:
            # (torch's convolution on the dense fallback, a long fp32 sum: ABS_SUM_TOL)
            sc = g64.get(name + ":scale") if c["r"] not in FUSED_RESOLUTIONS else None
            if sc is None or not _rel_l2(g, ref_g, sc) < ABS_SUM_TOL:
                bad[name] = (err, None if sc is None else _rel_l2(g, ref_g, sc))
    err, err32, name = max(rows)
    for w in ("voxel_layers.0.weight", "voxel_layers.4.weight"):
        print(f"MEASURED train r{c['r']} {w} against sum |terms| {_rel_l2(mine[w], g64[w], g64[w + ':scale']):.2e} "
              f"(fp32 restatement {_rel_l2(g32[w], g64[w], g64[w + ':scale']):.2e})")
    print(f"MEASURED train r{c['r']} out {worst['out'][0]:.2e} per-channel {worst['out'][1]:.2e} worst grad {name} {err:.2e} "
          f"(fp32 restatement {err32:.2e})")
    assert not bad, bad
    return worst


@pytest.mark.parametrize("c", TRAIN_CASES, ids=lambda c: f"r{c['r']}-{c['cin']}x{c['cout']}-{c['cloud']}")
def test_pvconv_block_training(c):
    """train(), dropout p = 0, default P2PB_TRAIN_MATH: output and the gradients of the features, cond and every parameter vs
    float64 autograd of the restatement. r = 64 takes the devoxelisation gradient's global-atomic kernel (rows beyond the LDS)"""
    _train_case(c)


def test_pvconv_block_training_bf16x6(monkeypatch):
    """the same under P2PB_TRAIN_MATH=bf16x6 (fp32-faithful data and weight gradients)"""
    _train_case(dict(TRAIN_CASES[2], cond=True), "bf16x6", monkeypatch)


def test_pvconv_block_r64_deterministic_refuses():
    """under p2p_bridge_amd.deterministic() the r = 64 devoxelisation gradient has no fixed-order kernel: a clear error, no
    output"""
    import p2p_bridge_amd

    with p2p_bridge_amd.deterministic():
        with pytest.raises(RuntimeError, match="deterministic"):
            _train_run(TRAIN_CASES[4])
