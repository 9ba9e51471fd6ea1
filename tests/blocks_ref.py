"""Plain-torch restatement of the three composite blocks of the network besides PVConv (test infrastructure, no HIP):

    sa_block      PointNetSAModule  (models/pvcnn.py:337-424, BallQuery.forward :99-127)
    fp_block      PointNetFPModule  (models/pvcnn.py:427-467, the time-embedding concat of models/unet_pvc.py:254-256)
    pnet2_stage   Pnet2Stage        (models/pvcnn.py:803-932, MyGroupNorm :745-763)

Every function computes in the dtype of its floating inputs (the tests hand float64) from a parameter dict `params` whose
keys are the module's own `named_parameters()` names. The discrete decisions -- which points are centres, which points are
a centre's neighbours, which three coarse points a fine point interpolates from -- are INPUTS (index tensors), taken by the
tests from the product's integer ops, which test_ops_parity_gpu.py and test_oracle_bruteforce.py pin to the oracle: a
rounding flip cannot change what is compared. tests/test_blocks_ref.py pins this file to oracle/net_ref.py on the CPU.
"""
import torch


def swish(x):
    return x * torch.sigmoid(x)


def group_norm(x, w, b, groups, eps=1e-5):
    """GroupNorm over x[B, C, ...] with biased variance, affine (w, b) per channel"""
    B, C = x.shape[:2]
    g = x.reshape(B, groups, -1)
    mu = g.mean(-1, keepdim=True)
    var = ((g - mu) ** 2).mean(-1, keepdim=True)
    y = ((g - mu) / torch.sqrt(var + eps)).reshape(x.shape)
    shape = (1, C) + (1,) * (x.dim() - 2)
    return y * w.view(shape) + b.view(shape)


def norm(p, pre, x, cond, groups=8):
    """AdaGN (GroupNorm, then the per-sample factor / bias of a Linear on cond: models/modules.py:341-358) when the
    parameters hold one under `pre`, plain GroupNorm otherwise"""
    B, C = x.shape[:2]
    if pre + ".emd.weight" in p:
        y = group_norm(x, p[pre + ".norm.weight"], p[pre + ".norm.bias"], groups)
        style = cond @ p[pre + ".emd.weight"].t() + p[pre + ".emd.bias"]
        shape = (B, C) + (1,) * (x.dim() - 2)
        return y * style[:, :C].reshape(shape) + style[:, C:].reshape(shape)
    return group_norm(x, p[pre + ".weight"], p[pre + ".bias"], groups)


def conv1x1(x, w, b):
    """k = 1 convolution on x[B, Ci, ...]: w [Co, Ci(, 1(, 1))], b [Co]"""
    w = w.reshape(w.shape[0], -1)
    y = torch.einsum("oc,bc...->bo...", w, x)
    return y + b.view((1, -1) + (1,) * (x.dim() - 2))


def shared_mlp(p, pre, x, cond, groups=8, keep=None):
    """(1x1 conv -> AdaGN | GroupNorm -> Swish) for every conv `pre.layers.{3i}` in p (models/pvcnn.py:162-205).
    keep (dict): receives "pre_act" = what the LAST Swish is applied to"""
    i = 0
    while f"{pre}.layers.{3 * i}.weight" in p:
        x = conv1x1(x, p[f"{pre}.layers.{3 * i}.weight"], p[f"{pre}.layers.{3 * i}.bias"])
        x = norm(p, f"{pre}.layers.{3 * i + 1}", x, cond, groups)
        if keep is not None:
            keep["pre_act"] = x
        x = swish(x)
        i += 1
    assert i > 0, pre
    return x


def _take(x, idx):
    """x[B, C, N], idx int[B, ...] -> x[b, :, idx[b, ...]] as [B, C, ...]"""
    B, C = x.shape[:2]
    flat = idx.reshape(B, 1, -1).long().expand(B, C, -1)
    return x.gather(2, flat).reshape(B, C, *idx.shape[1:])


def sa_block(features, coords, time_emb, cond, params, centers_idx, nidx, groups=8, keep=None):
    """features [B,C,N] | None, coords [B,3,N], time_emb [B,E,N] | None, cond [B,D] | None, centers_idx int[B,M],
    nidx int[B,M,U] -> (pooled features [B,Cout,M], centres [B,3,M], time_emb[:, :, :M] | None).
    keep (dict): receives "pre_act" = what the last Swish is applied to, [B,Cout,M,U] (`min_share`)"""
    centers = _take(coords, centers_idx)
    rel = _take(coords, nidx) - centers.unsqueeze(-1)
    grouped = rel if features is None else torch.cat([rel, _take(features, nidx)], dim=1)
    y = shared_mlp(params, "mlps.0", grouped, cond, groups, keep)
    M = centers.shape[-1]
    return y.max(dim=-1).values, centers, None if time_emb is None else time_emb[:, :, :M]


def three_nn_weights(coords, lower_coords, idx3):
    """the interpolation weights [B,3,N] of the three coarse points idx3 int[B,3,N]: inverse squared distances, the
    squared distance clamped to [1e-10, 1e10], normalised (PN2/pvcnn_neighbor_interpolate_gpu.cu:67-75: d1 d2 / (d0 d1 +
    d0 d2 + d1 d2) and its two permutations = (1 / d_k) / sum_j (1 / d_j)), from the float32 coordinates in float64. A fine
    point that IS a coarse point (every level is a subset of the one above) has d = 0 -> 1e-10: weight 1 to ~1e-9"""
    d2 = ((coords.double().unsqueeze(2) - _take(lower_coords.double(), idx3)) ** 2).sum(1)  # [B,3,N]
    w = 1.0 / d2.clamp(1e-10, 1e10)
    return w / w.sum(1, keepdim=True)


def fp_block(coords, skip, lower_coords, lower_features, lower_temb, cond, params, idx3, groups=8):
    """coords [B,3,N], skip [B,Cs,N] | None, lower_coords [B,3,M], lower_features [B,Cg,M], lower_temb [B,E] | None (the
    time embedding the network concatenates to the coarse features before the interpolation), idx3 int[B,3,N]
    -> features [B,Cout,N]"""
    g = lower_features
    if lower_temb is not None:
        g = torch.cat([g, lower_temb.unsqueeze(-1).expand(-1, -1, g.shape[-1])], dim=1)
    w = three_nn_weights(coords, lower_coords, idx3).to(g.dtype)
    x = (_take(g, idx3) * w.unsqueeze(1)).sum(2)
    if skip is not None:
        x = torch.cat([x, skip], dim=1)
    return shared_mlp(params, "mlp", x, cond, groups)


def _pnet_mlp(p, pre, x, keep, groups=32):
    """one conv -> MyGroupNorm(32) -> Swish: the norm covers the first C - C % 32 channels, the rest pass through"""
    x = conv1x1(x, p[pre + ".mlp.0.weight"], p[pre + ".mlp.0.bias"])
    w = p[pre + ".mlp.1.group_norm.weight"]
    nc = w.shape[0]
    assert nc == x.shape[1] - x.shape[1] % groups
    x = torch.cat([group_norm(x[:, :nc], w, p[pre + ".mlp.1.group_norm.bias"], groups), x[:, nc:]], dim=1)
    if keep is not None:
        keep[pre.split(".")[0]] = x
    return swish(x)


def _cond_mlp(p, pre, x, keep):
    """ConditionedSharedMLPLayer without time / cond / residual; keep[pre] = what its last Swish is applied to"""
    x = _pnet_mlp(p, pre + ".shared_mlp_1", _pnet_mlp(p, pre + ".shared_mlp_0", x, None), keep)
    i = 0
    while f"{pre}.last_mlp_layers.{i}.mlp.0.weight" in p:
        x = _pnet_mlp(p, f"{pre}.last_mlp_layers.{i}", x, keep)
        i += 1
    return x


def pnet2_stage(coords, params, keep=None):
    """coords [B,3,N] -> the global conditioning vector [B,C]: mlp1, max over the points, concat of the broadcast maximum,
    mlp2, max over the points. keep (dict): receives "mlp1" / "mlp2" = what the last Swish in front of each of the two
    maxima is applied to, [B,C,N] (`min_share`)"""
    f = _cond_mlp(params, "mlp1", coords, keep)
    g = f.max(dim=-1, keepdim=True).values
    h = _cond_mlp(params, "mlp2", torch.cat([f, g.expand(-1, -1, f.shape[-1])], dim=1), keep)
    return h.max(dim=-1).values


def min_share(pre_act):
    """pre_act [..., K]: the values the last Swish is applied to (after the norm's affine). -> the share of rows (all
    leading axes) with swish(min) > swish(max), i.e. whose pooled value comes from the row MINIMUM -- the rows on which a
    kernel that pooled the maximum pre-activation alone would be wrong"""
    lo, hi = pre_act.min(dim=-1).values, pre_act.max(dim=-1).values
    return (swish(lo) > swish(hi)).double().mean().item()
