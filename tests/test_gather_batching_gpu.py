"""The point-major gather / scatter-back kernels of the sampler's critical stream issue their independent loads per batch
(csrc/neighbors.hip group_stats_kernel, group_sub_kernel, three_interp_add_kernel; csrc/devoxelize.hip devox_cl_kernel,
devox_cl4_kernel; from the audit of the other small kernels: csrc/voxel_gather.hip vox_gather_cl_split_kernel, far_field_kernel and the SE3d
bottleneck se_hidden of pvconv_tail_kernel / se_gate_affine_kernel: profiles/r07_gather_wait_audit.txt). Only the ORDER OF
THE LOADS may differ from the kernels before that change: every output bit is held to what the previous kernels wrote,
recorded once by tools/make_golden_gather_tails.py (run on the GPU with the library of the commit before the change) in
tests/golden/gather_tails.npz.

Shapes are the smallest at which batching can go wrong, not the workload's: ragged batches (m*u = 56, 96, 160 against slots
of 128 and tiles of 64 positions), masked steps (positions >= m*u, channels >= c in a ragged channel block of either
template), clamped addresses (n = 1, 63, 65, 130 against 64-point tiles; points on the grid's faces).

The file stores the GroupNorm partials in full and every large tensor as the SHA-256 of its bytes (equal digests = equal
bits): the full tensors of all cases are about 9 MB, too much for a fixture. group_stats and group_sub
have a second, independent witness: a NumPy float32 loop in the documented summation order."""
import hashlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gather_tails.npz")

GS_B, GS_N = 2, 40
GS_MU = [(3, 32), (4, 32), (5, 32), (24, 4), (2, 64), (7, 8)]  # m*u = 96, 128, 160 (partial last slot), 96, 128, 56
GS_C = [8, 32, 40, 64, 72]  # both templates (c <= 32: two positions per step), a ragged channel block in each
TI_B, TI_M = 2, 5
TI_N = [1, 63, 64, 65, 130]
TI_C = [3, 64, 72, 128]
DV_B = 2
DV_R = [4, 8]
DV_N = [1, 63, 65, 130]
DV_C = [3, 35, 64, 128]  # devox_cl (3, 35) and devox_cl4 (64, 128; devox_cl there: test_voxel_switch_arms_gpu.py)
VG_B, VG_R = 2, 4  # 64 voxels: the one-pass split gather runs where a cloud has more than a quarter point per voxel
VG_N = [20, 130, 257]  # empty voxels, voxels of 1 .. 67 points: ragged and whole batches of four points
VG_C = [4, 12, 36, 64]  # multiples of 4 (16-byte rows), ragged against the 8-channel thread and the 16-channel chunk
FF_B = 2
FF_CI = [3, 32, 35, 64, 100]  # 0, 4, 4 + ragged, 8, 12 + ragged chunks of eight input channels (whole chunks go four at a time)
FF_CO = [16, 40]
SE_B = 2
SE_C = [8, 64, 200, 576, 1032]  # a lane's 1, 1, 4 (ragged), 9, 17 terms: inside one batch of eight, two, three


def _digest(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8).copy()


def _full(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- seeded inputs (NumPy generators: the same values on every machine) ----
def gs_inputs(m, u, c):
    rng = np.random.default_rng(1000 * m + 10 * u + c)
    zt = rng.standard_normal((GS_B, GS_N, c)).astype(np.float32)
    cxt = (0.5 * rng.standard_normal((GS_B, m, c))).astype(np.float32)
    idx = rng.integers(0, GS_N, size=(GS_B, m, u)).astype(np.int32)
    idx[:, 0, 0] = 0
    idx[:, 0, 1] = GS_N - 1
    idx[:, -1, -1] = GS_N - 1
    idx[:, -1, 0] = idx[:, -1, 1]  # a repeat inside one centre's neighbourhood (the small cloud repeats many more)
    return zt, cxt, idx


def ti_inputs(n, c):
    rng = np.random.default_rng(7000 + 10 * n + c)
    czt = rng.standard_normal((TI_B, TI_M, c)).astype(np.float32)
    idx = rng.integers(0, TI_M, size=(TI_B, 3, n)).astype(np.int32)
    w = rng.random((TI_B, 3, n)).astype(np.float32) + np.float32(0.05)
    w = (w / w.sum(axis=1, keepdims=True)).astype(np.float32)
    add = rng.standard_normal((TI_B, c, n)).astype(np.float32)
    bias = (0.3 * rng.standard_normal(c)).astype(np.float32)
    return czt, idx, w, add, bias


def dv_inputs(r, n, c):
    rng = np.random.default_rng(90000 + 1000 * r + 10 * n + c)
    grid = rng.standard_normal((DV_B, r, r, r, c)).astype(np.float32)
    co = (rng.random((DV_B, 3, n)) * (r - 1)).astype(np.float32)
    # points on the grid's faces and on voxel centres: integer coordinates, 0 and r - 1 (clamped upper corners)
    co[:, :, 0] = r - 1
    if n > 3:
        co[:, :, 1] = 0.0
        co[:, 0, 2] = r - 1
        co[:, 1, 3] = np.floor(co[:, 1, 3])
        co[:, 2, n - 1] = r - 1
        co[:, 0, n - 2] = 0.0
    co = np.minimum(co, np.float32(r - 1))
    a = (1.0 + 0.3 * rng.standard_normal((DV_B, c))).astype(np.float32)
    bb = (0.2 * rng.standard_normal((DV_B, c))).astype(np.float32)
    h = (2.0 * rng.standard_normal((DV_B, c, n))).astype(np.float32)
    hs = (1.0 + 0.3 * rng.standard_normal((DV_B, c))).astype(np.float32)
    hb = (0.2 * rng.standard_normal((DV_B, c))).astype(np.float32)
    return grid, co, a, bb, h, hs, hb


def vg_inputs(n, c):
    rng = np.random.default_rng(50000 + 10 * n + c)
    feat = rng.standard_normal((VG_B, c, n)).astype(np.float32)
    vox = rng.integers(0, VG_R, size=(VG_B, 3, n)).astype(np.int32)
    if n > 64:  # some voxels crowded (more than eight points), some left empty
        vox[:, :, : n // 4] = vox[:, :, :1]
        vox[0][:, vox[0, 0] == VG_R - 1] = 0
    return feat, vox


def ff_inputs(ci, co):
    rng = np.random.default_rng(60000 + 100 * ci + co)
    w = (rng.standard_normal((co, ci, 3, 3, 3)) / np.sqrt(27.0 * ci)).astype(np.float32)
    bias = (0.1 * rng.standard_normal(co)).astype(np.float32)
    prev_bias = (0.3 * rng.standard_normal(ci)).astype(np.float32)
    sc = (1.0 + 0.3 * rng.standard_normal((FF_B, ci))).astype(np.float32)
    sh = (0.2 * rng.standard_normal((FF_B, ci))).astype(np.float32)
    return w, bias, prev_bias, sc, sh


def se_inputs(c):
    rng = np.random.default_rng(70000 + c)
    hidden = max(1, c // 8)
    mean = rng.standard_normal((SE_B, c)).astype(np.float32)
    w1 = (rng.standard_normal((hidden, c)) / np.sqrt(c)).astype(np.float32)
    w2 = (rng.standard_normal((c, hidden)) / np.sqrt(hidden)).astype(np.float32)
    sc = (1.0 + 0.3 * rng.standard_normal((SE_B, c))).astype(np.float32)
    sh = (0.2 * rng.standard_normal((SE_B, c))).astype(np.float32)
    part = rng.standard_normal((SE_B, 4, c, 2)).astype(np.float32)  # {sum, sum of squares} partials of 4 slots x 16 values
    part[..., 1] = 16.0 + 4.0 * np.abs(part[..., 1])
    gamma = (1.0 + 0.3 * rng.standard_normal(c)).astype(np.float32)
    beta = (0.2 * rng.standard_normal(c)).astype(np.float32)
    return mean, w1, w2, sc, sh, part, gamma, beta


# ---- the operators over their grids: {key: array} ----
def compute_group_stats():
    from p2p_bridge_amd import fused

    out = {}
    for m, u in GS_MU:
        for c in GS_C:
            zt, cxt, idx = (_dev(x) for x in gs_inputs(m, u, c))
            for use_cx in (0, 1):
                _, st = fused.group_sub(zt, cxt if use_cx else None, idx, point_major=True, stats_only=True)
                out[f"group_stats/m{m}_u{u}_c{c}_cx{use_cx}/stats"] = _full(st)
    return out


def compute_group_sub():
    from p2p_bridge_amd import fused

    out = {}
    for m, u in GS_MU:
        for c in GS_C:
            zt, cxt, idx = (_dev(x) for x in gs_inputs(m, u, c))
            for use_cx in (0, 1):
                y, st = fused.group_sub(zt, cxt if use_cx else None, idx, point_major=True)
                k = f"group_sub/m{m}_u{u}_c{c}_cx{use_cx}"
                out[k + "/out"] = _digest(y)
                out[k + "/stats"] = _full(st)
    return out


def compute_three_interp_add():
    from p2p_bridge_amd import fused

    out = {}
    for n in TI_N:
        for c in TI_C:
            czt, idx, w, add, bias = (_dev(x) for x in ti_inputs(n, c))
            for use_add in (0, 1):
                for use_bias in (0, 1):
                    y, st = fused.interp_add(czt, idx, w, add if use_add else None, bias if use_bias else None, point_major=True)
                    k = f"three_interp_add/n{n}_c{c}_add{use_add}_bias{use_bias}"
                    out[k + "/out"] = _digest(y)
                    out[k + "/stats"] = _full(st)
    return out


def compute_devox():
    from p2p_bridge_amd.fused import call, ptr, stream_ptr

    out = {}
    for r in DV_R:
        for n in DV_N:
            for c in DV_C:
                grid, co, a, bb, h, hs, hb = (_dev(x) for x in dv_inputs(r, n, c))
                for use_aff in (0, 1):
                    for use_add in (0, 1):
                        y = torch.empty(DV_B, c, n, dtype=torch.float32, device="cuda")
                        # (the entry point itself: fused.devoxelize_affine always passes the affine)
                        call("p2pb_trilinear_devoxelize_cl_affine", DV_B, c, n, r, ptr(co), ptr(grid),
                             ptr(a if use_aff else None), ptr(bb if use_aff else None), ptr(h if use_add else None),
                             ptr(hs if use_add else None), ptr(hb if use_add else None), ptr(y), stream_ptr())
                        out[f"devox/r{r}_n{n}_c{c}_aff{use_aff}_add{use_add}/out"] = _digest(y)
    torch.cuda.synchronize()
    return out


def compute_vox_gather_split():
    from p2p_bridge_amd import fused

    out = {}
    for n in VG_N:
        for c in VG_C:
            feat, vox = (_dev(x) for x in vg_inputs(n, c))
            cnt, ws = fused.voxel_sort(vox, VG_R)
            out[f"vox_gather_split/n{n}_c{c}/out"] = _full(fused.voxelize_cl_gather(feat, cnt, ws, VG_R, split=True))
    return out


def compute_far_field():
    from p2p_bridge_amd import fused

    out = {}
    for ci in FF_CI:
        for co in FF_CO:
            w, bias, prev_bias, sc, sh = ff_inputs(ci, co)
            conv = torch.nn.Conv3d(ci, co, 3, padding=1)
            with torch.no_grad():
                conv.weight.copy_(torch.from_numpy(w))
                conv.bias.copy_(torch.from_numpy(bias))
            a, k = fused.conv3d_far_field(_dev(prev_bias), conv.cuda(), _dev(sc), _dev(sh))
            out[f"far_field/ci{ci}_co{co}/a"] = _full(a)
            out[f"far_field/ci{ci}_co{co}/k"] = _full(k)
    return out


def compute_se_gate():
    from p2p_bridge_amd import fused

    out = {}
    for c in SE_C:
        mean, w1, w2, sc, sh, part, gamma, beta = (_dev(x) for x in se_inputs(c))
        a, b = fused.se_gate_affine(mean, w1, w2, sc, sh)
        out[f"se_gate/c{c}/affine"] = _full(torch.stack([a, b]))
        a, b, _, _ = fused.pvconv_tail(part, (64.0, 8, gamma, beta, None, 1e-5, False), se=(w1, w2))
        out[f"se_gate/c{c}/tail"] = _full(torch.stack([a, b]))
    return out


def compute_all():
    out = {}
    for f in (compute_group_stats, compute_group_sub, compute_three_interp_add, compute_devox, compute_vox_gather_split,
              compute_far_field, compute_se_gate):
        out.update(f())
    return out


# ---- against the recorded bits ----
@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN_FILE) as z:
        return {k: z[k] for k in z.files}


def _check(computed, golden, prefix, expected_count):
    want = sorted(k for k in golden if k.startswith(prefix + "/"))
    assert sorted(computed) == want and len(want) == expected_count
    bad = [k for k in want if not torch.equal(torch.from_numpy(computed[k]), torch.from_numpy(golden[k]))]
    assert not bad, f"{len(bad)} of {len(want)} outputs differ from the recorded bits, first: {bad[:6]}"


def test_group_stats_bits(golden):
    _check(compute_group_stats(), golden, "group_stats", len(GS_MU) * len(GS_C) * 2)


def test_group_sub_bits(golden):
    _check(compute_group_sub(), golden, "group_sub", len(GS_MU) * len(GS_C) * 2 * 2)


def test_three_interp_add_bits(golden):
    _check(compute_three_interp_add(), golden, "three_interp_add", len(TI_N) * len(TI_C) * 4 * 2)


def test_devox_bits(golden):
    _check(compute_devox(), golden, "devox", len(DV_R) * len(DV_N) * len(DV_C) * 4)


def test_vox_gather_split_bits(golden):
    _check(compute_vox_gather_split(), golden, "vox_gather_split", len(VG_N) * len(VG_C))


def test_far_field_bits(golden):
    _check(compute_far_field(), golden, "far_field", len(FF_CI) * len(FF_CO) * 2)


def test_se_gate_bits(golden):
    _check(compute_se_gate(), golden, "se_gate", len(SE_C) * 2)


# ---- the second witness: NumPy float32 in the documented order ----
def _np_group_stats(zt, cxt, idx, m, u, c):
    """csrc/neighbors.hip group_stats_kernel: slots of 128 positions, every channel adds {v, v * v} (v = z[idx] - cx, separate
    float32 multiply and add) in ascending position order; c <= 32: even and odd positions of the slot apart, then even + odd"""
    mu = m * u
    nslots = (mu + 127) // 128
    st = np.zeros((GS_B, nslots, c, 2), np.float32)
    flat = idx.reshape(GS_B, mu)
    for b in range(GS_B):
        for s in range(nslots):
            lanes = 2 if c <= 32 else 1
            s1 = np.zeros((lanes, c), np.float32)
            s2 = np.zeros((lanes, c), np.float32)
            for pl in range(128):
                p = s * 128 + pl
                if p >= mu:
                    continue
                v = zt[b, flat[b, p]]
                if cxt is not None:
                    v = v - cxt[b, p // u]
                h = pl % lanes
                s1[h] = s1[h] + v
                s2[h] = s2[h] + v * v
            st[b, s, :, 0] = s1[0] + s1[1] if lanes == 2 else s1[0]
            st[b, s, :, 1] = s2[0] + s2[1] if lanes == 2 else s2[0]
    return st


@pytest.mark.parametrize("m,u", GS_MU)
def test_group_stats_numpy_order(m, u):
    from p2p_bridge_amd import fused

    for c in GS_C:
        zt, cxt, idx = gs_inputs(m, u, c)
        for use_cx in (0, 1):
            _, st = fused.group_sub(_dev(zt), _dev(cxt) if use_cx else None, _dev(idx), point_major=True, stats_only=True)
            want = _np_group_stats(zt, cxt if use_cx else None, idx, m, u, c)
            assert torch.equal(st.cpu(), torch.from_numpy(want)), (m, u, c, use_cx)


def test_group_sub_numpy_values():
    """the stored tensor is one exact float32 subtraction per element: z[idx] - cx"""
    from p2p_bridge_amd import fused

    for m, u in GS_MU:
        for c in GS_C:
            zt, cxt, idx = gs_inputs(m, u, c)
            flat = idx.reshape(GS_B, m * u)
            for use_cx in (0, 1):
                y, _ = fused.group_sub(_dev(zt), _dev(cxt) if use_cx else None, _dev(idx), point_major=True)
                want = np.stack([zt[b, flat[b]] for b in range(GS_B)])  # [b, mu, c]
                if use_cx:
                    want = want - np.repeat(cxt, u, axis=1)
                assert torch.equal(y.cpu(), torch.from_numpy(np.ascontiguousarray(want.transpose(0, 2, 1)))), (m, u, c, use_cx)
