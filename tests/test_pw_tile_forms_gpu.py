"""The wide forms of the split-operand 1x1 GEMM (csrc/pointwise_split.hip): pw_split_kernel<WM=4> and the ping-pong
kernel of csrc/pw_pp512.h -- which production only picks for grids of >= 1024 workgroups --
forced here on small shapes: ragged channel / position counts, an odd number of 128-channel blocks, the folded operand
transform, both pooling epilogues and the statistics, against float64 references of the same layer
(models/pvcnn.py:162-205 SharedMLP, :414 neighbour max, :923,930 Pnet2Stage pools). The choice is read once per process,
hence subprocesses."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CODE = r"""
import sys, torch
sys.path.insert(0, %r)
from p2p_bridge_amd import fused
torch.manual_seed(0)
def swish(x): return x * torch.sigmoid(x)
for (B, ci, co, P, u) in [(2, 512, 1024, 512, 0), (3, 128, 384, 1000, 0), (2, 256, 512, 2048, 32), (1, 160, 300, 260, 0),
                          (2, 1024, 256, 128, 8)]:
    x = torch.randn(B, ci, P, device="cuda")
    conv = torch.nn.Conv1d(ci, co, 1).cuda()
    sc, sh = torch.rand(B, ci, device="cuda") + 0.5, torch.randn(B, ci, device="cuda")
    bias_b = torch.randn(B, co, device="cuda")
    with torch.no_grad():
        xin = swish(x.double() * sc[:, :, None].double() + sh[:, :, None].double())
        ref = torch.nn.functional.conv1d(xin, conv.weight.double(), conv.bias.double()) + bias_b[:, :, None].double()
        scale = ref.abs().max().item()
        y, st = fused.pw_conv(x, conv, sc, sh, swish=True, bias_b=bias_b)
        assert (y.double() - ref).abs().max().item() < 1e-5 * scale, "output"
        s = st.double().sum(1)
        assert (s[..., 0] - ref.sum(2)).abs().max().item() < 1e-4 * scale * P ** 0.5 + 1e-3, "sum"
        assert ((s[..., 1] - (ref * ref).sum(2)).abs() / (ref * ref).sum(2)).max().item() < 1e-5, "sumsq"
        plain = torch.nn.functional.conv1d(x.double(), conv.weight.double(), conv.bias.double())
        y0, _ = fused.pw_conv(x, conv, stats=False)
        assert (y0.double() - plain).abs().max().item() < 1e-5 * plain.abs().max().item(), "plain"
        if fused.pool_supported(P, u):
            _, st, mm = fused.pw_conv(x, conv, sc, sh, swish=True, bias_b=bias_b, pool_u=u, store=False)
            if u == 0:
                mn, mx = mm[..., 0].min(1).values.double(), mm[..., 1].max(1).values.double()
                assert (mn - ref.min(2).values).abs().max().item() < 1e-5 * scale and (mx - ref.max(2).values).abs().max().item() < 1e-5 * scale
            else:
                g = ref.view(B, co, P // u, u)
                assert (mm[..., 0].double() - g.min(3).values).abs().max().item() < 1e-5 * scale
                assert (mm[..., 1].double() - g.max(3).values).abs().max().item() < 1e-5 * scale
print("TILE-FORMS-OK")
""" % ROOT


@pytest.mark.parametrize("pp", ["1", "0"])
def test_256_channel_forms(pp):
    """pp = 1 (default): shapes with whole 512-channel blocks and an even stage count take the ping-pong kernel
    (pw_pp512.h), the others pw_split_kernel<WM = 4>; pp = 0: pw_split_kernel for all"""
    env = dict(os.environ, P2PB_EXPERIMENT=f"pw_wm=4;pw_pp={pp}")
    r = subprocess.run([sys.executable, "-c", CODE], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "TILE-FORMS-OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


P5_CODE = r"""
import sys, ctypes, torch
sys.path.insert(0, %r)
from p2p_bridge_amd import fused, _lib
torch.manual_seed(2)
def swish(x): return x * torch.sigmoid(x)
def form(ci, co, P):
    return _lib.lib().p2pb_debug_pointwise_form(ci, co, P, None)
# (B, cin, cout, P, transform): 4 .. 16 stages, 1 .. 3 channel blocks of 512, whole and RAGGED position tiles (P %% 128 != 0, down to
# a single partial tile), odd grid sizes
for (B, ci, co, P, xf) in [(1, 128, 512, 128, "swish"), (3, 128, 512, 768, "affine"), (2, 512, 1024, 2048, "swish"),
                           (5, 192, 1536, 256, "none"), (2, 256, 512, 1284, "swish"), (1, 128, 1024, 60, "affine"),
                           (2, 512, 1024, 12500, "swish"), (1, 320, 512, 1000, "none")]:
    x = torch.randn(B, ci, P, device="cuda") * 3
    conv = torch.nn.Conv1d(ci, co, 1).cuda()
    sc, sh = torch.rand(B, ci, device="cuda") + 0.5, torch.randn(B, ci, device="cuda")
    bias_b = torch.randn(B, co, device="cuda")
    with torch.no_grad():
        xin = x.double()
        if xf != "none":
            xin = xin * sc[:, :, None].double() + sh[:, :, None].double()
        if xf == "swish":
            xin = swish(xin)
        ref = torch.nn.functional.conv1d(xin, conv.weight.double(), conv.bias.double()) + bias_b[:, :, None].double()
        mag = torch.nn.functional.conv1d(xin.abs(), conv.weight.double().abs()) + conv.bias.double().abs()[None, :, None] + bias_b[:, :, None].double().abs()
        args = (x, conv) if xf == "none" else (x, conv, sc, sh)
        kw = dict(bias_b=bias_b, swish=(xf == "swish")) if xf != "none" else dict(bias_b=bias_b)
        y, st = fused.pw_conv(*args, **kw)
        assert form(ci, co, P) == 5, ("the ping-pong form did not run", ci, co, P, form(ci, co, P))
        assert ((y.double() - ref).abs() / mag).max().item() < 2e-6, ("output", B, ci, co, P)
        nslots = (P + 255) // 256 * 4
        assert st.shape[1] == nslots
        # statistics per 128 positions = a pair of 64-position slots (sums in the even slot, zero in the odd one; extrema in
        # both); slots past the last tile are zero. The tail tile's columns >= P contribute nothing.
        T = nslots // 2
        pad = T * 128 - P
        rp = torch.nn.functional.pad(ref, (0, pad)).view(B, co, T, 128)
        mp = torch.nn.functional.pad(mag, (0, pad)).view(B, co, T, 128) + 1e-30
        s = st.double().view(B, T, 2, co, 2).sum(2)
        assert ((s[..., 0] - rp.sum(3).transpose(1, 2)).abs() / (mp.sum(3).transpose(1, 2) + 1e-30)).max().item() < 2e-6, "slot sums"
        q = (rp * rp).sum(3).transpose(1, 2)
        assert ((s[..., 1] - q).abs() / (q + 1e-30)).max().item() < 1e-5, "slot sumsq"
        _, st2, mm = fused.pw_conv(*args, pool_u=0, store=False, **kw)
        assert torch.equal(st2, st), "statistics with / without the stored output"
        T2 = (P + 127) // 128
        assert mm.shape[1] == 2 * T2
        mm = mm.view(B, T2, 2, co, 2)
        assert torch.equal(mm[:, :, 0], mm[:, :, 1])
        pad2 = T2 * 128 - P
        rmin = torch.nn.functional.pad(ref, (0, pad2), value=float("inf")).view(B, co, T2, 128).min(3).values.transpose(1, 2)
        rmax = torch.nn.functional.pad(ref, (0, pad2), value=float("-inf")).view(B, co, T2, 128).max(3).values.transpose(1, 2)
        mmax = torch.nn.functional.pad(mag, (0, pad2)).view(B, co, T2, 128).max(3).values.transpose(1, 2)
        assert ((mm[:, :, 0, :, 0].double() - rmin).abs() / mmax).max().item() < 2e-6
        assert ((mm[:, :, 0, :, 1].double() - rmax).abs() / mmax).max().item() < 2e-6
        for _ in range(3):  # deterministic: the hand-counted waits and the raw barriers leave no race
            y2, st3 = fused.pw_conv(*args, **kw)
            assert torch.equal(y2, y) and torch.equal(st3, st)
        # out of range is loud here too, and stays inside its column
        if P > 6:
            xb = x.clone(); xb[0, 3, 5] = float("nan")
            yb, _ = fused.pw_conv(*((xb,) + args[1:]), **kw)
            assert not torch.isfinite(yb[0, :, 5]).any() and torch.equal(yb[:, :, :5], y[:, :, :5]) and torch.equal(yb[0, :, 6:], y[0, :, 6:])
print("PP512-OK")
""" % ROOT


def test_pp512_kernel_shapes():
    """pw_pp512_kernel (round 4: 512 channels x 128 positions per workgroup) on its own shape family, ragged position counts
    included (PVDL's 12500-point level): every output against float64 with per-element bounds, per-slot statistics and
    extrema, zeroed / masked tails, run-to-run identical; the form table confirms the kernel ran"""
    if os.environ.get("P2PB_CONV_MATH", "f16x3") != "f16x3":
        pytest.skip("pw_pp512_kernel exists in the f16x3 arithmetic only")
    env = dict(os.environ, P2PB_EXPERIMENT="pw_wm=4;pw_pp=1")
    r = subprocess.run([sys.executable, "-c", P5_CODE], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "PP512-OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


def _swish(x):
    return x * torch.sigmoid(x)


def _layer64(x, conv, sc, sh, bias_b):
    """float64 reference of one folded layer, sample by sample (the largest row's output is 268 MB in float64)"""
    w, bias = conv.weight.double().flatten(1), conv.bias.double()
    for b in range(x.shape[0]):
        xin = _swish(x[b].double() * sc[b, :, None].double() + sh[b, :, None].double())
        yield b, w @ xin + (bias + bias_b[b].double())[:, None]


def test_dispatch_table(monkeypatch):
    """Which kernel form each kind of layer takes in production -- no P2PB_EXPERIMENT: the library reads pw_wm / pw_pp once
    per process --, read back from the form table after every call (csrc/common.h P2PB_FORM_PW_*; the choice is made in
    csrc/pointwise.hip pw_run / pw_run_split), and every row's output against float64 with test_256_channel_forms' bound
    (1e-5 of the output's scale), so that the right kernel with the wrong arguments fails too.
    Forms 2, 5 and 6 (pw_wide_kernel on the split pack, pw_pp512_kernel, the gathered operand) exist in the f16x3 arithmetic
    only: under P2PB_CONV_MATH=bf16x6 the rows that expect 5 run pw_split_kernel<WM = 4> (4) and the rows that expect 2 or 6
    are left out. 192 -> 512 is in whole 64-channel stages (192 = 3 * 64), so at 1024 workgroups it takes the ping-pong kernel;
    160 -> 512 is the layer that qualifies for 256-channel workgroups and not for ping-pong (cin % 64 != 0)."""
    from p2p_bridge_amd import fused, _lib
    f16 = os.environ.get("P2PB_CONV_MATH", "f16x3") == "f16x3"
    pp = 5 if f16 else 4
    monkeypatch.setattr(fused, "PW_SPLIT_MIN_CIN", 64)  # lets pw_conv put the 64 -> 512 rows on the split pack (flags 4)
    form = lambda ci, co, P: _lib.lib().p2pb_debug_pointwise_form(ci, co, P, None)  # noqa: E731
    torch.manual_seed(3)
    rows = [  # (B, cin, cout, P, keywords of pw_conv, expected form)
        (1, 8, 8, 30, dict(math="fp32"), 0),             # fp32 pack, rows not in whole quads
        (1, 8, 8, 32, dict(math="fp32"), 1),             # fp32 pack, 16-byte rows
        (1, 16, 8, 32, dict(), 2),                       # flags 4 | 128
        (1, 128, 128, 256, dict(), 3),
        (8, 160, 512, 8192, dict(), 4),                  # exactly 1024 workgroups of 128 x 256; cin % 64 != 0
        (7, 160, 512, 8192, dict(), 3),                  # 896 workgroups
        (8, 192, 512, 8192, dict(), pp),
        (7, 192, 512, 8192, dict(), 3),
        (8, 64, 512, 8192, dict(), pp),
        (8, 64, 512, 8192, dict(pool_u=32), 4),          # ping-pong has only the global pool
        (8, 64, 512, 8192, dict(point_major=True, stats=False), 3),
    ]
    with torch.no_grad():
        for (B, ci, co, P, kw, want) in rows:
            if want == 2 and not f16:
                continue
            _lib.lib().p2pb_debug_pointwise_form(-1, 0, 0, None)
            x = torch.randn(B, ci, P, device="cuda")
            conv = torch.nn.Conv1d(ci, co, 1).cuda()
            sc, sh = torch.rand(B, ci, device="cuda") + 0.5, torch.randn(B, ci, device="cuda")
            bias_b = torch.randn(B, co, device="cuda")
            res = fused.pw_conv(x, conv, sc, sh, swish=True, bias_b=bias_b, **kw)
            assert form(ci, co, P) == want, (B, ci, co, P, kw, form(ci, co, P))
            y = res[0].transpose(1, 2) if kw.get("point_major") else res[0]
            err = mmerr = scale = 0.0
            for b, ref in _layer64(x, conv, sc, sh, bias_b):
                scale = max(scale, ref.abs().max().item())
                err = max(err, (y[b].double() - ref).abs().max().item())
                if "pool_u" in kw:
                    g = ref.view(co, P // kw["pool_u"], kw["pool_u"])
                    mmerr = max(mmerr, (res[2][b, ..., 0].double() - g.min(2).values).abs().max().item(),
                                (res[2][b, ..., 1].double() - g.max(2).values).abs().max().item())
            assert err < 1e-5 * scale and mmerr < 1e-5 * scale, (B, ci, co, P, kw, err, mmerr, scale)
        if f16:  # the gather entry point: operand[ci, (m, u)] = zt[idx[m, u], ci] - cxt[m, ci], only {min, max} over u come out
            B, ci, co, n, m, u = 2, 8, 16, 16, 4, 4
            _lib.lib().p2pb_debug_pointwise_form(-1, 0, 0, None)
            zt, cxt = torch.randn(B, n, ci, device="cuda"), torch.randn(B, m, ci, device="cuda")
            idx = torch.randint(0, n, (B, m, u), device="cuda", dtype=torch.int32)
            conv = torch.nn.Conv1d(ci, co, 1).cuda()
            sc, sh = torch.rand(B, ci, device="cuda") + 0.5, torch.randn(B, ci, device="cuda")
            _, mm = fused.pw_conv_pool_gather(zt, cxt, idx, conv, sc, sh, swish=True)
            assert form(ci, co, m * u) == 6, form(ci, co, m * u)
            grouped = torch.stack([zt[b][idx[b].long()] for b in range(B)]) - cxt[:, :, None, :]  # [B, m, u, ci]
            x = grouped.permute(0, 3, 1, 2).reshape(B, ci, m * u)
            for b, ref in _layer64(x, conv, sc, sh, torch.zeros(B, co, device="cuda")):
                g, scale = ref.view(co, m, u), ref.abs().max().item()
                assert (mm[b, ..., 0].double() - g.min(2).values).abs().max().item() < 1e-5 * scale
                assert (mm[b, ..., 1].double() - g.max(2).values).abs().max().item() < 1e-5 * scale
