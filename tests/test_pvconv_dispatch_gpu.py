"""WHICH library entry points a PVConv's inference forward runs, in order, with the integers that select a kernel form.

Every convolution form of the fused voxel branch (compact, brick lists, dense; far-field or plain second convolution; pre-split
or fp32 operand) computes the same function, and tests/test_pvconv_block_gpu.py holds each of them to float64 -- so a dispatch
edit that sent r = 16 to the dense kernel, or dropped `listed_only`, would pass there and only make the sampler slower. Here the
forward of one block runs with a recording proxy in place of the loaded library (p2p_bridge_amd._lib._lib) and the record is
compared with the literal TABLE below.

What is compared per call (`_digest`): the entry point's name, its `swish` / `flags` integers, WHICH optional operands were
handed over (a pointer that is null or not: `+in_scale`, `+in_sub`, `+out_class`, `+style`, `+se`, `+point`, ...), and for the
list-driven convolutions `which` list they read, derived from the list pointer's offset in the tensor that
p2pb_conv3d_active_lists / p2pb_conv3d_brick_lists filled just before. Sizes are not compared: the table pins no shape. Host
queries (`*_floats`, `*_bytes`, `p2pb_get_split_terms`, ...) are left out.

TABLE was recorded from the hand-written dispatch code this test was added to guard, before that code was rewritten around
pvcnn_unet.voxel_conv_plan; it is NOT computed from the plan. A deliberate change of a default (compact plan, pre-split plan) or a
new launch on this path changes it: re-record with `pytest -rP` (every case prints its digest) and review the difference."""
import ctypes

import pytest
import torch

from test_pvconv_block_gpu import _block, _cloud, _geometry

pytestmark = pytest.mark.gpu


def _case(r, math="f16x3", geo=True, compact=None, sparse=True, se=True, cond=True, pin=None):
    return dict(r=r, math=math, geo=geo, compact=compact, sparse=sparse, se=se, cond=cond, pin=pin)


CASES = (
    # the defaults, with the geometry stream (lists and pre-split operands come from it) and without
    [_case(r, geo=g) for r in (4, 8, 16, 32) for g in (True, False)]
    # no pre-split operands outside f16x3; no compact form under fp32
    + [_case(r, math=m) for m in ("bf16x6", "fp32") for r in (16, 32)]
    # compact plans: off; first convolution compact and second one plain (norm_affine between them); r = 8
    + [_case(16, compact=""), _case(32, compact="32,16:16"), _case(8, compact="8:8")]
    + [_case(r, sparse=False) for r in (16, 32)]
    # SE / AdaGN change the arguments of pvconv_tail, far_field_gn and gn_affine_params only
    + [_case(16, se=False), _case(16, cond=False), _case(32, se=False, cond=False), _case(8, se=False, cond=False)]
    # a layer pinned to another arithmetic takes its operand as fp32, the other one stays pre-split
    + [_case(16, pin=0), _case(16, pin=4)])


def _cid(c):
    return (f"r{c['r']}-{c['math']}-{'geo' if c['geo'] else 'nogeo'}-compact{'default' if c['compact'] is None else (c['compact'] or 'off')}"
            f"-{'sparse' if c['sparse'] else 'dense'}-{'se' if c['se'] else 'nose'}-{'adagn' if c['cond'] else 'gn'}"
            + ("" if c["pin"] is None else f"-pin{c['pin']}"))


class Recorder:
    """stands in for the ctypes library: every function called through it is logged as (name, [("i", int) | ("p", address | None)
    | ("x", None) per argument]) and then run"""

    def __init__(self, real):
        self._real, self.log = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def wrapped(*args):
            row = []
            for a in args:
                if isinstance(a, (ctypes.c_int, ctypes.c_long)):
                    row.append(("i", int(a.value)))
                elif isinstance(a, int):
                    row.append(("i", a))
                elif isinstance(a, ctypes.c_void_p):
                    row.append(("p", a.value))
                else:
                    row.append(("x", None))
            self.log.append((name, row))
            return fn(*args)

        return wrapped


def record(monkeypatch, fn):
    """run fn() with the recording proxy in place of the loaded library -> (fn's result, the log)"""
    from p2p_bridge_amd import _lib

    rec = Recorder(_lib.lib())
    with monkeypatch.context() as mp:  # (undone on failure too)
        mp.setattr(_lib, "_lib", rec)
        out = fn()
        torch.cuda.synchronize()
    return out, rec.log


def run_case(c, monkeypatch):
    """-> (output of the block, log): a fresh PVConv(16 -> 32) in eval mode on one cloud of 256 points; the geometry stream's
    preparation (pvcnn_unet.Geometry) is part of the record"""
    from p2p_bridge_amd import _experiment, fused
    from p2p_bridge_amd.pvcnn_unet import PVCData

    if c["compact"] is not None:
        monkeypatch.setenv("P2PB_EXPERIMENT", _experiment.setting(compact=c["compact"]))
    gen = torch.Generator().manual_seed(77)
    coords, normalize = _cloud("surface", 1, 256, gen)
    feats = torch.randn(1, 16, 256, generator=gen).cuda()
    cond = torch.randn(1, 16, generator=gen).cuda() if c["cond"] else None
    coords = coords.cuda()
    blk = _block(16, 32, c["r"], c["se"], c["cond"], normalize, 0.1, seed=5)
    blk.sparse_conv = c["sparse"]
    blk.eval()
    if c["pin"] is not None:
        fused.pin_layer_math(blk.voxel_layers[c["pin"]], "bf16x6")
    prev = fused._conv_math_override
    fused.set_conv_math(c["math"])

    def forward():
        with torch.no_grad():
            data = PVCData(features=feats, coords=coords, cond=cond)
            if c["geo"]:
                blk.level = 0
                data.geo = _geometry(coords, c["r"], normalize)
            out = blk(data).features
            if c["geo"]:
                torch.cuda.current_stream().wait_event(data.geo.join)
        return out

    try:
        return record(monkeypatch, forward)
    finally:
        fused.set_conv_math(prev)


# entry point -> ({index among the integer arguments: label}, {index among the pointer arguments: label of an optional operand})
_CONV = ({4: "swish", 5: "flags"}, {3: "out_class", 4: "in_scale", 6: "in_sub"})
SPEC = {
    "p2pb_conv3d_k3_forward_ex": _CONV, "p2pb_conv3d_k3_forward_sparse": _CONV, "p2pb_conv3d_k3_forward_compact": _CONV,
    "p2pb_conv3d_k3_forward_compact_pre": ({4: "flags"}, {3: "out_class"}),
    "p2pb_conv3d_presplit": ({3: "swish"}, {1: "in_scale", 3: "in_sub"}),
    "p2pb_conv3d_k3_far_field_gn": ({6: "swish"}, {4: "style"}),
    "p2pb_gn_affine_params": ({}, {3: "style", 6: "chmean"}),
    "p2pb_pvconv_tail": ({}, {3: "style", 4: "se", 8: "point"}),
    "p2pb_trilinear_devoxelize_cl_affine": ({}, {4: "add"}),
    "p2pb_pointwise_conv_forward": ({4: "swish", 5: "flags"}, {4: "in_scale"}),
    "p2pb_set_split_terms_thread": ({0: "terms"}, {}),
}
# the list operand of the list-driven convolutions (index among the pointer arguments) and the call that filled the tensor it
# points into (index of that tensor among ITS pointer arguments)
LIST_ARG = {"p2pb_conv3d_k3_forward_sparse": (7, "p2pb_conv3d_brick_lists", 2), "p2pb_conv3d_k3_forward_compact": (7, "p2pb_conv3d_active_lists", 1),
            "p2pb_conv3d_k3_forward_compact_pre": (4, "p2pb_conv3d_active_lists", 1)}
QUERIES = ("_floats", "_bytes", "_slots", "_supported", "p2pb_get_split_terms", "p2pb_set_split_terms")


def digest(log):
    """the log as the strings TABLE holds: one per launch, sizes and addresses left out"""
    out, base = [], {}
    for name, row in log:
        if name.endswith(QUERIES):
            continue
        ints = [v for k, v in row if k == "i"]
        ptrs = [v for k, v in row if k == "p"]
        if name in ("p2pb_conv3d_brick_lists", "p2pb_conv3d_active_lists"):
            base[name] = ptrs[{"p2pb_conv3d_brick_lists": 2, "p2pb_conv3d_active_lists": 1}[name]]
        labels_i, labels_p = SPEC.get(name, ({}, {}))
        s = name[len("p2pb_"):]
        if name in LIST_ARG:
            at, maker, _ = LIST_ARG[name]
            assert maker in base, f"{name} reads lists that {maker} did not make"
            assert ptrs[at] >= base[maker]
            s += f" which={int(ptrs[at] != base[maker])}"
        s += "".join(f" {lab}={ints[i]}" for i, lab in sorted(labels_i.items()))
        s += "".join(f" +{lab}" for i, lab in sorted(labels_p.items()) if ptrs[i])
        out.append(s)
    return tuple(out)


TABLE = {
    'r4-f16x3-geo-compactdefault-sparse-se-adagn': (
        'voxel_coords', 'voxel_sort', 'pointwise_pack_weights_split', 'pointwise_conv_forward swish=0 flags=132', 'avg_voxelize_cl_gather',
        'conv3d_k3_pack_weights_split', 'conv3d_k3_forward_ex swish=0 flags=14', 'gn_affine_params +style', 'conv3d_k3_pack_weights_split',
        'conv3d_k3_forward_ex swish=1 flags=14 +in_scale', 'pvconv_tail +style +se +point', 'trilinear_devoxelize_cl_affine +add',
    ),
    'r4-f16x3-nogeo-compactdefault-sparse-se-adagn': (
        'pointwise_pack_weights_split', 'pointwise_conv_forward swish=0 flags=132', 'voxel_coords', 'avg_voxelize_cl_forward',
        'conv3d_k3_pack_weights_split', 'conv3d_k3_forward_ex swish=0 flags=14', 'gn_affine_params +style', 'conv3d_k3_pack_weights_split',
        'conv3d_k3_forward_ex swish=1 flags=14 +in_scale', 'pvconv_tail +style +se +point', 'trilinear_devoxelize_cl_affine +add',
    ),
    'r8-f16x3-geo-compactdefault-sparse-se-adagn': (
        'voxel_coords', 'voxel_sort', 'pointwise_pack_weights_split', 'pointwise_conv_forward swish=0 flags=132',
        'avg_voxelize_cl_gather_split', 'conv3d_k3_pack_weights_split', 'conv3d_k3_forward_ex swish=0 flags=30', 'gn_affine_params +style',
        'conv3d_presplit swish=1 +in_scale', 'conv3d_k3_pack_weights_split', 'conv3d_k3_forward_ex swish=0 flags=30',
        'pvconv_tail +style +se +point', 'trilinear_devoxelize_cl_affine +add',
    ),
    'r8-f16x3-nogeo-compactdefault-sparse-se-adagn': (
        'pointwise_pack_weights_split', 'pointwise_conv_forward swish=0 flags=132', 'voxel_coords', 'avg_voxelize_cl_forward',
        'conv3d_k3_pack_weights_split', 'conv3d_k3_forward_ex swish=0 flags=14', 'gn_affine_params +style', 'conv3d_k3_pack_weights_split',
        'conv3d_k3_forward_ex swish=1 flags=14 +in_scale', 'pvconv_tail +style +se +point', 'trilinear_devoxelize_cl_affine +add',
    ),
    'r16-f16x3-geo-compactdefault-sparse-se-adagn': (
        'voxel_coords', 'voxel_sort', 'conv3d_active_lists', 'pointwise_pack_weights_split', 'pointwise_conv_forward swish=0 flags=132',
        'avg_voxelize_cl_gather_split', 'conv3d_k3_pack_weights_split', 'conv3d_k3_forward_compact_pre which=0 flags=0',
        'conv3d_k3_pack_weights', 'conv3d_k3_far_field_gn swish=1 +style', 'conv3d_presplit swish=1 +in_scale +in_sub',
        'conv3d_k3_pack_weights_split', 'conv3d_k3_forward_compact_pre which=1 flags=32 +out_class', 'pvconv_tail +style +se +point',
        'trilinear_devoxelize_cl_affine +add',
    ),
    'r16-f16x3-nogeo-compactdefault-sparse-se-adagn': (
        'pointwise_pack_weights_split', 'pointwise_conv_forward swish=0 flags=132', 'voxel_coords', 'avg_voxelize_cl_forward',
        'conv3d_active_lists', 'conv3d_k3_pack_weights_split', 'conv3d_k3_forward_compact which=0 swish=0 flags=0',
        'conv3d_k3_pack_weights', 'conv3d_k3_far_field_gn swish=1 +style', 'conv3d_k3_pack_weights_split',
        'conv3d_k3_forward_compact which=1 swish=1 flags=32 +out_class +in_scale +in_sub', 'pvconv_tail +style +se +point',
        'trilinear_devoxelize_cl_affine +add',
    ),
    'r32-f16x3-geo-compactdefault-sparse-se-adagn': (
        'voxel_coords', 'voxel_sort', 'conv3d_brick_lists', 'pointwise_pack_weights_split', 'pointwise_conv_forward swish=0 flags=132',
        'avg_voxelize_cl_gather_split', 'conv3d_k3_pack_weights_split', 'conv3d_k3_forward_sparse which=0 swish=0 flags=28',
        'conv3d_k3_pack_weights', 'conv3d_k3_far_field_gn swish=1 +style', 'conv3d_k3_pack_weights_split',
        'conv3d_k3_forward_sparse which=1 swish=1 flags=44 +out_class +in_scale +in_sub', 'pvconv_tail +style +se +point',
        'trilinear_devoxelize_cl_affine +add',
    ),
    'r32-f16x3-nogeo-compactdefault-sparse-se-adagn': (
        'pointwise_pack_weights_split', 'pointwise_conv_forward swish=0 flags=132', 'voxel_coords', 'avg_voxelize_cl_forward',
        'conv3d_brick_lists', 'conv3d_k3_pack_weights_split', 'conv3d_k3_forward_sparse which=0 swish=0 flags=12', 'conv3d_k3_pack_weights',
        'conv3d_k3_far_field_gn swish=1 +style', 'conv3d_k3_pack_weights_split',
        'conv3d_k3_forward_sparse which=1 swish=1 flags=44 +out_class +in_scale +in_sub', 'pvconv_tail +style +se +point',
        'trilinear_devoxelize_cl_affine +add',
    ),
    'r16-bf16x6-geo-compactdefault-sparse-se-adagn': (
        'voxel_coords', 'voxel_sort', 'conv3d_active_lists', 'pointwise_pack_weights', 'pointwise_conv_forward swish=0 flags=0',
        'avg_voxelize_cl_gather', 'conv3d_k3_pack_weights_split', 'conv3d_k3_forward_compact which=0 swish=0 flags=0',
        'conv3d_k3_pack_weights', 'conv3d_k3_far_field_gn swish=1 +style', 'conv3d_k3_pack_weights_split',
        'conv3d_k3_forward_compact which=1 swish=1 flags=32 +out_class +in_scale +in_sub', 'pvconv_tail +style +se +point',
        'trilinear_devoxelize_cl_affine +add',
    ),
    'r32-bf16x6-geo-compactdefault-sparse-se-adagn': (
        'voxel_coords', 'voxel_sort', 'conv3d_brick_lists', 'pointwise_pack_weights', 'pointwise_conv_forward swish=0 flags=0',
        'avg_voxelize_cl_gather', 'conv3d_k3_pack_weights_split', 'conv3d_k3_forward_sparse which=0 swish=0 flags=12',
        'conv3d_k3_pack_weights', 'conv3d_k3_far_field_gn swish=1 +style', 'conv3d_k3_pack_weights_split',
        'conv3d_k3_forward_sparse which=1 swish=1 flags=44 +out_class +in_scale +in_sub', 'pvconv_tail +style +se +point',
        'trilinear_devoxelize_cl_affine +add',
    ),
    'r16-fp32-geo-compactdefault-sparse-se-adagn': (
        'voxel_coords', 'voxel_sort', 'pointwise_pack_weights', 'pointwise_conv_forward swish=0 flags=0', 'avg_voxelize_cl_gather',
        'conv3d_k3_pack_weights', 'conv3d_k3_forward_ex swish=0 flags=10', 'gn_affine_params +style', 'conv3d_k3_pack_weights',
        'conv3d_k3_forward_ex swish=1 flags=10 +in_scale', 'pvconv_tail +style +se +point', 'trilinear_devoxelize_cl_affine +add',
    ),
    'r32-fp32-geo-compactdefault-sparse-se-adagn': (
        'voxel_coords', 'voxel_sort', 'conv3d_brick_lists', 'pointwise_pack_weights', 'pointwise_conv_forward swish=0 flags=0',
        'avg_voxelize_cl_gather', 'conv3d_k3_pack_weights', 'conv3d_k3_forward_sparse which=0 swish=0 flags=8', 'conv3d_k3_pack_weights',
        'conv3d_k3_far_field_gn swish=1 +style', 'conv3d_k3_forward_sparse which=1 swish=1 flags=40 +out_class +in_scale +in_sub',
        'pvconv_tail +style +se +point', 'trilinear_devoxelize_cl_affine +add',
    ),
    'r16-f16x3-geo-compactoff-sparse-se-adagn': (
        'voxel_coords', 'voxel_sort', 'pointwise_pack_weights_split', 'pointwise_conv_forward swish=0 flags=132',
        'avg_voxelize_cl_gather_split', 'conv3d_k3_pack_weights_split', 'conv3d_k3_forward_ex swish=0 flags=30', 'gn_affine_params +style',
        'conv3d_presplit swish=1 +in_scale', 'conv3d_k3_pack_weights_split', 'conv3d_k3_forward_ex swish=0 flags=30',
        'pvconv_tail +style +se +point', 'trilinear_devoxelize_cl_affine +add',
    ),
    'r32-f16x3-geo-compact32,16:16-sparse-se-adagn': (
        'voxel_coords', 'voxel_sort', 'conv3d_active_lists', 'pointwise_pack_weights_split', 'pointwise_conv_forward swish=0 flags=132',
        'avg_voxelize_cl_gather_split', 'conv3d_k3_pack_weights_split', 'conv3d_k3_forward_compact_pre which=0 flags=0',
        'gn_affine_params +style', 'conv3d_k3_pack_weights_split', 'conv3d_k3_forward_ex swish=1 flags=14 +in_scale',
        'pvconv_tail +style +se +point', 'trilinear_devoxelize_cl_affine +add',
    ),
    'r8-f16x3-geo-compact8:8-sparse-se-adagn': (
        'voxel_coords', 'voxel_sort', 'conv3d_active_lists', 'pointwise_pack_weights_split', 'pointwise_conv_forward swish=0 flags=132',
        'avg_voxelize_cl_gather_split', 'conv3d_k3_pack_weights_split', 'conv3d_k3_forward_compact_pre which=0 flags=0',
        'conv3d_k3_pack_weights', 'conv3d_k3_far_field_gn swish=1 +style', 'conv3d_presplit swish=1 +in_scale +in_sub',
        'conv3d_k3_pack_weights_split', 'conv3d_k3_forward_compact_pre which=1 flags=32 +out_class', 'pvconv_tail +style +se +point',
        'trilinear_devoxelize_cl_affine +add',
    ),
    'r16-f16x3-geo-compactdefault-dense-se-adagn': (
        'voxel_coords', 'voxel_sort', 'conv3d_active_lists', 'pointwise_pack_weights_split', 'pointwise_conv_forward swish=0 flags=132',
        'avg_voxelize_cl_gather_split', 'conv3d_k3_pack_weights_split', 'conv3d_k3_forward_ex swish=0 flags=30', 'gn_affine_params +style',
        'conv3d_presplit swish=1 +in_scale', 'conv3d_k3_pack_weights_split', 'conv3d_k3_forward_ex swish=0 flags=30',
        'pvconv_tail +style +se +point', 'trilinear_devoxelize_cl_affine +add',
    ),
    'r32-f16x3-geo-compactdefault-dense-se-adagn': (
        'voxel_coords', 'voxel_sort', 'conv3d_brick_lists', 'pointwise_pack_weights_split', 'pointwise_conv_forward swish=0 flags=132',
        'avg_voxelize_cl_gather_split', 'conv3d_k3_pack_weights_split', 'conv3d_k3_forward_ex swish=0 flags=30', 'gn_affine_params +style',
        'conv3d_k3_pack_weights_split', 'conv3d_k3_forward_ex swish=1 flags=14 +in_scale', 'pvconv_tail +style +se +point',
        'trilinear_devoxelize_cl_affine +add',
    ),
    'r16-f16x3-geo-compactdefault-sparse-nose-adagn': (
        'voxel_coords', 'voxel_sort', 'conv3d_active_lists', 'pointwise_pack_weights_split', 'pointwise_conv_forward swish=0 flags=132',
        'avg_voxelize_cl_gather_split', 'conv3d_k3_pack_weights_split', 'conv3d_k3_forward_compact_pre which=0 flags=0',
        'conv3d_k3_pack_weights', 'conv3d_k3_far_field_gn swish=1 +style', 'conv3d_presplit swish=1 +in_scale +in_sub',
        'conv3d_k3_pack_weights_split', 'conv3d_k3_forward_compact_pre which=1 flags=32 +out_class', 'pvconv_tail +style +point',
        'trilinear_devoxelize_cl_affine +add',
    ),
    'r16-f16x3-geo-compactdefault-sparse-se-gn': (
        'voxel_coords', 'voxel_sort', 'conv3d_active_lists', 'pointwise_pack_weights_split', 'pointwise_conv_forward swish=0 flags=132',
        'avg_voxelize_cl_gather_split', 'conv3d_k3_pack_weights_split', 'conv3d_k3_forward_compact_pre which=0 flags=0',
        'conv3d_k3_pack_weights', 'conv3d_k3_far_field_gn swish=1', 'conv3d_presplit swish=1 +in_scale +in_sub',
        'conv3d_k3_pack_weights_split', 'conv3d_k3_forward_compact_pre which=1 flags=32 +out_class', 'pvconv_tail +se +point',
        'trilinear_devoxelize_cl_affine +add',
    ),
    'r32-f16x3-geo-compactdefault-sparse-nose-gn': (
        'voxel_coords', 'voxel_sort', 'conv3d_brick_lists', 'pointwise_pack_weights_split', 'pointwise_conv_forward swish=0 flags=132',
        'avg_voxelize_cl_gather_split', 'conv3d_k3_pack_weights_split', 'conv3d_k3_forward_sparse which=0 swish=0 flags=28',
        'conv3d_k3_pack_weights', 'conv3d_k3_far_field_gn swish=1', 'conv3d_k3_pack_weights_split',
        'conv3d_k3_forward_sparse which=1 swish=1 flags=44 +out_class +in_scale +in_sub', 'pvconv_tail +point',
        'trilinear_devoxelize_cl_affine +add',
    ),
    'r8-f16x3-geo-compactdefault-sparse-nose-gn': (
        'voxel_coords', 'voxel_sort', 'pointwise_pack_weights_split', 'pointwise_conv_forward swish=0 flags=132',
        'avg_voxelize_cl_gather_split', 'conv3d_k3_pack_weights_split', 'conv3d_k3_forward_ex swish=0 flags=30', 'gn_affine_params',
        'conv3d_presplit swish=1 +in_scale', 'conv3d_k3_pack_weights_split', 'conv3d_k3_forward_ex swish=0 flags=30', 'pvconv_tail +point',
        'trilinear_devoxelize_cl_affine +add',
    ),
    'r16-f16x3-geo-compactdefault-sparse-se-adagn-pin0': (
        'voxel_coords', 'voxel_sort', 'conv3d_active_lists', 'pointwise_pack_weights_split', 'pointwise_conv_forward swish=0 flags=132',
        'avg_voxelize_cl_gather', 'set_split_terms_thread terms=6', 'conv3d_k3_pack_weights_split',
        'conv3d_k3_forward_compact which=0 swish=0 flags=0', 'set_split_terms_thread terms=0', 'conv3d_k3_pack_weights',
        'conv3d_k3_far_field_gn swish=1 +style', 'conv3d_presplit swish=1 +in_scale +in_sub', 'conv3d_k3_pack_weights_split',
        'conv3d_k3_forward_compact_pre which=1 flags=32 +out_class', 'pvconv_tail +style +se +point', 'trilinear_devoxelize_cl_affine +add',
    ),
    'r16-f16x3-geo-compactdefault-sparse-se-adagn-pin4': (
        'voxel_coords', 'voxel_sort', 'conv3d_active_lists', 'pointwise_pack_weights_split', 'pointwise_conv_forward swish=0 flags=132',
        'avg_voxelize_cl_gather_split', 'conv3d_k3_pack_weights_split', 'conv3d_k3_forward_compact_pre which=0 flags=0',
        'conv3d_k3_pack_weights', 'conv3d_k3_far_field_gn swish=1 +style', 'set_split_terms_thread terms=6', 'conv3d_k3_pack_weights_split',
        'conv3d_k3_forward_compact which=1 swish=1 flags=32 +out_class +in_scale +in_sub', 'set_split_terms_thread terms=0',
        'pvconv_tail +style +se +point', 'trilinear_devoxelize_cl_affine +add',
    ),
}


def test_table_lists_the_cases():
    assert set(TABLE) == {_cid(c) for c in CASES} and len(TABLE) == len(CASES)


@pytest.mark.parametrize("c", CASES, ids=_cid)
def test_pvconv_dispatch(c, monkeypatch):
    out, log = run_case(c, monkeypatch)
    got = digest(log)
    print(f"RECORDED {_cid(c)!r}: (\n" + "".join(f"    {s!r},\n" for s in got) + "),")
    assert torch.isfinite(out).all()
    assert got == TABLE[_cid(c)]
