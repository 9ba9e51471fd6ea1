"""Error behaviour at the C ABI (include/p2pb_hip.h: "0 on success, P2PB_EINVAL (-22) for unsupported arguments, else the
hipError_t of the failed launch"; the reference exit(-1)s on a failed launch, PN2/cuda_utils.cuh:30-39, and its Python
side raises RuntimeError on non-CUDA / non-contiguous / wrong-dtype tensors, PN2/utils.hpp:7-18): every entry point
rejects degenerate sizes and missing workspaces with -22 WITHOUT launching anything, the ctypes layer turns that into
P2PBError (a RuntimeError), the tensor preconditions raise RuntimeError -- and the device is still healthy afterwards."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
_i, _f = ctypes.c_int, ctypes.c_float
NULL = ctypes.c_void_p(0)


@pytest.fixture(scope="module")
def L():
    from p2p_bridge_amd import _lib
    return _lib


def _pointwise_refusals(p, q, s):
    """one row per P2PB_EINVAL condition of the pointwise entry points (csrc/pointwise.hip, pointwise_act.hip): (entry point,
    arithmetic of the calling thread, arguments). Every row is otherwise well-formed -- b = 1, 8 -> 8 channels (8 -> 16 for the gather
    form), 8 positions, p a 16-byte aligned buffer -- so the one condition it names is what refuses it; q = p + 4 bytes."""
    F16, BF6, BF3 = 16, 6, 3
    d = ctypes.c_double
    no_fin = (d(0.0), _i(0), NULL, NULL, NULL, _i(0), _f(0.0), NULL, NULL, NULL)
    bad_fin = (d(4.0), _i(5), NULL, NULL, NULL, _i(0), _f(1e-5), p, p, NULL)  # 16 % 5 != 0: gn_shape_ok refuses

    def conv(npos=8, x=p, xf=NULL, flags=0, out=p, st=NULL):
        return (_i(1), _i(8), _i(8), _i(npos), x, p, p, NULL, xf, xf, _i(0), _i(flags), out, st, *no_fin, s)

    def pool(npos=8, x=p, flags=0, st=p, u=4, mm=p):
        return (_i(1), _i(8), _i(8), _i(npos), x, p, p, NULL, NULL, NULL, _i(0), _i(flags), p, st, _i(u), mm, *no_fin, s)

    def gather(cin=8, u=4, zt=p, idx=p, xf=p, fin=no_fin):
        return (_i(1), _i(cin), _i(16), _i(16), _i(4), _i(u), zt, p, idx, p, p, xf, xf, _i(0), p, p, *fin, s)

    def pool_gn(c=8, groups=4, scale=p):
        return (_i(1), _i(c), _i(4), p, p, _i(4), d(4.0), _i(groups), NULL, NULL, NULL, _i(0), _f(1e-5), _i(1), scale, p, p, s)

    cf, cp, cg, mg = ("p2pb_pointwise_conv_forward", "p2pb_pointwise_conv_pool_forward", "p2pb_pointwise_conv_pool_gather",
                      "p2pb_minmax_act_pool_gn")
    return [
        (cf, F16, conv(out=NULL)),
        (cf, F16, conv(flags=32, st=p)),            # point-major output has no statistics
        (cf, F16, conv(flags=4, npos=6)),           # the split pack needs rows of whole quads ...
        (cf, F16, conv(flags=4, x=q)),              # ... that start on 16-byte boundaries
        (cf, F16, conv(flags=4 | 128, npos=6)),
        (cf, BF6, conv(flags=4 | 128)),             # the wide tiling on the split pack exists in f16x3 only
        (cf, F16, conv(flags=32, npos=6)),          # fp32 pack: the unaligned fallback has no point-major form
        (cf, BF3, conv(flags=4, xf=p)),             # bf16x3: plain operand ...
        (cf, BF3, conv(flags=4 | 32)),              # ... and channel-major output only
        (cp, F16, pool(mm=NULL)),
        (cp, F16, pool(st=NULL)),
        (cp, F16, pool(u=5)),
        (cp, F16, pool(npos=12, u=8)),              # npos % pool_u
        (cp, F16, pool(npos=6, u=0)),               # npos % 4
        (cp, F16, pool(x=q)),
        (cp, BF3, pool(flags=4)),                   # bf16x3 has no pooling epilogue
        (cg, F16, gather(cin=12)),                  # cin % 8
        (cg, F16, gather(u=0)),
        (cg, F16, gather(idx=NULL)),
        (cg, F16, gather(xf=NULL)),
        (cg, F16, gather(zt=q)),
        (cg, BF6, gather()),                        # the gathered form exists in f16x3 only
        (cg, F16, gather(fin=bad_fin)),
        (mg, F16, pool_gn(c=10)),                   # c % groups
        (mg, F16, pool_gn(c=8192, groups=32)),      # c > 4096
        (mg, F16, pool_gn(scale=NULL)),
    ]


def test_degenerate_sizes_are_einval(L):
    lib = L.lib()
    x = torch.zeros(64, device="cuda")
    p = L.ptr(x)
    s = L.stream_ptr()
    no_fin = (ctypes.c_double(0.0), _i(0), NULL, NULL, NULL, _i(0), _f(0.0), NULL, NULL, NULL)  # fin_scale == NULL: no finisher
    calls = {
        "p2pb_furthest_point_sampling": (_i(0), _i(8), _i(2), p, NULL, p, s),
        "p2pb_furthest_point_sampling_grid": (_i(1), _i(8), _i(2), p, NULL, p, s),          # no workspace
        "p2pb_furthest_point_sampling_coop": (_i(1), _i(100), _i(2), p, p, p, s),             # n <= 16384
        "p2pb_ball_query": (_i(1), _i(0), _i(4), _f(0.1), _i(8), p, p, p, s),
        "p2pb_chamfer_forward": (_i(0), _i(4), _i(4), p, p, p, p, p, p, s),
        "p2pb_conv3d_k3_forward": (_i(1), _i(0), _i(8), _i(8), p, p, p, NULL, NULL, _i(0), p, NULL, s),
        "p2pb_conv3d_k3_forward_ex": (_i(1), _i(8), _i(8), _i(5), p, p, p, NULL, NULL, NULL, _i(0), NULL, _i(4), p, NULL, s),  # r = 5
        "p2pb_pointwise_conv_forward": (_i(1), _i(8), _i(8), _i(0), p, p, p, NULL, NULL, NULL, _i(0), _i(0), p, NULL, *no_fin, s),
        "p2pb_gn_affine_params": (_i(1), _i(12), _i(5), _i(1), ctypes.c_double(4.0), p, NULL, NULL, NULL, _i(0), _f(1e-5), p, p, NULL, s),  # 12 % 5
        "p2pb_radius_count": (_i(1), _i(4), p, p, _f(-1.0), p, s),                             # negative radius
        "p2pb_linear_attention_forward": (_i(1), _i(2), _i(16), _i(8), p, p, NULL, s),        # dim_head != 32
        "p2pb_knn_points": (_i(1), _i(1), _i(4), _i(9), p, p, p, p, NULL, p, s),              # k > n
        "p2pb_three_nn": (_i(1), _i(0), _i(4), p, p, p, p, s),
        # round 6: the training step's folded entry points
        "p2pb_affine_act_train": (_i(1), _i(8), _i(8), p, p, p, _i(1), NULL, NULL, _f(0.1), NULL, ctypes.c_uint(1), p, s),  # dropout without a seed
        "p2pb_grouping_backward_pitched": (_i(1), _i(2), _i(8), _i(2), _i(2), p, ctypes.c_long(7), p, p, s),           # pitch < c*m*u
        "p2pb_three_nn_interpolate_backward_pitched": (_i(1), _i(2), _i(8), _i(4), p, ctypes.c_long(15), p, p, p, s),  # pitch < c*n
    }
    nab = lambda **k: (_i(1), _i(8), _i(2), _i(8), p, p, p, p, p, NULL, NULL, NULL, _i(0), _i(k.get("swish", 0)),  # noqa: E731
                       ctypes.c_long(k.get("pitch", 0)), k.get("gmean", NULL), k.get("res", NULL), k.get("rgate", NULL),
                       _f(k.get("drop", 0.0)), k.get("seed", NULL), ctypes.c_uint(0), p, NULL, NULL, NULL, k.get("dres", NULL),
                       k.get("drgate", NULL), p, s)
    for bad in (dict(drop=1.0, seed=p), dict(drop=0.2), dict(gmean=p, swish=1), dict(gmean=p, drop=0.1, seed=p), dict(pitch=63),
                dict(pitch=66), dict(dres=p, drgate=p), dict(res=p, rgate=p, dres=p)):
        assert lib.p2pb_norm_act_backward_ex(*nab(**bad)) == -22, bad
    # the GroupNorm finisher of the pointwise entry points is checked before the producer is launched (b, cin, cout, npos; stats;
    # groups; style, stride): no statistics to finish, 12 % 5, a style row shorter than 2 * cout
    pwf = lambda co, st, groups, style, stride: (_i(1), _i(8), _i(co), _i(4), p, p, p, NULL, NULL, NULL, _i(0), _i(0), p, st,  # noqa: E731
                                                 ctypes.c_double(4.0), _i(groups), NULL, NULL, style, _i(stride), _f(1e-5), p, p, NULL, s)
    for k, bad in enumerate(((8, NULL, 4, NULL, 0), (12, p, 5, NULL, 0), (8, p, 4, p, 15))):
        assert lib.p2pb_pointwise_conv_forward(*pwf(*bad)) == -22, k
    for name, args in calls.items():
        rc = getattr(lib, name)(*args)
        assert rc == -22, (name, rc)
    try:
        for k, (name, terms, args) in enumerate(_pointwise_refusals(p, L.ptr(x[1:]), s)):
            assert lib.p2pb_set_split_terms_thread(terms) == 0
            rc = getattr(lib, name)(*args)
            assert rc == -22, (k, name, rc)
    finally:
        lib.p2pb_set_split_terms_thread(0)
    with pytest.raises(L.P2PBError):
        L.call("p2pb_furthest_point_sampling", _i(0), _i(8), _i(2), p, NULL, p, s)
    assert issubclass(L.P2PBError, RuntimeError)
    torch.cuda.synchronize()  # nothing was launched, nothing is pending
    assert float((torch.ones(4, device="cuda") * 2).sum()) == 8.0


def test_tensor_preconditions_raise_runtime_error():
    from p2p_bridge_amd import pointnet2_batch_cuda as ext

    c = torch.rand(2, 3, 64, device="cuda")
    with pytest.raises(RuntimeError, match="CUDA"):
        ext.furthest_point_sampling_forward(c.cpu(), 8)
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.furthest_point_sampling_forward(c.transpose(1, 2).contiguous().transpose(1, 2), 8)
    with pytest.raises(RuntimeError, match="float"):
        ext.furthest_point_sampling_forward(c.double(), 8)
    assert ext.furthest_point_sampling_forward(c, 8).shape == (2, 8)


# (b, cin, cout, r | npos) -> K-splits under math 0 and 1 (bf16x3, bf16x6), under math 2 (exact fp32)
_WGRAD_CONV_SPLITS = {(8, 64, 64, 32): (113, 113), (8, 128, 64, 16): (56, 56), (8, 256, 256, 8): (7, 7), (2, 8, 16, 4): (8, 2),
                      (1, 8, 16, 4): (4, 1), (2, 512, 512, 8): (1, 1), (3, 3, 70, 8): (48, 6), (64, 256, 256, 32): (7, 7),
                      (2, 35, 32, 32): (170, 192)}
_WGRAD_PW_SPLITS = {(2, 3, 128, 1000): (32, 8), (2, 512, 1024, 2048): (4, 4), (2, 67, 64, 333): (42, 4), (2, 64, 64, 17): (4, 2),
                    (1, 256, 384, 8): (1, 1), (8, 128, 3, 2048): (192, 64), (2, 1024, 1024, 128): (2, 2), (1, 64, 64, 3): (1, 1)}


def test_wgrad_plan(L):
    """The workspace of a dense weight gradient (csrc/wgrad.hip: conv_wgrad_plan, pw_wgrad_plan) is whole partial rows -- cout * cin *
    taps weights + cout bias sums -- one per K-split. The split counts are pinned for every limit of the plan (the chip-filling
    target, the 48 MB of partials, the K units of the form that runs, the cap of 192) under the three kernel forms: host-only
    calls, nothing is launched."""
    lib = L.lib()
    for name, taps, table in (("p2pb_conv3d_k3_wgrad_ws_floats", 27, _WGRAD_CONV_SPLITS),
                              ("p2pb_pointwise_wgrad_ws_floats", 1, _WGRAD_PW_SPLITS)):
        for (b, cin, cout, n), (ns_bf16, ns_fp32) in table.items():
            row = cout * cin * taps + cout
            for math, ns in ((0, ns_bf16), (1, ns_bf16), (2, ns_fp32)):
                floats = getattr(lib, name)(_i(b), _i(cin), _i(cout), _i(n), _i(math))
                assert floats % row == 0 and floats // row == ns, (name, b, cin, cout, n, math, floats / row)
