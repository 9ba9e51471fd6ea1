"""The packed-batch surface (`pointops_cuda`, `pointops`, `chamfer`) without a GPU: every name exists, none has a CPU path,
and install_dropin() registers the two modules."""
import sys

import pytest
import torch

F32, I32 = torch.float32, torch.int32
B, N, M, C, WC, U, K = 2, 16, 6, 4, 2, 3, 3


def z(*shape, dtype=F32):
    return torch.zeros(*shape, dtype=dtype)


# the 11 own names -> arguments in the reference's pybind order, on the CPU
CALLS = {
    "knnquery_cuda": (M, U, z(N, 3), z(M, 3), z(B, dtype=I32), z(B, dtype=I32), z(M, U, dtype=I32), z(M, U)),
    "ballquery_cuda": (M, 0.5, U, z(N, 3), z(M, 3), z(B, dtype=I32), z(B, dtype=I32), z(M, U, dtype=I32)),
    "furthestsampling_cuda": (B, N, z(N, 3), z(B, dtype=I32), z(B, dtype=I32), z(N), z(M, dtype=I32)),
    "grouping_forward_cuda": (M, U, C, z(N, C), z(M, U, dtype=I32), z(M, U, C)),
    "grouping_backward_cuda": (M, U, C, z(M, U, C), z(M, U, dtype=I32), z(N, C)),
    "interpolation_forward_cuda": (N, C, K, z(M, C), z(N, K, dtype=I32), z(N, K), z(N, C)),
    "interpolation_backward_cuda": (N, C, K, z(N, C), z(N, K, dtype=I32), z(N, K), z(M, C)),
    "subtraction_forward_cuda": (N, U, C, z(N, C), z(N, C), z(N, U, dtype=I32), z(N, U, C)),
    "subtraction_backward_cuda": (N, U, C, z(N, U, dtype=I32), z(N, U, C), z(N, C), z(N, C)),
    "aggregation_forward_cuda": (N, U, C, WC, z(N, C), z(N, U, C), z(N, U, WC), z(N, U, dtype=I32), z(N, C)),
    "aggregation_backward_cuda": (N, U, C, WC, z(N, C), z(N, U, C), z(N, U, WC), z(N, U, dtype=I32), z(N, C), z(N, C),
                                  z(N, U, C), z(N, U, WC)),
}
# third_party/openpoints/cpp/pointops/src/pointops_api.cpp:15-27
REFERENCE_NAMES = sorted(CALLS) + ["avg_voxelize_backward", "avg_voxelize_forward"]


def test_the_13_names_exist():
    from p2p_bridge_amd import pointops_cuda as ext

    assert len(REFERENCE_NAMES) == 13
    for name in REFERENCE_NAMES:
        assert callable(getattr(ext, name)), name
    assert sorted(ext.__all__) == sorted(REFERENCE_NAMES)


@pytest.mark.parametrize("name", sorted(CALLS))
def test_wrapper_refuses_cpu_tensors(name):
    from p2p_bridge_amd import pointops_cuda as ext

    args = tuple(a.fill_(3) if torch.is_tensor(a) else a for a in CALLS[name])
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        getattr(ext, name)(*args)
    for t in args:
        if torch.is_tensor(t):
            assert bool((t == 3).all())  # nothing was computed on the host


def test_voxelize_names_are_the_ones_already_served():
    from p2p_bridge_amd import pointnet2_batch_cuda, pointops_cuda

    assert pointops_cuda.avg_voxelize_forward is pointnet2_batch_cuda.avg_voxelize_forward
    assert pointops_cuda.avg_voxelize_backward is pointnet2_batch_cuda.avg_voxelize_backward
    with pytest.raises(RuntimeError):
        pointops_cuda.avg_voxelize_forward(z(1, 2, 16), z(1, 3, 16, dtype=I32), 4)


def test_chamfer_module_refuses_cpu_tensors():
    from p2p_bridge_amd.metric_modules import chamfer

    a, b = z(1, 8, 3).fill_(3), z(1, 5, 3).fill_(3)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        chamfer.forward(a, b)
    i1, i2, g1, g2 = z(1, 8, dtype=I32), z(1, 5, dtype=I32), z(1, 8).fill_(3), z(1, 5).fill_(3)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        chamfer.backward(a, b, i1, i2, g1, g2)
    for t in (a, b, g1, g2):
        assert bool((t == 3).all())
    assert not i1.any() and not i2.any()
    assert sorted(k for k in vars(chamfer) if not k.startswith("__")) == ["backward", "forward"]


def test_layer_api_names_and_no_cpu_path():
    from p2p_bridge_amd import metrics, pointops

    for name in ("FurthestSampling", "KNNQuery", "BallQuery", "Grouping", "Subtraction", "Aggregation", "Interpolation"):
        assert issubclass(getattr(pointops, name), torch.autograd.Function), name
    for name in ("furthestsampling", "knnquery", "ballquery", "grouping", "subtraction", "aggregation", "interpolation2",
                 "querygroup", "queryandgroup", "interpolation"):
        assert callable(getattr(pointops, name)), name
    assert issubclass(metrics.ChamferFunction, torch.autograd.Function)
    for name in ("ChamferDistanceL2", "ChamferDistanceL2_split", "ChamferDistanceL1"):
        layer = getattr(metrics, name)(ignore_zeros=True)
        assert isinstance(layer, torch.nn.Module) and layer.ignore_zeros is True
        with pytest.raises(RuntimeError):
            layer(z(1, 8, 3), z(1, 5, 3))
    offset, new_offset = torch.tensor([10, N], dtype=I32), torch.tensor([2, M], dtype=I32)
    with pytest.raises(RuntimeError):
        pointops.knnquery(U, z(N, 3), None, offset, offset)
    with pytest.raises(ValueError):  # neither nsample nor idx: nothing to group by
        pointops.querygroup(None, z(N, 3), None, z(N, C), offset, offset)
    with pytest.raises(RuntimeError):
        pointops.furthestsampling(z(N, 3), offset, new_offset)
    with pytest.raises(RuntimeError):
        pointops.grouping(z(N, C).requires_grad_(), z(M, U, dtype=I32))


def test_install_dropin_registers_pointops_cuda_and_chamfer():
    import p2p_bridge_amd

    p2p_bridge_amd.install_dropin()
    import chamfer
    import pointops_cuda

    assert sys.modules["pointops_cuda"] is pointops_cuda and sys.modules["chamfer"] is chamfer
    assert sorted(k for k in vars(pointops_cuda) if not k.startswith("__")) == sorted(REFERENCE_NAMES)
    assert callable(chamfer.forward) and callable(chamfer.backward)
    for name in ("pointnet2_batch_cuda", "_pvcnn_backend", "chamfer_3D", "emd_cuda", "emd_assignment"):
        assert name in sys.modules, name  # (the five registered before are still there)
